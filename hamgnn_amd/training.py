"""The training step: what the reference's Lightning `training_step` + `loss.backward()` do per batch (hamgnn/main.py:389-420,
hamgnn/models/Model.py:150-196), on the HIP kernels and without an autograd graph.

  training_step(model, batch, ...)   forward with the layer inputs kept -> loss(es) -> head backward -> backbone backward -> `.grad` of EVERY
                                     parameter in the reference's names / flat layouts (any torch optimiser steps them); both backbones
                                     (HamGNNConvE3, HamGNNTransformer), the non-SOC / SOC so3 / SOC su2 heads, `losses=[{metric, prediction:
                                     hamiltonian | hamiltonian_real | hamiltonian_imag | band_energy | band_gap | overlap, target, loss_weight}]` as in
                                     the reference's config (metric: mae | mse | rmse | cosine_similarity | euclidean_loss | sum_zero,
                                     hamgnn/utils/losses.py); hamiltonian-type losses are multiplied by the head's `sparsity_ratio` as the reference
                                     does (Model.py:158-162), `overlap` (a ham_only=False head) and the k-space losses are not; `band_energy` and
                                     `band_gap` of one step share one eigen-chain per crystal (kspace.band_energy_backward).  `wavefunction` and
                                     `peak` are not built: the reference's own config names a metric for them that its parser lacks, and no head emits `peak`
  head_training_step(...)            the cheap variant for a frozen backbone (its representation can be reused across steps)
  allreduce_gradients(model)         data-parallel training (the reference's DDP): mean of the ranks' gradients, one flat bucket
  parallel.shard_graph(g, r, w)      model-parallel training of ONE large crystal: pass the rank's shard to training_step -- node-level partial
                                     sums are all-reduced inside the backward, per-edge parameter gradients summed over the ranks; the `losses` list
                                     works on a shard too (row losses: on-site rows once + the ranks' off-site rows; band_energy / band_gap: H(k) and
                                     S(k) summed over the ranks, the k-points dealt to them -- kspace.py)
  weights_changed(model)             after `optimizer.step()`: message blocks repack their weights on the device at the next forward
                                     (hamgnn_amd/repack.py); training_step calls it for the step that follows

No Lightning loop, no scheduler / logging / checkpoint policy: the caller owns those (`Model.save_checkpoint` writes the reference's layout)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import parallel
from .topo import gget


def _loss_and_grad(pred: torch.Tensor, target: torch.Tensor, metric: str):
    """(loss, d loss / d pred) of the reference's metrics (hamgnn/utils/losses.py; parse_metric_func): mae | mse | rmse element-wise, and the
    three row-wise ones with the reference's axes -- cosine_similarity = mean(1 - <p, t> / (|p| |t|)) and euclidean_loss = mean |p - t|_2 with
    the products / norms over the LAST axis and the mean over all others (a 1-D prediction is one row); sum_zero = |sum over axis 0 of p|_2
    over the last axis (the target is not read; a 1-D prediction gives |sum p|; beyond 2-D the reference's expression is not a scalar)"""
    metric = metric.lower()
    if metric in ("cosine_similarity", "euclidean_loss", "sum_zero"):
        if metric == "sum_zero":
            if pred.dim() > 2:
                raise ValueError("sum_zero: the reference's expression is a scalar for 1-D and 2-D predictions only")
            p2 = pred.reshape(pred.shape[0], -1) if pred.dim() else pred.reshape(1, 1)
            v = p2.sum(0)
            nv = torch.linalg.vector_norm(v)
            return nv, (v / nv.clamp_min(1e-30)).expand_as(p2).reshape(pred.shape)
        p2 = pred.reshape(-1, pred.shape[-1]) if pred.dim() else pred.reshape(1, 1)
        t2 = target.reshape(p2.shape)
        rows = p2.shape[0]
        if metric == "euclidean_loss":
            d = p2 - t2
            nd = torch.linalg.vector_norm(d, dim=1, keepdim=True)
            return nd.mean(), (d / (rows * nd.clamp_min(1e-30))).reshape(pred.shape)
        npd, ntg = torch.linalg.vector_norm(p2, dim=1, keepdim=True), torch.linalg.vector_norm(t2, dim=1, keepdim=True)
        cos = (p2 * t2).sum(1, keepdim=True) / (npd * ntg)
        return (1.0 - cos).mean(), (-(t2 / (npd * ntg) - cos * p2 / (npd * npd)) / rows).reshape(pred.shape)
    diff = pred - target
    n = diff.numel()
    if metric == "mae":
        return diff.abs().mean(), torch.sign(diff) / n
    if metric == "mse":
        return (diff * diff).mean(), 2.0 * diff / n
    if metric == "rmse":
        rm = torch.sqrt((diff * diff).mean())
        return rm, diff / (n * rm.clamp_min(1e-30))
    raise ValueError(f"unsupported loss metric {metric!r} (mae | mse | rmse | cosine_similarity | euclidean_loss | sum_zero)")


def _loss_and_grad_sharded(pred, target, metric: str, n_on: int):
    """the element-wise metrics (mae | mse | rmse) over [replicated on-site rows; this rank's off-site rows] of an edge-sharded crystal == the
    loss of the whole crystal: the off-site sums are added up over the ranks, the on-site rows counted once"""
    import torch.distributed as dist
    diff = pred - target
    metric = metric.lower()
    f = {"mae": torch.abs, "mse": torch.square, "rmse": torch.square}.get(metric)
    if f is None:
        raise ValueError(f"unsupported loss metric {metric!r} (mae | mse | rmse)")
    stats = torch.stack([f(diff[n_on:]).sum().double(), torch.tensor(float(diff[n_on:].numel()), dtype=torch.float64, device=diff.device)])
    dist.all_reduce(stats, op=dist.ReduceOp.SUM)
    n = float(stats[1]) + diff[:n_on].numel()
    total = (stats[0] + f(diff[:n_on]).sum().double()) / n
    if metric == "mae":
        return total.to(pred.dtype), torch.sign(diff) / n
    if metric == "mse":
        return total.to(pred.dtype), 2.0 * diff / n
    rm = torch.sqrt(total)
    return rm.to(pred.dtype), diff / (n * rm.clamp_min(1e-30).to(pred.dtype))


def _row_loss_and_grad_sharded(pred, target, metric: str, n_on: int):
    """every metric of _loss_and_grad on the rows of an edge-sharded crystal, i.e. _loss_and_grad on [on-site rows once; all ranks' off-site
    rows] (the formulas of hamgnn/utils/losses.py): the element-wise metrics through _loss_and_grad_sharded; the row-wise ones reduce their
    per-row statistics in one small all-reduce -- the sum of the off-site rows' 1 - cos or |p - t|_2 and the row count; sum_zero the column
    sums of the off-site rows."""
    import torch.distributed as dist
    metric = metric.lower()
    if metric not in ("cosine_similarity", "euclidean_loss", "sum_zero"):
        if metric not in ("mae", "mse", "rmse"):
            raise ValueError(f"unsupported loss metric {metric!r} (mae | mse | rmse | cosine_similarity | euclidean_loss | sum_zero)")
        return _loss_and_grad_sharded(pred, target, metric, n_on)
    if pred.dim() != 2:
        raise ValueError(f"{metric} on an edge-sharded graph: [rows, columns] predictions (the Hamiltonian / overlap rows)")
    if metric == "sum_zero":
        part = pred[n_on:].sum(0).double()
        dist.all_reduce(part, op=dist.ReduceOp.SUM)
        v = (part + pred[:n_on].sum(0).double()).to(pred.dtype)
        nv = torch.linalg.vector_norm(v)
        return nv, (v / nv.clamp_min(1e-30)).expand_as(pred)
    t2 = target.reshape(pred.shape)
    if metric == "euclidean_loss":
        d = pred - t2
        per_row = torch.linalg.vector_norm(d, dim=1, keepdim=True)
    else:
        npd, ntg = torch.linalg.vector_norm(pred, dim=1, keepdim=True), torch.linalg.vector_norm(t2, dim=1, keepdim=True)
        cos = (pred * t2).sum(1, keepdim=True) / (npd * ntg)
        per_row = 1.0 - cos
    stats = torch.stack([per_row[n_on:].sum().double(), torch.tensor(float(pred.shape[0] - n_on), dtype=torch.float64, device=pred.device)])
    dist.all_reduce(stats, op=dist.ReduceOp.SUM)
    rows = float(stats[1]) + n_on
    total = ((stats[0] + per_row[:n_on].sum().double()) / rows).to(pred.dtype)
    if metric == "euclidean_loss":
        return total, d / (rows * per_row.clamp_min(1e-30))
    return total, -(t2 / (npd * ntg) - cos * pred / (npd * npd)) / rows


def _sparsity_weighted(out, loss, grad):
    """the reference multiplies every hamiltonian / hamiltonian_real / hamiltonian_imag loss by predictions['sparsity_ratio'] whenever the
    head emits it (hamgnn/models/Model.py:158-162; calculate_sparsity=True is the default of the head)"""
    sr = out.get("sparsity_ratio") if hasattr(out, "get") else None
    if sr is None:
        return loss, grad
    sr = sr.to(loss.dtype)
    return loss * sr, grad * sr


@torch.no_grad()
def head_training_step(model, batch, metric: str = "mae", target: Optional[torch.Tensor] = None,
                       representation=None) -> Dict[str, torch.Tensor]:
    """One loss / gradient evaluation for the head of `model` (hamgnn_amd.models.model.Model): forward, loss(hamiltonian, target),
    backward through the head on the GPU kernels, `.grad` of every head parameter set (accumulated if already present).  The caller owns
    the optimiser: `opt.step(); opt.zero_grad()` -- the head repacks its weights on the next forward.
    representation: reuse a frozen backbone's output for this batch (it does not change while only the head is trained)."""
    head = model.output_module
    rep = representation if representation is not None else model.representation(batch)
    out = head(batch, rep)
    tgt = target if target is not None else gget(batch, "hamiltonian")
    if tgt is None:
        raise ValueError("head_training_step: the batch carries no target (Hon / Hoff or hamiltonian)")
    H = out["hamiltonian"]
    loss, gH = _loss_and_grad(H, tgt.to(H.dtype), metric)
    loss, gH = _sparsity_weighted(out, loss, gH)
    g_node, g_edge, grads = head.backward(batch, rep, gH)
    params = dict(head.named_parameters())
    for k, g in grads.items():
        p = params[k]
        g = g.reshape(p.shape).to(p.dtype)
        p.grad = g.clone() if p.grad is None else p.grad + g
    _invalidate(head)                                          # the packed weight fragments are stale once the optimiser has stepped
    return {"loss": loss, "representation": rep, "g_node_planar": g_node, "g_edge_planar_rot": g_edge}


def _sharded_sparsity_ratio(head, batch):
    """calculate_sparsity_ratio of the whole crystal from its shards: on-site rows once, off-site counts summed over the ranks"""
    import torch.distributed as dist
    z = batch.z
    n2 = head.nao_max ** 2
    src, dst = batch.edge_index
    ni = head._norb[z]
    both = head._defined[z[src]] & head._defined[z[dst]]
    off = torch.stack([torch.where(both, ni[src] * ni[dst], torch.full_like(src, n2)).sum().double(),
                       torch.tensor(float(src.numel()), dtype=torch.float64, device=z.device)])
    dist.all_reduce(off, op=dist.ReduceOp.SUM)
    eff = (ni * ni).sum().double() + off[0]
    total = (z.numel() + off[1]) * n2
    return (total / eff).to(torch.float32)


def weights_changed(model):
    """call after the optimiser stepped (training_step does it for the step that follows): the backbone's message blocks repack their
    weights on the device, everything else is dropped and repacked by the next forward"""
    rep = getattr(model, "representation", None)
    if rep is not None and hasattr(rep, "refresh_weights"):
        _invalidate(model.output_module)
        rep.refresh_at_next_forward()                          # the optimiser steps AFTER training_step returns
    else:
        _invalidate(model)


def allreduce_gradients(model, average: bool = True):
    """Data-parallel training (the reference's DDP, hamgnn/main.py:318-321: every rank steps the same model on its own batches): average the
    `.grad` of all parameters over the ranks of the default process group -- ONE flat bucket, i.e. one RCCL all-reduce per step (xGMI
    rings are per-link bound: few large collectives; the whole set-A model is 30 MB of fp32 gradients).  A no-op without an initialised
    process group or with one rank.  Parameters without a gradient on this rank contribute zeros."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    params = [p for p in model.parameters() if p.requires_grad]
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in params])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    if average:
        flat /= dist.get_world_size()
    o = 0
    for p in params:
        n = p.numel()
        p.grad = flat[o:o + n].reshape(p.shape).to(p.dtype)
        o += n


def _invalidate(module):
    """the packed weight fragments / adjoint tables are stale once the optimiser has stepped: every module that holds some marks or drops its own
    (nn.DeviceState.weights_changed), repacked on the next forward"""
    from .nn import DeviceState
    for m in module.modules():
        if isinstance(m, DeviceState):
            m.weights_changed()


def enable_row_programs(module):
    """after training: let the HamLayers build their fused inference chains (csrc/rowprog.hip) again -- _invalidate switches them off while the
    weights move, and the flag is sticky (validation / inference inside a training run stay on the separate kernels)"""
    from .nn import DeviceState
    for m in module.modules():
        if isinstance(m, DeviceState):
            m.enable_row_program()


@torch.no_grad()
def training_step(model, batch, metric: str = "mae", target: Optional[torch.Tensor] = None, losses=None) -> Dict[str, torch.Tensor]:
    """One loss / gradient evaluation of the WHOLE model (HamGNNConvE3 backbone + non-SOC HamGNNPlusPlusOut head): forward with the
    layer inputs kept, loss(hamiltonian, target) or the `losses` list (module docstring), backward through head and backbone on the GPU
    kernels, `.grad` of every parameter set (accumulated if already present; the overlap networks of a ham_only=False head get zeros
    unless a loss names `overlap`).  The caller owns the optimiser (`opt.step(); opt.zero_grad()`); all packed weights are dropped
    here and repacked by the next forward (a host-side repack of every block: fine for fine-tuning runs, the thing to make
    incremental for long trainings)."""
    backbone, head = model.representation, model.output_module
    if getattr(backbone, "use_kan", False):
        raise NotImplementedError("training_step of a model with HamGNN_pre.use_kan=True is not built (the KAN weight generators run forward only)")
    rep = backbone(batch, save_for_backward=True)
    out = head(batch, rep)
    tgt = target if target is not None else gget(batch, "hamiltonian")
    if tgt is None:
        raise ValueError("training_step: the batch carries no target (Hon / Hoff or hamiltonian)")
    H = out["hamiltonian"]
    g_overlap = None                                           # gradient w.r.t. result["overlap"] (losses with prediction: overlap)
    g_unshifted = None                                         # gradient w.r.t. the blocks before the zero-point shift (band energies, band gap)
    sharded = parallel.is_sharded(batch)
    if sharded:
        # model-parallel step on an edge-sharded crystal: the on-site rows are replicated, every rank holds its own off-site rows.  The row-wise
        # losses count the on-site rows once and sum the off-site rows over the ranks; the sparsity ratio is the WHOLE crystal's (the shard's own
        # count would differ per rank)
        n_on = int(batch.z.shape[0])
        row_loss = lambda p_, t_, m_: _row_loss_and_grad_sharded(p_, t_, m_, n_on)
        sr = _sharded_sparsity_ratio(head, batch) if out.get("sparsity_ratio") is not None else None
        ham_weighted = lambda l_, g_: (l_, g_) if sr is None else (l_ * sr.to(l_.dtype), g_ * sr.to(l_.dtype))
    else:
        row_loss = _loss_and_grad
        ham_weighted = lambda l_, g_: _sparsity_weighted(out, l_, g_)
    if losses is None:
        loss, gH = ham_weighted(*row_loss(H, tgt.to(H.dtype), metric))
    else:
        # the reference's `losses` list (Model.py:150-196): [{metric, prediction, target, loss_weight}] over the Hamiltonian rows, the overlap
        # rows and / or `band_energy` / `band_gap` (the second training stage: bands of H(k) against the bands of the target Hamiltonian).
        # On an edge-sharded crystal the bands and the gap in `out` are the whole crystal's on every rank (kspace.py): their losses are plain
        loss, gH = H.new_zeros(()), torch.zeros_like(H)
        g_bands = g_gap = None                                 # cotangents of the k-space losses: ONE band_energy_backward call after the loop
        for spec in losses:
            w, pred = float(spec.get("loss_weight", 1.0)), spec["prediction"].lower()
            if pred == "hamiltonian":
                t_ = gget(batch, spec["target"].lower()) if spec.get("target") else tgt
                li, gi = ham_weighted(*row_loss(H, t_.to(H.dtype), spec["metric"]))
                gH += w * gi
            elif pred in ("hamiltonian_real", "hamiltonian_imag"):
                # SOC heads: result["hamiltonian"] = [real rows; imaginary rows] (hamgnn_output.py:3621-3626 attaches the targets alike)
                if out.get(pred) is None:
                    raise ValueError(f"a {pred} loss needs a spin-orbit head")
                half = H.shape[0] // 2
                rows = slice(0, half) if pred == "hamiltonian_real" else slice(half, None)
                t_ = gget(batch, spec.get("target", pred).lower())
                li, gi = ham_weighted(*row_loss(H[rows], t_.to(H.dtype), spec["metric"]))
                gH[rows] += w * gi
            elif pred == "band_energy":
                if out.get("band_energy") is None:
                    raise ValueError("a band_energy loss needs HamGNNPlusPlusOut(calculate_band_energy=True)")
                be = out["band_energy"]
                li, gbe = _loss_and_grad(be, gget(batch, spec.get("target", "band_energy").lower()).to(be.dtype), spec["metric"])
                if head.zero_point_shift:
                    # the bands were computed from the blocks BEFORE the shift (hamgnn_output.py:3802-3880 precede :3971-3981) and then aligned
                    # by their mean (:3983-3985): adjoint of the alignment = g - mean(g)
                    gbe = gbe - gbe.mean()
                g_bands = w * gbe if g_bands is None else g_bands + w * gbe
            elif pred == "band_gap":
                # the gap of the bands around half filling (hamgnn_output.py:1930-1936): non-SOC head only, as in the reference; computed from
                # the unshifted blocks, and the mean alignment of the bands under zero_point_shift does not touch it
                if out.get("band_gap") is None:
                    raise ValueError("a band_gap loss needs a non-SOC HamGNNPlusPlusOut(calculate_band_energy=True): the spin-orbit heads emit no band_gap")
                gp = out["band_gap"]
                li, ggp = _loss_and_grad(gp, gget(batch, spec.get("target", "band_gap").lower()).to(gp.dtype), spec["metric"])
                g_gap = w * ggp if g_gap is None else g_gap + w * ggp
            elif pred == "overlap":
                # the overlap networks' prediction (ham_only=False) against the reference overlaps; no sparsity_ratio factor (Model.py:158-162
                # applies it to the three hamiltonian predictions only)
                if getattr(head, "ham_only", True) or out.get("overlap") is None:
                    raise ValueError("an overlap loss needs HamGNNPlusPlusOut(ham_only=False): ham_only=True builds no overlap networks")
                Sp = out["overlap"]
                t_ = gget(batch, spec.get("target", "overlap").lower())
                if t_ is None:
                    t_ = head._cat_by_crystal(batch, gget(batch, "Son"), gget(batch, "Soff"), head._global_inverse(batch)[1])
                li, gi = row_loss(Sp, t_.to(Sp.dtype), spec["metric"])
                g_overlap = w * gi if g_overlap is None else g_overlap + w * gi
            else:
                raise ValueError(f"training_step: losses on {pred!r} are not built (hamiltonian | hamiltonian_real | hamiltonian_imag | band_energy | band_gap | overlap)")
            loss = loss + w * li
        if g_bands is not None or g_gap is not None:
            from . import kspace
            edge_counts = head._global_inverse(batch)[1]
            Hb = head._unshifted if head.zero_point_shift else H  # (the forward kept the unshifted rows for this re-evaluation)
            if getattr(head, "soc_switch", False):
                # spin-orbit head: rows [real (N + E); imaginary (N + E)] of width (2 nao)^2, the bands of the stacked spinor H(k)
                half = Hb.shape[0] // 2
                on_r, off_r = head._split_by_crystal(batch, Hb[:half], edge_counts)
                on_i, off_i = head._split_by_crystal(batch, Hb[half:], edge_counts)
                gs = kspace.band_energy_backward_soc(head, on_r.contiguous(), on_i.contiguous(), off_r.contiguous(), off_i.contiguous(), batch, g_bands)
                g_unshifted = torch.cat([head._cat_by_crystal(batch, gs[0], gs[2], edge_counts), head._cat_by_crystal(batch, gs[1], gs[3], edge_counts)], 0)
            else:
                on, off = head._split_by_crystal(batch, Hb, edge_counts)
                g_on, g_off = kspace.band_energy_backward(head, on.contiguous(), off.contiguous(), batch, g_bands, gap_cotangent=g_gap)
                g_unshifted = head._cat_by_crystal(batch, g_on, g_off, edge_counts)
    okw = {} if g_overlap is None else {"grad_overlap": g_overlap}
    g_node, g_edge, g_head = head.backward(batch, rep, gH, grad_unshifted=g_unshifted, **okw)
    g_back = backbone.backward(batch, rep, g_node, g_edge)
    if sharded:                                                # per-edge parameters: sum the ranks' partial gradients (one flat bucket each)
        parallel.allreduce_edge_summed_gradients(g_head, batch)
        parallel.allreduce_edge_summed_gradients(g_back, batch)
    for mod, grads in ((head, g_head), (backbone, g_back)):
        params = dict(mod.named_parameters())
        missing = set(params) - set(grads)
        if missing:
            raise RuntimeError(f"training_step: no gradient for {sorted(missing)[:4]} ...")
        for k, g in grads.items():
            p = params[k]
            g = g.reshape(p.shape).to(p.dtype)
            p.grad = g.clone() if p.grad is None else p.grad + g
    if not sharded:                                            # (a sharded step uses the process group for the model-parallel sums)
        allreduce_gradients(model)                             # data-parallel runs: mean over ranks, one collective; else a no-op
    weights_changed(model)
    return {"loss": loss, "hamiltonian": H}
