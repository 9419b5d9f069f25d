"""Shared checks of the k-space step and the `losses` list on an EDGE-SHARDED crystal (parallel.shard_graph; tests/test_sharded_losses_gloo.py on the
CPU stand-ins over gloo, tests/dist_gpu_losses_check.py on the HIP kernels with two ranks sharing one GPU).  Every function is called by ALL ranks of
an initialised process group with the same arguments and returns the figures on rank 0 (None elsewhere).  References: the single-process forward /
training step of the whole crystal, and -- for the k-space losses -- torch.autograd through the fp64 oracle with the same weights, the construction of
gpu_checks.check_full_backward(bands=True) / train_targets_checks.check_full_targets (Hermitian targets, positive-definite S(k), fixed k-path, nk = 5).
Crystals of 3 to 6 atoms, nao 13, MINI irreps, radial_MLP [16, 16]."""
import math

import numpy as np
import torch
import torch.distributed as dist

from tests import gpu_checks as G
from tests import train_targets_checks as TT

NAO, SPECIES = 13, [6, 8, 1]                                   # (the 13-orbital openmx table has no Si)
KPATH, NK = TT.KPATH, TT.NK
KPATH2 = [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]                    # two nodes: a path that nk = 2 can sample
GAP_SEED_LARGE = 5  # a seed at which the fp64 reference's gap is isolated on the 2-layer model with the correlation block (gap_is_isolated: asserted by the tests)


def _cfg(num_layers, corr=False):
    return dict(num_types=20, irreps_edge_sh=G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False,
                cutoff=26.0, rbf_func="bessel", num_radial=8, num_layers=num_layers, irreps_node_features=G.MINI, use_kan=False,
                radial_MLP=[16, 16], correlation=2, num_hidden_features=4, use_corr_prod=corr, legacy_edge_update=False)


def band_graph(n_atoms=3, seed=4, soc=False):
    """the band set-up of check_full_backward(bands=True): Hermitian overlaps with S(k) positive definite and (non-SOC) Hermitian targets"""
    from hamgnn_amd.data import synthetic as S
    g = S.add_random_targets(S.random_cell(n_atoms, SPECIES, seed=seed, density=0.004), NAO, seed=seed, soc=soc)
    gen_s = torch.Generator().manual_seed(seed + 71)
    inv_ = g.inv_edge_idx
    so = 0.004 * torch.randn(g.num_edges, NAO, NAO, generator=gen_s)
    g["Soff"] = (0.5 * (so + so[inv_].transpose(1, 2))).reshape(g.num_edges, -1)
    sn = 0.004 * torch.randn(g.num_nodes, NAO, NAO, generator=gen_s)
    g["Son"] = (torch.eye(NAO) + 0.5 * (sn + sn.transpose(1, 2))).reshape(g.num_nodes, -1)
    if not soc:                                                # (SOC: eigh reads the lower triangle of the random spinor targets on both sides)
        ho = g["Hoff"].reshape(-1, NAO, NAO)
        g["Hoff"] = (0.5 * (ho + ho[inv_].transpose(1, 2))).reshape(g.num_edges, -1)
        hn = g["Hon"].reshape(-1, NAO, NAO)
        g["Hon"] = (0.5 * (hn + hn.transpose(1, 2))).reshape(g.num_nodes, -1)
    return g


def overlap_graph(n_atoms=5, seed=4, soc=False):
    """random targets with random overlap targets (the generator writes zeros; as check_full_targets('overlap'))"""
    from hamgnn_amd.data import synthetic as S
    g = S.add_random_targets(S.random_cell(n_atoms, SPECIES, seed=seed, density=0.004), NAO, seed=seed, soc=soc)
    gen_s = torch.Generator().manual_seed(seed + 71)
    g["Son"] = torch.eye(NAO).reshape(1, -1).repeat(g.num_nodes, 1) + 0.05 * torch.randn(g.num_nodes, NAO * NAO, generator=gen_s)
    g["Soff"] = 0.05 * torch.randn(g.num_edges, NAO * NAO, generator=gen_s)
    return g


def product_model(num_layers=2, seed=31, corr=False, **head_kw):
    """the same randomly initialised model on every rank"""
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    from hamgnn_amd.models.model import Model
    kw = dict(nao_max=NAO, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=False, soc_switch=False, calculate_sparsity=False,
              zero_point_shift=False)
    kw.update(head_kw)
    torch.manual_seed(seed)
    return Model(HamGNNConvE3(_cfg(num_layers, corr)), HamGNNPlusPlusOut(G.MINI, G.MINI, **kw))


def _single_process(fn):
    """run fn as a plain single-process step although a process group is up (training_step would average the gradients over the ranks)"""
    from hamgnn_amd import training as T
    keep = T.allreduce_gradients
    T.allreduce_gradients = lambda m, average=True: None
    try:
        return fn()
    finally:
        T.allreduce_gradients = keep


def _gather(obj, world):
    out = [None] * world
    dist.all_gather_object(out, obj)
    return out


def _cpu(t):
    return None if t is None else t.detach().cpu()


def _shard(g, rank, world, device):
    from hamgnn_amd import parallel
    return parallel.shard_graph(g, rank, world).to(device)


# ------------------------------------------------------------------------------------------------ 1. forward bands
def check_forward_bands(rank, world, device, soc=False, nk=NK, k_path=KPATH, n_atoms=3):
    """HamGNNPlusPlusOut(calculate_band_energy=True, zero_point_shift=True) on the shards: band_energy / band_gap / the target bands on `data` /
    k_vecs identical on all ranks, band_energy == the single-process forward of the whole crystal.  k_path=None: every rank seeds numpy's global RNG
    differently on purpose -- the k-vectors are rank 0's."""
    head_kw = dict(soc_switch=soc, soc_basis="so3", zero_point_shift=True, calculate_band_energy=True, num_k=nk, k_path=k_path)
    g = band_graph(n_atoms, seed=4, soc=soc)
    sg = _shard(g, rank, world, device)
    model = product_model(1, **head_kw).to(device)
    np.random.seed(100 + rank)
    with torch.no_grad():
        out = model(sg)
    mine = {"band_energy": _cpu(out["band_energy"]), "band_gap": _cpu(out.get("band_gap")), "wavefunction": _cpu(out["wavefunction"]),
            "target_band_energy": _cpu(sg["band_energy"]), "k_vecs": _cpu(sg["k_vecs"]), "edges": int(sg.edge_index.shape[1])}
    everyone = _gather(mine, world)
    if rank != 0:
        return None
    ref_model = product_model(1, **head_kw).to(device)
    gd = g.to(device)
    np.random.seed(100)                                        # rank 0's draw
    with torch.no_grad():
        ref = ref_model(gd)
    across = 0.0
    for other in everyone[1:]:
        for k in ("band_energy", "band_gap", "wavefunction", "target_band_energy", "k_vecs"):
            if everyone[0][k] is not None:
                assert other[k].shape == everyone[0][k].shape, k
                across = max(across, float((other[k] - everyone[0][k]).abs().max()))
    be, be_ref = everyone[0]["band_energy"].double(), ref["band_energy"].double().cpu()
    tb, tb_ref = everyone[0]["target_band_energy"].double(), gd["band_energy"].double().cpu()
    res = {"world": world, "nk": nk, "edges_per_rank": [e["edges"] for e in everyone], "bands_shape": list(be.shape), "across_ranks_max_diff": across,
           "band_energy_err": float((be - be_ref).abs().max() / be_ref.abs().max()),
           "target_band_energy_err": float((tb - tb_ref).abs().max() / tb_ref.abs().max()),
           "k_vecs_err": float((everyone[0]["k_vecs"] - gd["k_vecs"].cpu()).abs().max()),
           "wavefunction_numel_ok": everyone[0]["wavefunction"].numel() == ref["wavefunction"].numel()}
    if not soc:
        scale = float(be_ref.abs().max())
        res["band_gap_err"] = float((everyone[0]["band_gap"].double() - ref["band_gap"].double().cpu()).abs().max()) / scale
    return res


# ------------------------------------------------------------------------------------------------ 2. `losses` vs the single-process step
def _losses_case(kind):
    """-> (graph, head options, losses)"""
    L = lambda pred, metric, w=1.0, **kw: dict(metric=metric, prediction=pred, target=kw.get("target", pred), loss_weight=w)
    if kind == "overlap":                                      # list A
        return overlap_graph(5), dict(ham_only=False), [L("hamiltonian", "mae", 1.0), L("overlap", "mse", 0.5)]
    if kind == "soc_split":                                    # list B
        return (overlap_graph(4, soc=True), dict(soc_switch=True, soc_basis="so3", calculate_sparsity=True),
                [L("hamiltonian_real", "mae", 1.0), L("hamiltonian_imag", "mae", 0.5)])
    if kind in ("cosine_similarity", "euclidean_loss", "sum_zero"):                # list C
        return overlap_graph(5), {}, [L("hamiltonian", kind, 1.0)]
    raise ValueError(kind)


def _step_and_grads(model, graph, losses):
    from hamgnn_amd.training import training_step
    r = training_step(model, graph, losses=losses)
    return float(r["loss"]), {k: p.grad.detach().clone().cpu() for k, p in model.named_parameters()}


def _worst(grads, ref):
    return max(float((grads[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-6) for k in ref)


def check_losses_vs_single(rank, world, device, kind):
    """training_step(shard, losses=...) == the single-process step on the whole crystal: loss and every parameter gradient"""
    g, head_kw, losses = _losses_case(kind)
    model = product_model(2, corr=True, **head_kw).to(device)
    loss, grads = _step_and_grads(model, _shard(g, rank, world, device), losses)
    everyone = _gather((loss, grads), world)
    if rank != 0:
        return None
    loss0, grads0 = _single_process(lambda: _step_and_grads(product_model(2, corr=True, **head_kw).to(device), g.to(device), losses))
    return {"kind": kind, "loss": loss, "loss_ref": loss0, "loss_err": abs(loss - loss0) / abs(loss0), "grad_err": _worst(grads, grads0), "n": len(grads),
            "loss_across_ranks": max(abs(l - loss) for l, _ in everyone), "grad_across_ranks": max(_worst(gr, grads) for _, gr in everyone)}


def check_two_sharded_steps(rank, world, device):
    """a sharded `losses` step, opt.step(), a second sharded step: the repack after the step works on shards -- the loss moves"""
    from hamgnn_amd.training import training_step
    g, head_kw, losses = _losses_case("overlap")
    model = product_model(2, corr=True, **head_kw).to(device)
    sg = _shard(g, rank, world, device)
    opt = torch.optim.Adam(model.parameters(), lr=2e-3)
    first = float(training_step(model, sg, losses=losses)["loss"])
    opt.step()
    opt.zero_grad()
    second = float(training_step(model, sg, losses=losses)["loss"])
    finite = all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    everyone = _gather((first, second, finite), world)
    if rank != 0:
        return None
    return {"first": first, "second": second, "finite": all(e[2] for e in everyone), "same_on_all_ranks": all(e[:2] == everyone[0][:2] for e in everyone)}


# ------------------------------------------------------------------------------------------------ 3. k-space losses vs autograd through the oracle
def check_kspace_losses_vs_oracle(rank, world, device, kind, zps=False, num_layers=1, corr=False, seed=None):
    """kind: bands      [hamiltonian x 1.0, band_energy x 0.3], non-SOC, mae
             bands_gap  [hamiltonian, band_energy x 0.3, band_gap x 0.2], non-SOC, mae (the gap must be isolated on the fp64 reference: returned)
             soc_bands  [hamiltonian_real x 1.0, hamiltonian_imag x 0.5, band_energy x 0.3], SOC / so3, mse
    The sharded step's loss and every parameter gradient vs torch.autograd through the fp64 oracle on the whole crystal; on rank 0 also the
    single-process step of the product (figures for the record: `vs_single_*`)."""
    from oracle import hamgnn_ref as R
    from hamgnn_amd import kspace
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    from hamgnn_amd.models.model import Model
    soc = kind == "soc_bands"
    metric = "mse" if soc else "mae"
    seed = TT.GAP_SEED if seed is None else seed
    cfg = _cfg(num_layers, corr)
    skw = dict(soc_switch=True, soc_basis="so3") if soc else {}
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        rb = R.HamGNNConvE3(cfg)
        rh = R.HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=NAO, ham_type="openmx", symmetrize=True, add_H0=False, zero_point_shift=zps, **skw)
    finally:
        torch.set_default_dtype(prev)
    g = band_graph(3, seed=seed, soc=soc)
    g["k_vecs"] = kspace.make_k_vectors(KPATH, NK, g.cell)
    L = lambda pred, w: dict(metric=metric, prediction=pred, target=pred, loss_weight=w)
    if soc:
        losses = [L("hamiltonian_real", 1.0), L("hamiltonian_imag", 0.5), L("band_energy", 0.3)]
    else:
        losses = [L("hamiltonian", 1.0), L("band_energy", 0.3)] + ([L("band_gap", 0.2)] if kind == "bands_gap" else [])

    def build():
        return Model(G.load_weights(HamGNNConvE3(cfg), dict(rb.state_dict())),
                     G.load_weights(HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=NAO, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=False,
                                                      calculate_sparsity=False, zero_point_shift=zps, calculate_band_energy=True, num_k=NK, k_path=KPATH,
                                                      **(skw if soc else dict(soc_switch=False))), dict(rh.state_dict()))).to(device)
    solves = []
    real_solve, real_soc_solve = kspace._eig_solve, kspace._soc_solve

    def spy(Hk, *a, **kw):
        if Hk.requires_grad:
            solves.append(int(Hk.shape[0]))
        return (real_soc_solve if soc else real_solve)(Hk, *a, **kw)
    setattr(kspace, "_soc_solve" if soc else "_eig_solve", spy)
    try:
        loss, grads = _step_and_grads(build(), _shard(g, rank, world, device), losses)
    finally:
        kspace._eig_solve, kspace._soc_solve = real_solve, real_soc_solve
    everyone = _gather((loss, sum(solves)), world)
    if rank != 0:
        return None
    lf = {"mae": lambda d: d.abs().mean(), "mse": lambda d: (d * d).mean()}[metric]
    g64 = type(g)({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in g.items()})
    N_ = g.num_nodes
    Href = rh(g64, rb(g64))["hamiltonian"]
    rh.zero_point_shift = False
    Hu = rh(g64, rb(g64))["hamiltonian"]                       # the bands and the gap come from the blocks BEFORE the zero-point shift
    rh.zero_point_shift = zps
    res = {"kind": kind, "zps": zps}
    if soc:
        h_ = Hu.shape[0] // 2
        be = rh.calculate_band_energies_with_spin_orbit_coupling(Hu[:N_], Hu[h_:h_ + N_], Hu[N_:h_], Hu[h_ + N_:], g64)[0]
        with torch.no_grad():
            tb = rh.calculate_band_energies_with_spin_orbit_coupling(g64["Hon"], g64["iHon"], g64["Hoff"], g64["iHoff"], g64)[0]
        if zps:
            be = be - torch.mean(be - tb)
        tr, ti = torch.cat([g64["Hon"], g64["Hoff"]], 0), torch.cat([g64["iHon"], g64["iHoff"]], 0)
        half = Href.shape[0] // 2
        loss_ref = lf(Href[:half] - tr) + 0.5 * lf(Href[half:] - ti) + 0.3 * lf(be - tb)
    else:
        be, _, gap, _ = rh.calculate_band_energies(Hu[:N_], Hu[N_:], g64)
        with torch.no_grad():
            tb, _, tgap, _ = rh.calculate_band_energies(g64["Hon"], g64["Hoff"], g64)
        nhalf = math.ceil(sum(float(rh.num_valence[int(zz)]) for zz in g.z.tolist()) / 2)
        res["gap_isolated"], res["gap_separations"] = TT.gap_is_isolated(be.detach().transpose(0, 1), nhalf)
        if zps:
            be = be - torch.mean(be - tb)
        loss_ref = lf(Href - torch.cat([g64["Hon"], g64["Hoff"]], 0)) + 0.3 * lf(be - tb) + (0.2 * lf(gap - tgap) if kind == "bands_gap" else 0.0)
    loss_ref.backward()
    want = {}
    for prefix, ref in (("representation.", rb), ("output_module.", rh)):
        for k, p in ref.named_parameters():
            want[prefix + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach()
    assert set(want) == set(grads), sorted(set(want) ^ set(grads))[:4]
    worst = {k: float((grads[k].double().reshape(want[k].shape) - want[k]).abs().max()) / max(float(want[k].abs().max()), 1e-6) for k in want}
    k = max(worst, key=worst.get)
    lr = float(loss_ref.detach())
    res.update(loss=loss, loss_ref=lr, loss_rel_err=abs(loss - lr) / abs(lr), max_rel_err=worst[k], worst=k, n=len(worst),
               loss_across_ranks=max(abs(e[0] - loss) for e in everyone), k_points_solved_in_backward=[e[1] for e in everyone])
    loss1, grads1 = _single_process(lambda: _step_and_grads(build(), g.to(device), losses))
    res.update(vs_single_loss_err=abs(loss - loss1) / abs(loss1), vs_single_grad_err=_worst(grads, grads1))
    return res


# ------------------------------------------------------------------------------------------------ 4. refusals, and the unsharded path
def check_refusals(rank, world, device):
    """export_reciprocal_values on a sharded graph: NotImplementedError; `wavefunction` / `peak` losses: ValueError('... not built ...') as on one rank"""
    from hamgnn_amd.training import training_step
    g = band_graph(3, seed=4)
    sg = _shard(g, rank, world, device)
    got = {}
    model = product_model(1, calculate_band_energy=True, num_k=NK, k_path=KPATH, export_reciprocal_values=True).to(device)
    sg["dSon"], sg["dSoff"] = torch.zeros(sg.z.shape[0], NAO * NAO, 3, device=device), torch.zeros(sg.edge_index.shape[1], NAO * NAO, 3, device=device)
    try:
        with torch.no_grad():
            model(sg)
        got["export"] = "no error"
    except NotImplementedError as e:
        got["export"] = "NotImplementedError: " + str(e)
    for pred in ("wavefunction", "peak"):
        model = product_model(1).to(device)
        try:
            training_step(model, _shard(g, rank, world, device), losses=[dict(metric="mae", prediction=pred, target=pred)])
            got[pred] = "no error"
        except ValueError as e:
            got[pred] = "ValueError: " + str(e)
    everyone = _gather(got, world)
    return everyone if rank == 0 else None


def check_unsharded_takes_the_old_path(device):
    """band_energies on an UNSHARDED graph under an initialised process group issues no collective (all_reduce / all_gather / broadcast fail here)"""
    from hamgnn_amd import kspace

    def boom(*a, **kw):
        raise AssertionError("a collective on an unsharded graph")
    keep = dist.all_reduce, dist.all_gather, dist.broadcast
    dist.all_reduce = dist.all_gather = dist.broadcast = boom
    try:
        g = band_graph(3, seed=4).to(device)
        model = product_model(1, calculate_band_energy=True, num_k=NK, k_path=KPATH).to(device)
        with torch.no_grad():
            out = model(g)
            head = model.output_module
            N = g.num_nodes
            be, _, gap, _ = kspace.band_energies(head, out["hamiltonian"][:N].contiguous(), out["hamiltonian"][N:].contiguous(), g)
        return {"bands_shape": list(be.shape), "same_as_forward": float((be - out["band_energy"]).abs().max())}
    finally:
        dist.all_reduce, dist.all_gather, dist.broadcast = keep
