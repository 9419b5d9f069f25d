"""Shared checks of the training targets beyond the Hamiltonian (tests/test_train_targets_gpu.py on the GPU, tests/test_train_targets_cpu.py on the
CPU stand-ins): the adjoint of the H(k) assembly (csrc/kspace.hip: hg_hk_assemble_adjoint) alone, `overlap` losses through a ham_only=False head,
`band_gap` losses through the k-space chain, and the row-wise metrics.  All references are fp64: oracle.hamgnn_ref under torch.autograd, and the torch
path of kspace.assemble_k_adjoint evaluated in fp64 on the CPU."""
import math
import os

import numpy as np
import torch

from tests import gpu_checks as G

KPATH, NK = [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.5, 0.5, 0.0]], 5
SU2_IRR = "8x0e+8x0o+4x1e+4x1o+4x2e+4x2o+2x3e+2x3o+2x4e+2x4o+2x5e+2x5o"      # features up to l = 5: every su2 coupling of a 13-orbital basis is fed


# ------------------------------------------------------------------------------------------------ the adjoint kernel alone
def orank_table(ham_type, nao):
    """[119, nao] rank of an orbital inside its element's valid set or -1 (what HamGNNPlusPlusOut.compile builds for the k-space step)"""
    from hamgnn_amd import basis as B
    tab = np.full((119, nao), -1, dtype=np.int32)
    for Z, orb in B.basis_table(ham_type, nao)["basis_def"].items():
        tab[Z, sorted(orb)] = np.arange(len(orb), dtype=np.int32)
    return torch.from_numpy(tab)


def adjoint_case(name, nk=5, seed=0):
    """-> (graph, n0, n, e0, e, k_vecs_c [nk, 3] float32, nao, orank_all [N, nao]); all on the CPU.
    one_atom: a 1-atom cell, every edge a self image -- the (i, i) pairs read the diagonal block g_on reads
    coh:      3 atoms C / O / H (one each), nao 13: H lacks orbitals (orank = -1 rows and columns); several images per atom pair
    batch2:   the SECOND crystal of a two-crystal batch (n0, e0 > 0)
    far:      coh with nbr_shift scaled so that max |k . shift| exceeds 20 turns (the double-precision phase)
    no_edges: the atoms of coh with an empty edge slice (npairs = 0: g_on is still written)"""
    from hamgnn_amd.data import synthetic as S, collate
    nao = 13
    if name == "one_atom":
        g = S.random_cell(1, [6], seed=3, density=0.004)
    elif name == "batch2":
        g = collate([S.random_cell(2, [6, 8, 1], seed=7, density=0.004), S.random_cell(3, [6, 8, 1], seed=0, density=0.012)])
    else:
        g = S.random_cell(3, [6, 8, 1], seed=0, density=0.012)
    from hamgnn_amd import kspace
    sl = kspace._crystal_slices(g)
    n0, n, e0, e = sl[-1]
    if name == "no_edges":
        e = 0
    gen = torch.Generator().manual_seed(seed)
    kv = (0.12 * torch.randn(nk, 3, generator=gen)).float()
    if name == "far":
        turns = (kv.double()[:, None, :] * g.nbr_shift.double()[None, e0:e0 + e, :]).sum(-1).abs().max()
        g["nbr_shift"] = (g.nbr_shift.double() * (25.0 / float(turns))).float()
    orank_all = orank_table("openmx", nao)[g.z].long()
    return g, n0, n, e0, e, kv, nao, orank_all


def hk_adjoint_numpy(G_, shift, kvec, pair_ptr, pair_edges, pair_ij, n_atoms, n_edges, nao, orank, ooff, absolute=False):
    """numpy twin of hg_hk_assemble_adjoint on the kernel's own tables and loop structure (pair -> edge of the pair -> element -> ascending k), fp64.
    absolute: the sum of the absolute values of the terms instead (the rounding scale of the bilinear form)"""
    G_ = np.asarray(G_)
    shift, kvec = np.asarray(shift, dtype=np.float64), np.asarray(kvec, dtype=np.float64)
    pair_ptr, pair_edges, pair_ij = (np.asarray(t) for t in (pair_ptr, pair_edges, pair_ij))
    orank, ooff = np.asarray(orank), np.asarray(ooff)
    nk = G_.shape[0]
    f = np.abs if absolute else (lambda x: x)
    g_on, g_off = np.zeros((n_atoms, nao, nao)), np.zeros((n_edges, nao, nao))
    for i in range(n_atoms):
        for a in range(nao):
            for b in range(nao):
                ra, rb = orank[i, a], orank[i, b]
                if ra >= 0 and rb >= 0:
                    g_on[i, a, b] = sum(f(G_[k, ooff[i] + ra, ooff[i] + rb].real) for k in range(nk))
    for p in range(pair_ij.shape[0]):
        i, j = int(pair_ij[p, 0]), int(pair_ij[p, 1])
        va, vb = np.nonzero(orank[i] >= 0)[0], np.nonzero(orank[j] >= 0)[0]
        rows, cols = ooff[i] + orank[i][va], ooff[j] + orank[j][vb]
        for t in range(int(pair_ptr[p]), int(pair_ptr[p + 1])):
            e = int(pair_edges[t])
            acc = np.zeros((len(va), len(vb)))
            for k in range(nk):
                ph = 2.0 * math.pi * float(kvec[k] @ shift[e])
                blk = G_[k][np.ix_(rows, cols)]
                acc += f(math.cos(ph) * blk.real) + f(math.sin(ph) * blk.imag)
            g_off[e][np.ix_(va, vb)] = acc
    return g_on.reshape(n_atoms, nao * nao), g_off.reshape(n_edges, nao * nao)


def _tab(case, device="cpu"):
    """the kspace.CrystalTables of the case's crystal"""
    from hamgnn_amd import kspace
    g, n0, n, e0, e, kv, nao, orank_all = case
    return kspace.CrystalTables.from_graph(g.to(device), n0, n, e0, e, orank_all.to(device))


def _tables(case):
    t = _tab(case)
    return t.pair_ptr, t.pair_edges, t.pair_ij, t.orank, t.ooff, t.M


def random_G(nk, M, seed=1, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(nk, M, M, generator=gen, dtype=dtype), torch.randn(nk, M, M, generator=gen, dtype=dtype))


def reference_adjoint(case, G64):
    """the torch path of the adjoint in fp64 on the CPU"""
    from hamgnn_amd import kspace
    return kspace._assemble_k_adjoint_torch(G64, _tab(case), case[5].double())      # (case[5]: its k-vectors)


def absent_mask(case):
    """bool [n, nao^2], [e, nao^2]: elements whose orbital a or b the atom lacks"""
    g, n0, n, e0, e, kv, nao, orank_all = case
    ok = orank_all[n0:n0 + n] >= 0
    src, dst = g.edge_index[0][e0:e0 + e] - n0, g.edge_index[1][e0:e0 + e] - n0
    on = ~(ok[:, :, None] & ok[:, None, :]).reshape(n, nao * nao)
    off = ~(ok[src][:, :, None] & ok[dst][:, None, :]).reshape(e, nao * nao)
    return on, off


def _rel0(a, b):
    """gpu_checks.rel, with an empty or all-zero reference compared absolutely"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def check_adjoint_kernel(device, name, nk):
    """ops.hk_assemble_adjoint vs the fp64 torch adjoint; the entries of absent orbitals are exactly 0; a second launch is bit-identical; with
    HG_HK_ADJOINT=torch the device's torch path agrees with the kernel"""
    from hamgnn_amd import kspace, ops
    case = adjoint_case(name, nk)
    g, n0, n, e0, e, kv, nao, orank_all = case
    ptr, order, pij, orank, ooff, M = _tables(case)
    G64 = random_G(nk, M)
    r_on, r_off = reference_adjoint(case, G64)
    Gd, kvd = G64.to(torch.complex64).to(device), kv.to(device)

    def run():
        t = _tab(case, device)
        return ops.hk_assemble_adjoint(Gd, t.shift, kvd, t.pair_ptr, t.pair_edges, t.pair_ij, n, e, nao, t.orank, t.ooff, t.M)
    a_on, a_off = run()
    b_on, b_off = run()
    via_on, via_off = kspace.assemble_k_adjoint(Gd, _tab(case, device), kvd)      # the public entry: the kernel on a GPU tensor
    prev = os.environ.get("HG_HK_ADJOINT")
    os.environ["HG_HK_ADJOINT"] = "torch"
    try:
        t_on, t_off = kspace.assemble_k_adjoint(Gd, _tab(case, device), kvd)
    finally:
        os.environ.pop("HG_HK_ADJOINT") if prev is None else os.environ.__setitem__("HG_HK_ADJOINT", prev)
    m_on, m_off = absent_mask(case)
    turns = float((kv.double()[:, None, :] * g.nbr_shift.double()[None, e0:e0 + e, :]).sum(-1).abs().max()) if e else 0.0
    counts = (ptr[1:] - ptr[:-1])
    return {"n0": n0, "e0": e0, "n": n, "e": e, "npairs": int(pij.shape[0]), "max_edges_per_pair": int(counts.max()) if counts.numel() else 0,
            "self_pairs": int((pij[:, 0] == pij[:, 1]).sum()) if pij.numel() else 0, "absent_on": int(m_on.sum()), "absent_off": int(m_off.sum()),
            "max_turns": turns,
            "g_on_rel_err": _rel0(a_on, r_on), "g_off_rel_err": _rel0(a_off, r_off),
            "absent_on_max": float(a_on.cpu()[m_on].abs().max()) if m_on.any() else 0.0,
            "absent_off_max": float(a_off.cpu()[m_off].abs().max()) if m_off.any() else 0.0,
            "relaunch_max_diff": max(float((a_on - b_on).abs().max()), float((a_off - b_off).abs().max()) if e else 0.0),
            "entry_max_diff": max(float((a_on - via_on).abs().max()), float((a_off - via_off).abs().max()) if e else 0.0),
            "torch_path_on_rel": _rel0(t_on, a_on), "torch_path_off_rel": _rel0(t_off, a_off)}


def check_adjoint_identity(device, name="coh", nk=5):
    """<hk_assemble(x), G> = <x, hk_assemble_adjoint(G)>, HIP against HIP, the dot products in fp64 on the host.  Bound: two fp32 evaluations of one
    bilinear form differ by at most 4 * 2^-24 * sum |terms| (the terms: x * phase component * G component)"""
    from hamgnn_amd import ops
    case = adjoint_case(name, nk)
    g, n0, n, e0, e, kv, nao, orank_all = case
    ptr, order, pij, orank, ooff, M = _tables(case)
    gen = torch.Generator().manual_seed(5)
    on, off = torch.randn(n, nao * nao, generator=gen), torch.randn(e, nao * nao, generator=gen)
    G32 = random_G(nk, M, dtype=torch.float32)
    dv = lambda t: t.to(device)
    shift = g.nbr_shift[e0:e0 + e].contiguous().float()
    Hk = ops.hk_assemble(dv(on), dv(off), dv(shift), dv(kv), dv(ptr), dv(order), dv(pij), n, nao, dv(orank), dv(ooff), M)
    a_on, a_off = ops.hk_assemble_adjoint(dv(G32), dv(shift), dv(kv), dv(ptr), dv(order), dv(pij), n, e, nao, dv(orank), dv(ooff), M)
    Hk, a_on, a_off = Hk.cpu().to(torch.complex128), a_on.double().cpu(), a_off.double().cpu()
    G64 = G32.to(torch.complex128)
    lhs = float((Hk.real * G64.real + Hk.imag * G64.imag).sum())
    rhs = float((on.double() * a_on).sum() + (off.double() * a_off).sum())
    s_on, s_off = hk_adjoint_numpy(G64.numpy(), shift.numpy(), kv.numpy(), ptr, order, pij, n, e, nao, orank, ooff, absolute=True)
    scale = float((on.double().abs() * torch.from_numpy(s_on)).sum() + (off.double().abs() * torch.from_numpy(s_off)).sum())
    return {"lhs": lhs, "rhs": rhs, "diff": abs(lhs - rhs), "bound": 4.0 * 2.0 ** -24 * scale}


def check_adjoint_twin(name, nk, flip=False):
    """the numpy twin vs kspace.assemble_k_adjoint (its torch path: CPU tensors) in fp64; flip: one orank entry of the twin's table is turned from
    'has the orbital' to 'lacks it' -- the comparison must then fail"""
    from hamgnn_amd import kspace
    case = adjoint_case(name, nk)
    g, n0, n, e0, e, kv, nao, orank_all = case
    ptr, order, pij, orank, ooff, M = _tables(case)
    G64 = random_G(nk, M)
    r_on, r_off = kspace.assemble_k_adjoint(G64, _tab(case), kv.double())
    orank = orank.clone()
    if flip:
        orank[0, int(torch.nonzero(orank[0] >= 0)[-1])] = -1
    t_on, t_off = hk_adjoint_numpy(G64.numpy(), g.nbr_shift[e0:e0 + e].double().numpy(), kv.double().numpy(), ptr, order, pij, n, e, nao, orank, ooff)
    return {"g_on_rel_err": _rel0(torch.from_numpy(t_on), r_on), "g_off_rel_err": _rel0(torch.from_numpy(t_off), r_off)}


# ------------------------------------------------------------------------------------------------ overlap: the head alone
def check_head_backward_overlap(device="cuda", basis=None, n_atoms=6, seed=1):
    """gpu_checks.check_head_backward / check_soc_head_backward with ham_only=False: gradient of (H * G_H).sum() + (S * G_S).sum() with respect to the
    representation and every head parameter -- the overlap networks' four groups included -- vs torch.autograd through the fp64 oracle.
    basis: None (non-SOC, openmx 19) | 'so3' (openmx 19) | 'su2' (abacus 13)"""
    from oracle import hamgnn_ref as R
    from hamgnn_amd import ops, plan as P
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    soc = basis is not None
    irr, ham_type, nao, zs = (SU2_IRR, "abacus", 13, [14, 8, 6]) if basis == "su2" else (G.MINI, "openmx", 19, [14, 8, 6, 1])
    kw = dict(soc_switch=True, soc_basis=basis) if soc else dict(soc_switch=False)
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = R.HamGNNPlusPlusOut(irr, irr, nao_max=nao, ham_type=ham_type, symmetrize=True, add_H0=True, ham_only=False, **kw)
    finally:
        torch.set_default_dtype(prev)
    g = S.add_random_targets(S.random_cell(n_atoms, zs, seed=seed, density=0.004), nao, seed=seed, soc=soc)
    N, E = g.num_nodes, g.num_edges
    gen = torch.Generator().manual_seed(seed)
    D = R.Irreps(irr).dim
    node = torch.randn(N, D, generator=gen, dtype=torch.float64).requires_grad_()
    edge = torch.randn(E, D, generator=gen, dtype=torch.float64).requires_grad_()
    G_H = torch.randn((2 if soc else 1) * (N + E), (4 if soc else 1) * nao * nao, generator=gen, dtype=torch.float64)
    G_S = torch.randn(N + E, nao * nao, generator=gen, dtype=torch.float64)
    g64 = type(g)({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in g.items()})
    o = ref(g64, {"node_attr": node, "edge_attr": edge})
    ((o["hamiltonian"] * G_H).sum() + (o["overlap"] * G_S).sum()).backward()
    hip = G.load_weights(HamGNNPlusPlusOut(irr, irr, nao_max=nao, ham_type=ham_type, ham_only=False, symmetrize=True, add_H0=True,
                                           calculate_sparsity=False, zero_point_shift=False, **kw), dict(ref.state_dict()))
    hip.compile(device)
    gd = g.to(device)
    lay = P.PlanarLayout(irr)
    imap = torch.from_numpy(lay.index_map().astype(np.int32)).to(device)
    geo = ops.Geometry(gd.pos, gd.edge_index, gd.nbr_shift, 1.0, 1, hip._lmax, hip._jtab)
    node_pl = ops.to_planar(node.detach().float().to(device), imap, lay.dim)
    edge_rot = ops.rotate_gather(ops.to_planar(edge.detach().float().to(device), imap, lay.dim), None, geo, hip._rot_tab)
    rep = {"_node_planar": node_pl, "_edge_planar_rot": edge_rot, "_geometry": geo}
    out = hip(gd, rep)
    g_node, g_edge, gw = hip.backward(gd, rep, G_H.float().to(device), grad_overlap=G_S.float().to(device))
    g_edge = ops.rotate_gather(g_edge, None, geo, hip._rot_tab, transpose=True)
    torch.cuda.synchronize()
    res = {"forward_rel_err": G.rel(out["hamiltonian"], o["hamiltonian"].detach()), "overlap_forward_rel_err": G.rel(out["overlap"], o["overlap"].detach()),
           "g_node_rel_err": G.rel(ops.from_planar(g_node, imap), node.grad), "g_edge_rel_err": G.rel(ops.from_planar(g_edge, imap), edge.grad)}
    refp = dict(ref.named_parameters())
    assert set(gw) == set(refp), sorted(set(gw) ^ set(refp))[:4]
    zero = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)
    errs = {k: float((gw[k].double().cpu().reshape(refp[k].shape) - zero(refp[k])).abs().max()) / max(float(zero(refp[k]).abs().max()), 1e-6) for k in gw}
    res["g_weights_max_rel_err"] = max(errs.values())
    res["overlap_groups_trained"] = sum(1 for k in refp if "overlap_network" in k and refp[k].grad is not None and float(refp[k].grad.abs().max()) > 0)
    return res


# ------------------------------------------------------------------------------------------------ whole model
def gap_is_isolated(evals, half):
    """the condition on the inputs of a band_gap check, on the fp64 reference alone: the gap is a min / max over k, not differentiable at ties.  evals
    [nk, bands]: the smallest and second-smallest value of band `half`, the largest and second-largest of band `half - 1`, each pair further apart
    than 1e-3 x the spectrum's scale (ten times the 1e-4 eigenvalue bar of the fp32 solver).  -> (ok, the two separations / scale)"""
    scale = float(evals.abs().max())
    lo = torch.sort(evals[:, half]).values
    hi = torch.sort(evals[:, half - 1], descending=True).values
    d_lo, d_hi = float(lo[1] - lo[0]) / scale, float(hi[0] - hi[1]) / scale
    return (d_lo > 1e-3 and d_hi > 1e-3), (d_lo, d_hi)


def check_full_targets(device="cuda", kind="overlap", zps=False, seed=None, metric="mae"):
    """gpu_checks.check_full_backward for the new targets: the whole model (HamGNNConvE3 + non-SOC head), training_step(model, g, losses=...) vs
    torch.autograd through the fp64 oracle with the same weights.
    kind: overlap      ham_only=False, 6 atoms, 2 layers, nao 19: [hamiltonian x 1.0, overlap x 0.5], random Son / Soff targets
          plain        the same ham_only=False model, plain metric='mse' (no `losses`): the overlap parameters' .grad is exactly zero; also
                       returns the largest deviation from the same step on the ham_only=True model
          gap_bands    3 atoms, 1 layer, nao 13, k-path: [hamiltonian, band_energy x 0.3, band_gap x 0.2]
          gap          ... [hamiltonian, band_gap]; counts the _eig_chain evaluations of the backward
          euclid       6 atoms, 2 layers, nao 19, ham_only=True: [hamiltonian with metric euclidean_loss]"""
    from oracle import hamgnn_ref as R
    from hamgnn_amd import kspace
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    from hamgnn_amd.models.model import Model
    from hamgnn_amd.training import training_step
    bands = kind in ("gap", "gap_bands")
    n_atoms, num_layers, nao = (3, 1, 13) if bands else (6, 2, 19)
    seed = (GAP_SEED if bands else 4) if seed is None else seed
    ham_only = kind not in ("overlap", "plain")
    cfg = dict(num_types=20, irreps_edge_sh=G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False,
               cutoff=26.0, rbf_func="bessel", num_radial=8, num_layers=num_layers, irreps_node_features=G.MINI, use_kan=False,
               radial_MLP=[16, 16], correlation=2, num_hidden_features=4, use_corr_prod=False, legacy_edge_update=False)
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        rb = R.HamGNNConvE3(cfg)
        rh = R.HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=nao, ham_type="openmx", symmetrize=True, add_H0=False, zero_point_shift=zps, ham_only=ham_only)
    finally:
        torch.set_default_dtype(prev)
    species = [6, 8, 1] if nao == 13 else [14, 8, 6, 1]
    g = S.add_random_targets(S.random_cell(n_atoms, species, seed=seed, density=0.004), nao, seed=seed)
    gen_s = torch.Generator().manual_seed(seed + 71)
    inv_ = g.inv_edge_idx
    if bands:                                                  # Hermitian overlaps with S(k) positive definite, Hermitian targets, a fixed k-path (as check_full_backward)
        so = 0.004 * torch.randn(g.num_edges, nao, nao, generator=gen_s)
        g["Soff"] = (0.5 * (so + so[inv_].transpose(1, 2))).reshape(g.num_edges, -1)
        sn = 0.004 * torch.randn(g.num_nodes, nao, nao, generator=gen_s)
        g["Son"] = (torch.eye(nao) + 0.5 * (sn + sn.transpose(1, 2))).reshape(g.num_nodes, -1)
        ho = g["Hoff"].reshape(-1, nao, nao)
        g["Hoff"] = (0.5 * (ho + ho[inv_].transpose(1, 2))).reshape(g.num_edges, -1)
        hn = g["Hon"].reshape(-1, nao, nao)
        g["Hon"] = (0.5 * (hn + hn.transpose(1, 2))).reshape(g.num_nodes, -1)
        g["k_vecs"] = kspace.make_k_vectors(KPATH, NK, g.cell)
    else:                                                      # random overlap targets (the generator writes zeros: mae against exact zeros is not informative)
        g["Son"] = torch.eye(nao).reshape(1, -1).repeat(g.num_nodes, 1) + 0.05 * torch.randn(g.num_nodes, nao * nao, generator=gen_s)
        g["Soff"] = 0.05 * torch.randn(g.num_edges, nao * nao, generator=gen_s)
    g64 = type(g)({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in g.items()})
    N_ = g.num_nodes
    o = rh(g64, rb(g64))
    Href = o["hamiltonian"]
    target = torch.cat([g64["Hon"], g64["Hoff"]], 0)
    lf = {"mae": lambda d: d.abs().mean(), "mse": lambda d: (d * d).mean()}[metric]
    res, step_kw = {}, {}
    if kind == "overlap":
        loss_ref = lf(Href - target) + 0.5 * lf(o["overlap"] - torch.cat([g64["Son"], g64["Soff"]], 0))
        step_kw["losses"] = [dict(metric=metric, prediction="hamiltonian", target="hamiltonian", loss_weight=1.0),
                             dict(metric=metric, prediction="overlap", target="overlap", loss_weight=0.5)]
    elif kind == "plain":
        target = 0.1 * torch.randn(Href.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        loss_ref = ((Href - target) ** 2).mean()
        step_kw.update(metric="mse", target=target.float().to(device))
    elif kind == "euclid":
        loss_ref = torch.linalg.vector_norm(Href - target, dim=1).mean()
        step_kw["losses"] = [dict(metric="euclidean_loss", prediction="hamiltonian", target="hamiltonian", loss_weight=1.0)]
    else:
        rh.zero_point_shift = False
        Hu = rh(g64, rb(g64))["hamiltonian"]                   # the bands and the gap come from the blocks BEFORE the zero-point shift
        rh.zero_point_shift = zps
        be, _, gap, _ = rh.calculate_band_energies(Hu[:N_], Hu[N_:], g64)
        with torch.no_grad():
            tb, _, tgap, _ = rh.calculate_band_energies(g64["Hon"], g64["Hoff"], g64)
        half = math.ceil(sum(float(rh.num_valence[int(zz)]) for zz in g.z.tolist()) / 2)
        res["gap_isolated"], res["gap_separations"] = gap_is_isolated(be.detach().transpose(0, 1), half)
        res["gap_ref"], res["gap_target"] = float(gap.detach()), float(tgap)
        if zps:
            be = be - torch.mean(be - tb)
        loss_ref = lf(Href - target) + (0.3 * lf(be - tb) + 0.2 * lf(gap - tgap) if kind == "gap_bands" else lf(gap - tgap))
        step_kw["losses"] = [dict(metric=metric, prediction="hamiltonian", target="hamiltonian", loss_weight=1.0)]
        if kind == "gap_bands":
            step_kw["losses"] += [dict(metric=metric, prediction="band_energy", target="band_energy", loss_weight=0.3),
                                  dict(metric=metric, prediction="band_gap", target="band_gap", loss_weight=0.2)]
        else:
            step_kw["losses"] += [dict(metric=metric, prediction="band_gap", target="band_gap")]

    def build(ham_only_):
        sd = {k: v for k, v in rh.state_dict().items() if not (ham_only_ and "overlap_network" in k)}
        return Model(G.load_weights(HamGNNConvE3(cfg), dict(rb.state_dict())),
                     G.load_weights(HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=nao, ham_type="openmx", ham_only=ham_only_, symmetrize=True, add_H0=False,
                                                      calculate_sparsity=False, zero_point_shift=zps, soc_switch=False,
                                                      **(dict(calculate_band_energy=True, num_k=NK, k_path=KPATH) if bands else {})), sd)).to(device)
    model = build(ham_only)
    gd = g.to(device)
    chains = []
    real_chain = kspace._eig_chain

    def spy_chain(head, Hk, *a):
        chains.append(bool(Hk.requires_grad))
        return real_chain(head, Hk, *a)
    kspace._eig_chain = spy_chain
    try:
        r = training_step(model, gd, **step_kw)
    finally:
        kspace._eig_chain = real_chain
    if device != "cpu":
        torch.cuda.synchronize()
    res["eig_chains_in_backward"] = sum(chains)
    loss_ref.backward()
    res.update(N=g.num_nodes, E=g.num_edges, loss_rel_err=abs(float(r["loss"]) - float(loss_ref.detach())) / abs(float(loss_ref.detach())))
    worst = {}
    for mod, ref in ((model.representation, rb), (model.output_module, rh)):
        refp = dict(ref.named_parameters())
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            want = refp[k].grad if refp[k].grad is not None else torch.zeros_like(refp[k])
            worst[k] = float((p.grad.double().cpu().reshape(want.shape) - want).abs().max()) / max(float(want.abs().max()), 1e-6)
    k = max(worst, key=worst.get)
    res.update(n_params=len(worst), max_rel_err=worst[k], worst=k)
    ov = {k_: p for k_, p in model.output_module.named_parameters() if "overlap_network" in k_}
    res["overlap_params"] = len(ov)
    res["overlap_grad_max"] = max((float(p.grad.abs().max()) for p in ov.values()), default=0.0)
    res["overlap_groups_trained"] = sum(1 for k_ in ov if dict(rh.named_parameters())[k_].grad is not None)
    if kind == "plain":                                        # all other gradients: as the ham_only=True model's (the same kernels on the same inputs)
        other = build(True)
        training_step(other, g.to(device), **step_kw)
        po = dict(other.named_parameters())
        res["vs_ham_only_max_rel"] = max(float((p.grad - po[k_].grad).abs().max()) / max(float(po[k_].grad.abs().max()), 1e-30)
                                         for k_, p in model.named_parameters() if "overlap_network" not in k_)
    return res


GAP_SEED = 4        # a seed at which the fp64 reference's gap is isolated for zps in {False, True} (gap_is_isolated: asserted by the tests)


def check_head_training_step_overlap(device="cuda"):
    """head_training_step on a ham_only=False head: runs, and sets the gradient of every head parameter (zeros on the overlap networks)"""
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    from hamgnn_amd.models.model import Model
    from hamgnn_amd.training import head_training_step
    model = _small_model(ham_only=False).to(device)
    g = S.add_random_targets(S.random_cell(3, [6, 8, 1], seed=3, density=0.004), 13, seed=3).to(device)
    r = head_training_step(model, g, metric="mae")
    head = model.output_module
    return {"loss": float(r["loss"]), "all_set": all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in head.parameters()),
            "overlap_grad_max": max(float(p.grad.abs().max()) for k, p in head.named_parameters() if "overlap_network" in k),
            "ham_grad_max": max(float(p.grad.abs().max()) for k, p in head.named_parameters() if "hamiltonian_network" in k)}


def _small_model(ham_only=True, soc=False, bands=False, seed=31):
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    from hamgnn_amd.models.model import Model
    cfg = dict(num_types=20, irreps_edge_sh=G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False,
               cutoff=26.0, rbf_func="bessel", num_radial=8, num_layers=1, irreps_node_features=G.MINI, use_kan=False, radial_MLP=[16, 16],
               correlation=2, num_hidden_features=4, use_corr_prod=False)
    torch.manual_seed(seed)
    return Model(HamGNNConvE3(cfg), HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=13, ham_type="openmx", ham_only=ham_only, symmetrize=True, add_H0=True,
                                                      soc_switch=soc, soc_basis="so3", calculate_sparsity=False, zero_point_shift=False,
                                                      calculate_band_energy=bands, num_k=4, k_path=None))


def refusal(device, what):
    """the training_step call that must raise ValueError: 'overlap_ham_only' | 'gap_no_bands' | 'gap_soc'"""
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.training import training_step
    soc = what == "gap_soc"
    model = _small_model(ham_only=True, soc=soc, bands=soc).to(device)
    g = S.add_random_targets(S.random_cell(2, [6, 8, 1], seed=3, density=0.004), 13, seed=3, soc=soc)
    g["Son"] = torch.eye(13).reshape(1, -1).repeat(g.num_nodes, 1)
    pred = "overlap" if what == "overlap_ham_only" else "band_gap"
    np.random.seed(0)
    training_step(model, g.to(device), losses=[dict(metric="mae", prediction="hamiltonian", target="hamiltonian"), dict(metric="mae", prediction=pred)])


def check_band_gap_backward(device="cuda"):
    """kspace.band_energy_backward(cotangent=None, gap_cotangent=...) on the fixture graph band_energies_openmx_13 vs autograd through
    oracle.hamgnn_ref.calculate_band_energies in fp64"""
    from oracle import hamgnn_ref as R
    from hamgnn_amd import kspace
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    f = G.load("band_energies_openmx_13")
    head = HamGNNPlusPlusOut("4x0e", "4x0e", nao_max=13, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=False, soc_switch=False,
                             calculate_band_energy=True, num_k=5, k_path=None, calculate_sparsity=False)
    head.compile(device)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = R.HamGNNPlusPlusOut("4x0e", "4x0e", nao_max=13, ham_type="openmx")
    finally:
        torch.set_default_dtype(prev)
    g64 = G.to_graph(f["graph"], "cpu", torch.float64)
    Hon, Hoff = (torch.from_numpy(f["inputs"][k]).double().requires_grad_() for k in ("Hon", "Hoff"))
    be, _, gap, _ = ref.calculate_band_energies(Hon, Hoff, g64)
    cot = torch.tensor([0.7, -1.3, 0.4, 1.1][:gap.numel()], dtype=torch.float64)
    (gap * cot).sum().backward()
    val = torch.zeros(119)
    for Z, c in ref.num_valence.items():
        val[int(Z)] = c
    isolated, row = [], 0
    for n0, n, e0, e in kspace._crystal_slices(g64):
        half = math.ceil(float(val[g64.z[n0:n0 + n]].sum()) / 2)
        nb = int((orank_table("openmx", 13)[g64.z[n0:n0 + n]] >= 0).sum())
        isolated.append(gap_is_isolated(be.detach()[row:row + nb].transpose(0, 1), half))
        row += nb
    g = G.to_graph(f["graph"], device)
    g_on, g_off = kspace.band_energy_backward(head, Hon.detach().float().to(device), Hoff.detach().float().to(device), g, None, gap_cotangent=cot.float().to(device))
    if device != "cpu":
        torch.cuda.synchronize()
    return {"crystals": int(gap.numel()), "gap_isolated": all(ok for ok, _ in isolated), "gap_separations": [s for _, s in isolated],
            "g_on_rel_err": G.rel(g_on, Hon.grad), "g_off_rel_err": G.rel(g_off, Hoff.grad)}


# ------------------------------------------------------------------------------------------------ metrics
METRIC_FORMULAS = {
    "cosine_similarity": lambda p, t: (1.0 - (p * t).sum(1) / (p.norm(dim=1) * t.norm(dim=1))).mean(),
    "euclidean_loss": lambda p, t: (p - t).norm(dim=1).mean(),
    "sum_zero": lambda p, t: p.sum(0).norm(),
}


def check_metric(name, rows=37, cols=169, seed=0):
    """training._loss_and_grad vs autograd of the formula (hamgnn/utils/losses.py:5-33) in fp64"""
    from hamgnn_amd.training import _loss_and_grad
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(rows, cols, generator=gen, dtype=torch.float64).requires_grad_()
    t = torch.randn(rows, cols, generator=gen, dtype=torch.float64)
    want = METRIC_FORMULAS[name](p, t)
    want.backward()
    loss, grad = _loss_and_grad(p.detach(), t, name)
    return {"min_row_norm": float(torch.minimum(p.detach().norm(dim=1).min(), t.norm(dim=1).min())), "min_diff_norm": float((p.detach() - t).norm(dim=1).min()),
            "loss_rel_err": abs(float(loss) - float(want.detach())) / abs(float(want.detach())), "grad_rel_err": G.rel(grad, p.grad)}
