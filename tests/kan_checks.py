"""Checks of the use_kan path (B-spline KAN weight generators), shared by tests/test_kan_gpu.py (HIP kernels) and tests/test_kan_cpu.py (host logic on the
stand-ins of tests/cpu_ops.py + the stand-in for hg_kan_hidden below).  References: tests/kan_ref.py (fp64) and the reference's own outputs in
tests/golden/kan_*.npz / backbone_kan.npz (tools/gen_golden_kan.py).  Nothing here reads the reference tree."""
import json
import math
import os

import numpy as np
import torch

from tests import gpu_checks as G
from tests import kan_ref as K

# kernel-alone shapes: (layer widths incl. the radial basis and the generator's output, grid size, scale of base_weight / spline_scaler, generators per launch)
KERNEL_SHAPES = {
    "8-16-16": ((8, 16, 16, 156), 3, 6.0, 1),
    "64-64-64_mfma": ((64, 64, 64, 300), 3, 4.0, 1),
    "8-12-20_padded": ((8, 12, 20, 40), 3, 6.0, 1),
    "one_hidden_layer": ((8, 16, 24), 3, 6.0, 1),
    "three_hidden_layers": ((8, 16, 8, 16, 24), 3, 6.0, 1),
    "grid5": ((8, 16, 16, 24), 5, 6.0, 1),
    "three_generators": ((8, 16, 16, 24), 3, 6.0, 3),
    "three_generators_mfma": ((64, 64, 64, 16), 3, 4.0, 3),
    "nonuniform_grid": ((8, 16, 16, 24), 3, 6.0, 1),
}


def make_generators(name, seed=0):
    hs, gs, scale, n = KERNEL_SHAPES[name]
    g = torch.Generator().manual_seed(500 + seed)
    gens = [K.KANRef(hs, gs, generator=g).scale_(scale) for _ in range(n)]
    if name == "nonuniform_grid":                              # strictly increasing, non-uniform, different for every feature (what update_grid leaves behind)
        for layer in gens[0].layers:
            nk = layer.grid.shape[1]
            steps = 0.25 + torch.rand(layer.grid.shape[0], nk - 1, generator=g, dtype=torch.float64)
            t = torch.cat([torch.zeros(layer.grid.shape[0], 1, dtype=torch.float64), steps.cumsum(1)], 1)
            layer.grid.copy_((t / t[:, -1:] * 4.0 - 2.0) * (0.8 + 0.4 * torch.rand(layer.grid.shape[0], 1, generator=g, dtype=torch.float64)))
    return gens


def kernel_inputs(gen0, E, seed=0):
    """1.5 randn; row 0 = exact knots, row 1 = +- the outermost knots, row 2 = +- 5, row 3 = 0 (as far as there are rows)"""
    g = torch.Generator().manual_seed(700 + seed)
    d0 = gen0.hs[0]
    x = 1.5 * torch.randn(E, d0, generator=g, dtype=torch.float64)
    grid = gen0.layers[0].grid
    nk = grid.shape[1]
    idx = torch.arange(d0)
    x[0] = grid[idx, idx % nk]
    if E > 3:
        x[1] = torch.where(idx % 2 == 0, grid[:, 0], grid[:, -1])
        x[2] = torch.where(idx % 2 == 0, torch.tensor(5.0, dtype=torch.float64), torch.tensor(-5.0, dtype=torch.float64))
        x[3] = 0.0
    return x.float()


def check_kan_kernel(device, name, E, seed=0):
    """hg_kan_hidden alone: Phi vs the fp64 features, Phi W3' vs the fp64 generator output (what the edge kernels use; independent of the feature order)"""
    from hamgnn_amd import ops, plan as P
    gens = make_generators(name, seed)
    rbf = kernel_inputs(gens[0], E, seed)
    dgens, W3s = [], []
    for k in gens:
        sd = {"g." + n: v for n, v in K.state_dict_np(k).items()}
        dgens.append(ops.KanGenerator(P.kan_layers(sd, "g"), device))
        W3s.append(P.kan_last_layer(sd, "g"))
    Phi = ops.kan_hidden_multi(rbf.to(device).contiguous(), dgens)
    if device != "cpu":
        torch.cuda.synchronize()
    Phi = Phi.double().cpu()
    out = {"packed": dgens[0].packed, "width": dgens[0].width, "phi_rel_err": 0.0, "out_rel_err": 0.0, "pad_contribution": 0.0, "min_region_count": 10 ** 9}
    for m, (k, (W3, H)) in enumerate(zip(gens, W3s)):
        assert H == dgens[m].width == Phi.shape[2]
        x64 = rbf.double()
        ref_phi, ref_out = k.features(x64), k(x64)
        out["phi_rel_err"] = max(out["phi_rel_err"], G.rel(Phi[m], ref_phi))
        out["out_rel_err"] = max(out["out_rel_err"], G.rel(Phi[m] @ torch.from_numpy(W3), ref_out))
        hl, hp = k.hs[-2], dgens[m].h_pad
        pad = np.ones(H, bool).reshape(-1, hp)
        pad[:, :hl] = False
        pad = pad.reshape(-1)
        if pad.any():                                          # the padded channels contribute exactly nothing: zero rows of W3' (and finite Phi)
            out["pad_contribution"] = max(out["pad_contribution"], float((Phi[m][:, pad].abs() @ torch.from_numpy(np.abs(W3[pad]))).max()))
            assert torch.isfinite(Phi[m]).all()
        for x, layer in zip(k.layer_inputs(x64), k.layers):
            out["min_region_count"] = min(out["min_region_count"], int(K.regions(x, layer.grid).min()))
    return out


# ------------------------------------------------------------------------------------------------ blocks
def _run_block(m, device, irr, sh_l, i, unrotate=True):
    """the path of gpu_checks.check_message_pack: fixture rows -> planar, rotated into the edge frames, MessagePackBlock.run, back"""
    from hamgnn_amd import ops, plan as P
    m.compile(device, unrotate=unrotate)
    lay = P.PlanarLayout(irr)
    E = i["src"].shape[0]
    n = np.asarray(i["sh"])[:, 1:4] / math.sqrt(3.0)
    v = np.stack([n[:, 2], n[:, 0], n[:, 1]], 1) * 2.0
    lm = max(P.Irreps(irr).lmax, sh_l)
    jtab = torch.from_numpy(P.wigner_jtab(lm)).to(device)
    ei = torch.stack([torch.zeros(E, dtype=torch.long), torch.ones(E, dtype=torch.long)]).to(device)
    geo = ops.Geometry(torch.zeros(2, 3, device=device), ei, torch.from_numpy(v).float().to(device), 8.0, 8, lm, jtab)
    geo.rbf = torch.as_tensor(i["rbf"]).float().to(device).contiguous()
    imap = torch.from_numpy(lay.index_map().astype(np.int32)).to(device)
    rot = torch.from_numpy(P.rotate_table(lay)).to(device)
    pl = lambda k: ops.to_planar(torch.as_tensor(i[k]).float().to(device), imap, lay.dim)
    xs, xd, fe = (ops.rotate_gather(pl(k), None, geo, rot) for k in ("src", "dst", "edge_feats"))
    out = m.run(xs, xd, fe, geo)
    if not unrotate:
        out = ops.rotate_gather(out, None, geo, rot, transpose=True)
    y = ops.from_planar(out, imap)
    if device != "cpu":
        torch.cuda.synchronize()
    return y, m


def check_message_pack_kan(device="cuda", lite=False, schedule=None):
    """the reference's own use_kan MessagePackBlock (tests/golden/kan_message_pack_block[_lite].npz)"""
    from hamgnn_amd import nn as hnn
    f = G.load("kan_message_pack_block_lite" if lite else "kan_message_pack_block")
    m = G.load_weights(hnn.MessagePackBlock(G.MINI, G.MINI, G.SH, G.MINI, 8, [16, 16], lite_mode=lite, use_kan=True), f["weights"])
    assert all(k in f["weights"] for k in m.state_dict() if k.endswith(".grid"))
    if schedule is not None:
        os.environ["HG_MP_KERNEL"] = schedule
    try:
        y, m = _run_block(m, device, G.MINI, 3, f["inputs"])
    finally:
        os.environ.pop("HG_MP_KERNEL", None) if schedule is not None else None
    assert schedule is None or (m._dp.sched is not None) == (schedule == "is")
    return {"message_pack_rel_err": G.rel(y, f["outputs"]["out"]), "hidden": m._dp.hidden}


def check_message_pack_random_kan(device="cuda", seed=0, radial=(16, 16), parts=None, E=83, num_radial=8, scale=4.0):
    """gpu_checks.check_message_pack_random with the oracle's generators swapped for KANs"""
    from oracle import hamgnn_ref as R, e3
    from hamgnn_amd import nn as hnn, plan as P
    from tests.test_plan_emu import _random_irreps
    rng = np.random.default_rng(100 + seed)
    lmax = int(rng.integers(1, 4))
    irr = _random_irreps(rng, lmax)
    if "0e" not in irr:
        irr = "5x0e+" + irr
    lsh = int(rng.integers(1, 4))
    sh = "+".join(f"{l}{'e' if l % 2 == 0 else 'o'}" for l in range(lsh + 1))
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = K.swap_generators(R.MessagePackBlock(irr, irr, sh, irr, f"{num_radial}x0e", radial_MLP=list(radial)), seed=seed, scale=scale)
        g = torch.Generator().manual_seed(seed)
        src, dst, ef = (torch.randn(E, ref.irreps_node_feats.dim, generator=g) for _ in range(3))
        n = torch.nn.functional.normalize(torch.randn(E, 3, generator=g) * 3.0, dim=-1)
        shv = e3.spherical_harmonics(list(range(lsh + 1)), n, True, "component")
        rbf = 1.5 * torch.randn(E, num_radial, generator=g)
        out = ref(src, dst, ef, shv, rbf).detach()
    finally:
        torch.set_default_dtype(prev)
    m = G.load_weights(hnn.MessagePackBlock(irr, irr, sh, irr, num_radial, list(radial), use_kan=True), K.state_dict_np(ref))
    os.environ["HG_MP_KERNEL"] = "auto"
    if parts is not None:
        os.environ["HG_IS_PARTS"] = str(parts)
    try:
        y, m = _run_block(m, device, irr, lsh, dict(src=src, dst=dst, edge_feats=ef, sh=shv, rbf=rbf))
        dp = m._dp_for(E)
        return {"irreps": irr, "sh": sh, "kernel": "seg" if dp.sched is None else "is", "parts": dp.is_parts_for(E) if dp.sched is not None else None,
                "hidden": dp.hidden, "rel_err": G.rel(y, out)}
    finally:
        os.environ.pop("HG_MP_KERNEL", None)
        os.environ.pop("HG_IS_PARTS", None)


# ------------------------------------------------------------------------------------------------ backbone
def kan_backbone_from_fixture():
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    f = G.load("backbone_kan")
    cfg = json.loads(str(f["meta"]["cfg"]))
    assert cfg["use_kan"] is True
    m = G.load_weights(HamGNNConvE3(cfg), f["weights"])
    assert all(k in f["weights"] for k in m.state_dict() if k.endswith(".grid"))
    return m, f


def check_backbone_kan(device="cuda"):
    m, f = kan_backbone_from_fixture()
    rep = m(G.to_graph(f["graph"], device))
    if device != "cpu":
        torch.cuda.synchronize()
    return {"backbone_node_rel_err": G.rel(rep["node_attr"], f["outputs"]["node_attr"]), "backbone_edge_rel_err": G.rel(rep["edge_attr"], f["outputs"]["edge_attr"]),
            "generators": len(m._radial_generators())}


def kan_config(radial=(16, 16), num_radial=8, irreps=G.MINI, sh=G.SH, **kw):
    return dict(dict(num_types=96, irreps_edge_sh=sh, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False, cutoff=26.0, rbf_func="bessel",
                     num_radial=num_radial, num_layers=2, irreps_node_features=irreps, use_kan=True, radial_MLP=list(radial), correlation=2, num_hidden_features=16,
                     radius_type="openmx", use_corr_prod=False, legacy_edge_update=False, lite_mode=False), **kw)


def kan_model_and_graph(device, n_atoms=6, seed=0, nao=19, with_oracle=True):
    """(HIP backbone, HIP head, graph on the device, oracle backbone with swapped generators, oracle head, fp64 graph)"""
    from oracle import hamgnn_ref as R
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    cfg = kan_config()
    torch.manual_seed(666 + seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = K.swap_generators(R.HamGNNConvE3(dict(cfg, use_kan=False)), seed=seed)
        ref_head = R.HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=nao, ham_type="openmx", symmetrize=True, add_H0=True, soc_switch=False)
    finally:
        torch.set_default_dtype(prev)
    g = S.add_random_targets(S.random_cell(n_atoms, [14, 8, 6, 1], seed=seed, density=0.004), nao, seed=seed, soc=False)
    hip = G.load_weights(HamGNNConvE3(cfg), K.state_dict_np(ref))
    hip_head = G.load_weights(HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=nao, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=True, soc_switch=False),
                              {k: v for k, v in ref_head.state_dict().items()})
    g64 = type(g)({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in g.items()})
    return hip, hip_head, g.to(device), ref, ref_head, g64


def check_full_forward_kan(device="cuda", n_atoms=6, seed=0):
    """whole model through the head: HIP (fp32) vs the oracle (fp64) with its generators swapped for KANs"""
    hip, hip_head, gd, ref, ref_head, g64 = kan_model_and_graph(device, n_atoms, seed)
    with torch.no_grad():
        rep_ref = ref(g64)
        H_ref = ref_head(g64, rep_ref)["hamiltonian"]
        rep = hip(gd)
        H = hip_head(gd, rep)["hamiltonian"]
    if device != "cpu":
        torch.cuda.synchronize()
    return {"E": int(g64.edge_index.shape[1]), "node_rel_err": G.rel(rep["node_attr"], rep_ref["node_attr"]), "edge_rel_err": G.rel(rep["edge_attr"], rep_ref["edge_attr"]),
            "H_rel_err": G.rel(H, H_ref)}


# ------------------------------------------------------------------------------------------------ CPU stand-in for hg_kan_hidden
def kan_hidden_multi_cpu(rbf, generators):
    """twin of ops.kan_hidden_multi that consumes EXACTLY the packed blob csrc/kan.hip reads (knot tables with their inverted denominators, W' plain or in
    MFMA fragment order), in fp32 like the kernel"""
    outs = []
    for gen in generators:
        b = gen.blob.detach().cpu().numpy()
        dims, Gs = gen.dims, gen.grid_size
        nk, NP = Gs + 7, Gs + 4
        KS = 4 * nk - 6
        x = rbf.detach().cpu().numpy().astype(np.float32)

        def phi(x, kt):                                        # [E, d] , [d, KS] -> [E, NP, d]
            t, r = kt[:, :nk], [None, kt[:, nk:2 * nk - 1], kt[:, 2 * nk - 1:3 * nk - 3], kt[:, 3 * nk - 3:]]
            d = x[:, :, None] - t[None]
            bs = ((x[:, :, None] >= t[None, :, :-1]) & (x[:, :, None] < t[None, :, 1:])).astype(np.float32)
            for k in (1, 2, 3):
                n = nk - 1 - k
                bs = d[:, :, :n] * r[k][None, :, :n] * bs[:, :, :n] - d[:, :, k + 1:k + 1 + n] * r[k][None, :, 1:n + 1] * bs[:, :, 1:n + 1]
            with np.errstate(over="ignore"):
                silu = x / (1.0 + np.exp(-x))
            return np.concatenate([silu[:, None], bs.transpose(0, 2, 1)], 1).astype(np.float32)

        off = 0
        for l in range(len(dims) - 1):
            di, dn = dims[l], dims[l + 1]
            kt = b[off:off + di * KS].reshape(di, KS)
            off += di * KS
            W = b[off:off + NP * di * dn]
            off += NP * di * dn
            if gen.packed:                                     # [T, p, rt, g, i, q] -> [p, T, g, q, rt, i]
                W = W.reshape(4, NP, 4, 4, 16, 4).transpose(1, 0, 3, 5, 2, 4)
            x = np.einsum("epi,pio->eo", phi(x, kt), W.reshape(NP, di, dn)).astype(np.float32)
        dl = dims[-1]
        kt = b[off:off + dl * KS].reshape(dl, KS)
        assert off + dl * KS == b.size
        out = np.zeros((x.shape[0], NP, gen.h_pad), np.float32)
        out[:, :, :dl] = phi(x, kt)
        outs.append(torch.from_numpy(out.reshape(x.shape[0], NP * gen.h_pad)))
    return torch.stack(outs)


def install_cpu(monkeypatch):
    """tests/cpu_ops.install + the stand-in above"""
    from hamgnn_amd import ops
    from tests import cpu_ops
    cpu_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "kan_hidden_multi", kan_hidden_multi_cpu)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
