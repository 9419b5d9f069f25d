"""Checks of HamGNN_pre.build_internal_graph (hamgnn_amd/internal_graph.py + the hg_neighbour_* kernels of csrc/neighbour.hip), shared by
tests/test_internal_graph_gpu.py (HIP kernels) and tests/test_internal_graph_cpu.py (host logic on the stand-ins of tests/cpu_ops.py + the numpy twin of the
three neighbour-list entry points below, which follows the kernels' binning and loop structure).

The exact statement of the neighbour rule is hamgnn_amd/data/synthetic.py:build_graph (cKDTree, fp64) run on the fp32-rounded positions and cell: the edge
lists must be bit-equal to it.  Every comparison first asserts, in fp64 on the host, that no candidate pair lies within 1e-9 Bohr of its cut-off, so the
edge set does not hang on the last bit of a distance.  Nothing here reads the reference tree."""
import numpy as np
import torch

from tests import gpu_checks as G

SCALE = 1.5
MARGIN = 1e-9
S_OFF, S_MAX = 16, 15


# ------------------------------------------------------------------------------------------------ crystals
def _random_cell_inputs(n_atoms, zs, seed=0, density=0.012):
    """the positions / cell / species synthetic.random_cell draws (same generator calls in the same order), without the neighbour search"""
    rng = np.random.default_rng(seed)
    L = (n_atoms / density) ** (1 / 3)
    m = int(np.ceil(n_atoms ** (1 / 3)))
    grid = np.array([(i, j, k) for i in range(m) for j in range(m) for k in range(m)], dtype=np.float64)
    rng.shuffle(grid)
    pos = (grid[:n_atoms] + 0.5) * (L / m) + rng.uniform(-0.6, 0.6, size=(n_atoms, 3))
    z = rng.choice(np.asarray(zs), size=n_atoms)
    return pos, np.diag([L, L, L]) + rng.normal(0, 0.2, size=(3, 3)), z


def heights(cell):
    vol = abs(np.linalg.det(cell))
    return vol / np.array([np.linalg.norm(np.cross(cell[1], cell[2])), np.linalg.norm(np.cross(cell[2], cell[0])), np.linalg.norm(np.cross(cell[0], cell[1]))])


def bins_per_direction(cell32, rcut):
    """floor(height / rcut) along every lattice direction of the fp32-rounded cell (what hg_neighbour_bin starts from)"""
    return np.floor(heights(np.asarray(cell32, dtype=np.float32).astype(np.float64)) / (rcut * (1.0 + 1e-9))).astype(int)


_WRAP = {}


def wrap_crystal(zs=(14, 8, 1), seed=0, density=0.004, scale=SCALE):
    """the smallest random_cell(n, zs, seed, density) whose cell holds at least three bins along every lattice vector at `scale`
    -> (graph, n_atoms, bins per direction, bin width = largest r_i + r_j)"""
    key = (tuple(zs), seed, density, scale)
    if key not in _WRAP:
        from hamgnn_amd.data import synthetic as S
        from hamgnn_amd.internal_graph import radius_table
        tab = radius_table("openmx", scale).numpy()
        n = max(1, int(density * (3 * 2 * tab[list(zs)].max() * 0.97) ** 3))
        while True:
            pos, cell, z = _random_cell_inputs(n, list(zs), seed, density)
            rcut = 2 * tab[z].max()
            nb = bins_per_direction(cell, rcut)
            if nb.min() >= 3:
                break
            n += 1
        g = S.random_cell(n, list(zs), seed=seed, density=density)
        assert np.array_equal(g.pos.numpy(), pos.astype(np.float32)) and np.array_equal(g.z.numpy(), z)       # the helper above draws what random_cell draws
        _WRAP[key] = (g, n, nb, rcut)
    return _WRAP[key]


_CRYSTALS = {}


def crystal(name):
    """the crystals of the issue (data graphs: the Hamiltonian's own sparsity pattern, radius_scale 1.0)"""
    if name not in _CRYSTALS:
        from hamgnn_amd.data import synthetic as S, collate
        if name == "si2":                                      # 2 atoms: every neighbour is an image, self images, several images per direction
            g = S.si_diamond(primitive=True)
        elif name == "skew5":                                  # skewed cell, three species (Si 7.0, O and H 6.0 Bohr in the openmx table)
            g = S.random_cell(5, [14, 8, 1], seed=4)
            assert len(set(g.z.tolist())) == 3
        elif name == "batch3":                                 # 1 + 2 + 5 atoms: cumulative offsets, a crystal with self images only
            g = collate([S.random_cell(1, [14], seed=1), S.si_diamond(primitive=True), S.random_cell(5, [14, 8, 1], seed=4)])
        elif name == "wrap":
            g = wrap_crystal()[0]
        else:
            raise KeyError(name)
        _CRYSTALS[name] = g
    return _CRYSTALS[name]


def split_crystals(g):
    """[(pos32 as fp64, cell32 as fp64, z, first atom)] per crystal of a (batched) graph"""
    nc = g["node_counts"].tolist() if "node_counts" in g else [g.num_nodes]
    cells = g["cell"].reshape(-1, 3, 3)
    out, o = [], 0
    for b, n in enumerate(nc):
        out.append((g["pos"][o:o + n].numpy().astype(np.float64), cells[b].numpy().astype(np.float64), g["z"][o:o + n].numpy(), o))
        o += n
    return out


def assert_margin(g, scale=SCALE, margin=MARGIN):
    """fp64 on the host: no periodic pair of `g` lies within `margin` of its cut-off radius_scale (r_i + r_j).  Returns the smallest gap."""
    from hamgnn_amd.internal_graph import radius_table
    tab = radius_table("openmx", scale).numpy()
    worst = np.inf
    for pos, cell, z, _ in split_crystals(g):
        rad = tab[z]
        cut = rad[:, None] + rad[None, :]
        nimg = np.ceil(cut.max() / heights(cell)).astype(int)
        for a in range(-nimg[0], nimg[0] + 1):
            for b in range(-nimg[1], nimg[1] + 1):
                for c in range(-nimg[2], nimg[2] + 1):
                    d = np.linalg.norm(pos[None, :, :] + (np.array([a, b, c], dtype=np.float64) @ cell)[None, None, :] - pos[:, None, :], axis=2)
                    worst = min(worst, float(np.abs(d - cut).min()))
    assert worst > margin, f"a pair lies {worst:.3e} Bohr from its cut-off: pick another seed"
    return worst


_HOST = {}


def host_internal(name, scale=SCALE):
    """synthetic.build_graph on the fp32-rounded positions and cell of crystal `name` at `scale` (per crystal, collated), cached and never modified"""
    if (name, scale) not in _HOST:
        from hamgnn_amd.data import synthetic as S, collate
        gs = [S.build_graph(pos, cell, z, radius_scale=scale) for pos, cell, z, _ in split_crystals(crystal(name))]
        _HOST[(name, scale)] = gs[0] if len(gs) == 1 else collate(gs)
    return _HOST[(name, scale)]


def host_match(g_data, g_int):
    """index of every data edge (i, j, S) in the internal list, by rows on the host"""
    rows = lambda g: np.concatenate([g["edge_index"].numpy().T, g["cell_shift"].numpy()], 1).astype(np.int64)
    where = {tuple(r): k for k, r in enumerate(rows(g_int).tolist())}
    return torch.tensor([where[tuple(r)] for r in rows(g_data).tolist()], dtype=torch.long)


def check_edge_list(name, device, scale=SCALE):
    """the device (or twin) list of crystal `name` against the host statement, and matching_edges against the data's own edges"""
    from hamgnn_amd.internal_graph import build_internal_graph
    g = crystal(name)
    gap = assert_margin(g, scale)
    ref = host_internal(name, scale)
    ig = build_internal_graph(g.to(device), "openmx", scale)
    if device != "cpu":
        torch.cuda.synchronize()
    ig = ig.to("cpu")
    m = ig["matching_edges"]
    same = lambda k: ig[k].dtype == ref[k].dtype and ig[k].shape == ref[k].shape and torch.equal(ig[k], ref[k])
    return {"name": name, "N": g.num_nodes, "E_data": g.num_edges, "E_internal": int(ig["edge_index"].shape[1]), "E_host": ref.num_edges, "gap": gap,
            "edge_index_equal": same("edge_index"), "cell_shift_equal": same("cell_shift"), "nbr_shift_equal": same("nbr_shift"),
            "match_reproduces_data": bool(m.shape[0] == g.num_edges and torch.equal(ig["edge_index"][:, m], g["edge_index"]) and torch.equal(ig["cell_shift"][m], g["cell_shift"])),
            "match_equals_host": torch.equal(m, host_match(g, ref)), "max_image": int(ig["cell_shift"].abs().max()),
            "self_images": int((ig["edge_index"][0] == ig["edge_index"][1]).sum())}


# ------------------------------------------------------------------------------------------------ whole model
T_IRREPS = "8x0e+4x0o+4x1o+2x1e+2x2o+4x2e+2x3o"            # (multiplicities divisible by the two heads: the irreps of the existing transformer tests)


def irreps_of(transformer):
    return T_IRREPS if transformer else G.MINI


def config(on, transformer=False, **kw):
    cfg = dict(num_types=96, irreps_edge_sh=G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=bool(on), cutoff=26.0,
               rbf_func="bessel", num_radial=8, num_layers=2, irreps_node_features=irreps_of(transformer), use_kan=False, radial_MLP=[16, 16], correlation=2, num_hidden_features=4,
               radius_type="openmx", use_corr_prod=False, legacy_edge_update=False, lite_mode=False)
    if on:
        cfg["radius_scale"] = SCALE
    if transformer:
        cfg["num_heads"] = 2
    return dict(cfg, **kw)


def _fp64(g):
    return type(g)({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in g.items()})


def models(name="skew5", transformer=False, nao=19, seed=0, add_H0=True, num_types=96):
    """(oracle backbone [switch off], oracle head, HIP backbone switch ON, HIP backbone switch OFF, HIP head, data graph with targets, host-built internal graph)
    -- one set of weights"""
    from oracle import hamgnn_ref as R
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    from hamgnn_amd.models.hamgnn_transformer import HamGNNTransformer
    irr = irreps_of(transformer)
    torch.manual_seed(777 + seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        rb = (R.HamGNNTransformer if transformer else R.HamGNNConvE3)(config(False, transformer, num_types=num_types))
        rh = R.HamGNNPlusPlusOut(irr, irr, nao_max=nao, ham_type="openmx", symmetrize=True, add_H0=add_H0, soc_switch=False)
    finally:
        torch.set_default_dtype(prev)
    Backbone = HamGNNTransformer if transformer else HamGNNConvE3
    on = G.load_weights(Backbone(config(True, transformer, num_types=num_types)), dict(rb.state_dict()))
    off = G.load_weights(Backbone(config(False, transformer, num_types=num_types)), dict(rb.state_dict()))
    head = G.load_weights(HamGNNPlusPlusOut(irr, irr, nao_max=nao, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=add_H0, soc_switch=False,
                                            calculate_sparsity=False), dict(rh.state_dict()))
    g0 = crystal(name)
    g = S.add_random_targets(type(g0)({k: (v.clone() if torch.is_tensor(v) else v) for k, v in g0.items() if not k.startswith("_hg")}), nao, seed=seed, soc=False)
    return rb, rh, on, off, head, g, host_internal(name)


def _gathered(rep_off, rows):
    """the representation of a switch-off forward on the internal graph, cut back to the data's edges `rows` (what the head reads: planar rows + geometry)"""
    from hamgnn_amd.internal_graph import restrict_geometry
    from hamgnn_amd.models.hamgnn_conv import Representation
    rep = Representation()
    rep["_node_planar"], rep["_edge_planar_rot"] = rep_off["_node_planar"], rep_off["_edge_planar_rot"].index_select(0, rows)
    rep["_geometry"] = restrict_geometry(rep_off["_geometry"], rows)
    return rep


def check_model_hip_vs_hip(device, name="skew5", transformer=False):
    """build_internal_graph=True on the data graph  vs  the same weights, switch off, on the host-built internal graph and then gathered: same launches, so the
    node rows, the edge rows and the head's Hamiltonian must not differ at all"""
    assert_margin(crystal(name))
    _, _, on, off, head, g, gi = models(name, transformer)
    rows = host_match(g, gi).to(device)
    gd, gid = g.to(device), gi.to(device)
    with torch.no_grad():
        rep_on = on(gd)
        H_on = head(gd, rep_on)["hamiltonian"]
        rep_off = off(gid)
        H_off = head(gd, _gathered(rep_off, rows))["hamiltonian"]
        node_on, edge_on, node_off, edge_off = rep_on["node_attr"], rep_on["edge_attr"], rep_off["node_attr"], rep_off["edge_attr"].index_select(0, rows)
    if device != "cpu":
        torch.cuda.synchronize()
    d = lambda a, b: float((a.double() - b.double()).abs().max())
    return {"E_data": g.num_edges, "E_internal": gi.num_edges, "edge_rows": tuple(rep_on["_edge_planar_rot"].shape), "geometry_rows": rep_on["_geometry"].E,
            "edge_attr_rows": int(edge_on.shape[0]), "node_diff": d(node_on, node_off), "edge_diff": d(edge_on, edge_off), "H_diff": d(H_on, H_off),
            "H_rows": int(H_on.shape[0]), "H_absmax": float(H_on.abs().max())}


def check_model_vs_oracle(device, name="skew5"):
    """the fp64 oracle with the switch off on the host-built internal graph, gathered by the host-side match, then its head"""
    assert_margin(crystal(name))
    rb, rh, on, _, head, g, gi = models(name)
    rows = host_match(g, gi)
    g64, gi64 = _fp64(g), _fp64(gi)
    with torch.no_grad():
        rep_ref = rb(gi64)
        rep_ref["edge_attr"] = rep_ref["edge_attr"][rows]
        H_ref = rh(g64, rep_ref)["hamiltonian"]
        gd = g.to(device)
        rep = on(gd)
        H = head(gd, rep)["hamiltonian"]
    if device != "cpu":
        torch.cuda.synchronize()
    return {"E_data": g.num_edges, "E_internal": gi.num_edges, "node_rel_err": G.rel(rep["node_attr"], rep_ref["node_attr"]),
            "edge_rel_err": G.rel(rep["edge_attr"], rep_ref["edge_attr"]), "H_rel_err": G.rel(H, H_ref)}


def check_training(device, name="skew5", transformer=False):
    """every parameter gradient of one training_step with the switch on vs torch.autograd through the oracle chain in fp64 (gpu_checks.check_full_backward's comparison)"""
    from hamgnn_amd.models.model import Model
    from hamgnn_amd.training import training_step
    assert_margin(crystal(name))
    rb, rh, on, _, head, g, gi = models(name, transformer, add_H0=False, num_types=20)
    rows = host_match(g, gi)
    g64, gi64 = _fp64(g), _fp64(gi)
    rep_ref = rb(gi64)
    rep_ref["edge_attr"] = rep_ref["edge_attr"][rows]
    Href = rh(g64, rep_ref)["hamiltonian"]
    target = 0.1 * torch.randn(Href.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    loss_ref = ((Href - target) ** 2).mean()
    model = Model(on, head).to(device)
    r = training_step(model, g.to(device), metric="mse", target=target.float().to(device))
    if device != "cpu":
        torch.cuda.synchronize()
    loss_ref.backward()
    worst = {}
    for mod, ref in ((model.representation, rb), (model.output_module, rh)):
        refp = dict(ref.named_parameters())
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            want = refp[k].grad if refp[k].grad is not None else torch.zeros_like(refp[k])
            worst[k] = float((p.grad.double().cpu().reshape(want.shape) - want).abs().max()) / max(float(want.abs().max()), 1e-6)
    k = max(worst, key=worst.get)
    return {"E_data": g.num_edges, "E_internal": gi.num_edges, "loss_rel_err": abs(float(r["loss"]) - float(loss_ref.detach())) / abs(float(loss_ref.detach())),
            "n_params": len(worst), "max_rel_err": worst[k], "worst": k}


def count_builds(monkeypatch):
    """-> list that grows by one per neighbour-list build (spy on ops.neighbour_bin, whichever implementation is installed)"""
    from hamgnn_amd import ops
    calls, real = [], ops.neighbour_bin

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "neighbour_bin", spy)
    return calls


def check_cache(device, monkeypatch):
    from hamgnn_amd.internal_graph import CACHE_ATTR, get_internal_graph
    from hamgnn_amd.parallel import shard_graph
    calls = count_builds(monkeypatch)
    g0 = crystal("skew5")
    g = type(g0)({k: (v.clone() if torch.is_tensor(v) else v) for k, v in g0.items() if not k.startswith("_hg")}).to(device)      # (own tensors: changed in place below)
    a = get_internal_graph(g, "openmx", SCALE)
    b = get_internal_graph(g, "openmx", SCALE)
    once = (len(calls), a is b)
    g.pos.add_(0.01)
    c = get_internal_graph(g, "openmx", SCALE)
    moved = (len(calls), c is not a)
    d = get_internal_graph(g, "openmx", 1.25)
    host = g.to("cpu")
    dict.__setitem__(host, CACHE_ATTR, g[CACHE_ATTR])
    return {"once": once, "after_inplace_change": moved, "other_scale": (len(calls), d is not c), "to_drops": CACHE_ATTR in g and CACHE_ATTR not in g.to(device),
            "shard_drops": CACHE_ATTR in host and CACHE_ATTR not in shard_graph(host, 0, 2)}


# ------------------------------------------------------------------------------------------------ numpy twin of hg_neighbour_bin / _pairs / _decode
def _flag(flags, bit):
    flags[0] |= bit


def neighbour_bin_cpu(pos, cell, batch, atom_ptr, rcut, flags):
    """twin of ops.neighbour_bin: nl_setup_kernel, nl_bin_offsets_kernel, nl_bin_kernel"""
    from hamgnn_amd import ops
    N, B = int(pos.shape[0]), int(cell.shape[0])
    bins_cap = N + 27 * B
    cpar, ipar = np.zeros((B, 20)), np.zeros((B, 8), np.int32)
    rc = float(rcut[0]) * (1.0 + 1e-9)
    off = 0
    for b in range(B):
        a = cell[b].numpy().astype(np.float64)
        c = np.stack([np.cross(a[(d + 1) % 3], a[(d + 2) % 3]) for d in range(3)])
        det = float(a[0] @ c[0])
        nb, nimg, bad = [1, 1, 1], [0, 0, 0], 0
        if not (abs(det) > 0 and np.isfinite(det) and rc > 0 and np.isfinite(rc)):
            bad |= 1
        else:
            for d in range(3):
                h = abs(det) / np.linalg.norm(c[d])
                q = h / rc
                if q >= 3.0:
                    nb[d] = int(min(q, 1024.0))
                else:
                    m = np.ceil(rc / h)
                    if not m <= S_MAX:
                        bad |= 2
                    else:
                        nimg[d] = int(m)
            n_b = int(atom_ptr[b + 1] - atom_ptr[b])
            for _ in range(3 * 1024):
                if nb[0] * nb[1] * nb[2] <= n_b:
                    break
                d = (0 if nb[0] >= nb[2] else 2) if nb[0] >= nb[1] else (1 if nb[1] >= nb[2] else 2)
                if nb[d] <= 3:
                    break
                nb[d] -= 1
        if bad:
            nb, nimg = [1, 1, 1], [0, 0, 0]
            _flag(flags, bad)
        cpar[b, :9] = a.reshape(-1)
        cpar[b, 9:18] = 0.0 if bad else (c.T / det).reshape(-1)      # [3 k + d] = c_d[k] / det
        cpar[b, 18] = rc
        ipar[b] = nb + nimg + [off, nb[0] * nb[1] * nb[2]]
        off += int(ipar[b, 7])
    assert off <= bins_cap
    p = pos.numpy().astype(np.float64)
    bt = np.zeros(N, np.int64) if batch is None else batch.numpy()
    bin_id, wrap = np.zeros(N, np.int64), np.zeros((N, 3), np.int32)
    for i in range(N):
        b = int(bt[i])
        f = p[i] @ cpar[b, 9:18].reshape(3, 3)
        w = np.floor(f)
        k = 0
        for d in range(3):
            nb = int(ipar[b, d])
            k = k * nb + min(max(int((f[d] - w[d]) * nb), 0), nb - 1)
        bin_id[i], wrap[i] = ipar[b, 6] + k, w.astype(np.int32)
    return ops.CellList(torch.from_numpy(cpar), torch.from_numpy(ipar), torch.from_numpy(bin_id), torch.from_numpy(wrap), bins_cap, B)


def neighbour_pairs_cpu(pos, radius, batch, cl, flags, seg_ptr=None, capacity=0):
    """twin of ops.neighbour_pairs (nl_pairs_kernel): per centre, the 3 x 3 x 3 bins with wrap-around or the images of a one-bin direction, in the kernel's loop order"""
    N = int(pos.shape[0])
    p, rad = pos.numpy().astype(np.float64), radius.numpy()
    bt = np.zeros(N, np.int64) if batch is None else batch.numpy()
    cpar, ipar, bin_id, wrap = cl.cpar.numpy(), cl.ipar.numpy(), cl.bin_id.numpy(), cl.wrap.numpy().astype(np.int64)
    bstart, batoms = cl.bin_start.numpy(), cl.bin_atoms.numpy()
    counts = np.zeros(N, np.int64)
    keys = None if seg_ptr is None else np.full(int(capacity), -7, np.int64)
    for i in range(N):
        b = int(bt[i])
        a = cpar[b, :9].reshape(3, 3)
        nb, nimg, boff = [int(v) for v in ipar[b, :3]], [int(v) for v in ipar[b, 3:6]], int(ipar[b, 6])
        lb = int(bin_id[i]) - boff
        bc = [lb // (nb[1] * nb[2]), (lb // nb[2]) % nb[1], lb % nb[2]]
        rng = [1 if nb[d] >= 3 else nimg[d] for d in range(3)]
        out = 0

        def step(d, o):
            if nb[d] < 3:
                return 0, o
            c = bc[d] + o
            return (c + nb[d], -1) if c < 0 else ((c - nb[d], 1) if c >= nb[d] else (c, 0))
        for o0 in range(-rng[0], rng[0] + 1):
            c0, m0 = step(0, o0)
            for o1 in range(-rng[1], rng[1] + 1):
                c1, m1 = step(1, o1)
                for o2 in range(-rng[2], rng[2] + 1):
                    c2, m2 = step(2, o2)
                    gbin = boff + (c0 * nb[1] + c1) * nb[2] + c2
                    js = batoms[bstart[gbin]:bstart[gbin + 1]]
                    if js.size == 0:
                        continue
                    s = np.array([m0, m1, m2], np.int64)[None, :] - wrap[js] + wrap[i][None, :]
                    v = p[js] + s.astype(np.float64) @ a - p[i][None, :]
                    keep = (np.sqrt((v * v).sum(1)) < rad[i] + rad[js]) & ~((js == i) & (np.abs(s).sum(1) == 0))
                    if (np.abs(s[keep]) > S_MAX).any():
                        _flag(flags, 2)
                        keep &= (np.abs(s) <= S_MAX).all(1)
                    for j, sj in zip(js[keep].tolist(), s[keep].tolist()):
                        if keys is not None:
                            if int(seg_ptr[i]) + out < min(int(seg_ptr[i + 1]), int(capacity)):
                                keys[int(seg_ptr[i]) + out] = (i << 39) | (j << 15) | ((sj[0] + S_OFF) << 10) | ((sj[1] + S_OFF) << 5) | (sj[2] + S_OFF)
                            else:
                                _flag(flags, 4)
                        out += 1
        counts[i] = out
        if keys is not None and out != int(seg_ptr[i + 1] - seg_ptr[i]):
            _flag(flags, 4)
    return torch.from_numpy(counts if keys is None else keys)


def neighbour_decode_cpu(keys, cell, batch, N):
    k = keys.numpy()
    i, j = (k >> 39) & 0xFFFFFF, (k >> 15) & 0xFFFFFF
    s = np.stack([((k >> 10) & 31) - S_OFF, ((k >> 5) & 31) - S_OFF, (k & 31) - S_OFF], 1)
    b = np.zeros_like(i) if batch is None else batch.numpy()[i]
    c = cell.numpy().astype(np.float64)[b]                      # [E, 3, 3]
    ns = (s[:, 0:1] * c[:, 0] + s[:, 1:2] * c[:, 1] + s[:, 2:3] * c[:, 2]).astype(np.float32)
    return torch.from_numpy(np.stack([i, j])), torch.from_numpy(s.astype(np.int64)), torch.from_numpy(ns)


def install_cpu(monkeypatch):
    """tests/cpu_ops.install + the numpy twin of the neighbour-list entry points"""
    from hamgnn_amd import ops
    from tests import cpu_ops
    cpu_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "neighbour_bin", neighbour_bin_cpu)
    monkeypatch.setattr(ops, "neighbour_pairs", neighbour_pairs_cpu)
    monkeypatch.setattr(ops, "neighbour_decode", neighbour_decode_cpu)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
