"""tools/gen_golden_kan.py -- TEST INFRASTRUCTURE ONLY, build container only (needs the reference tree, like oracle/gen_golden.py whose stubs it uses).

Runs the reference's OWN modules with `use_kan=True` -- MessagePackBlock (lite_mode False and True) and a 2-layer HamGNNConvE3 -- in fp64 and writes
{weights incl. the `grid` buffers, inputs, outputs} as data to
    tests/golden/kan_message_pack_block.npz   tests/golden/kan_message_pack_block_lite.npz   tests/golden/backbone_kan.npz
The same state dict goes into the oracle module with its generators swapped for tests/kan_ref.KANRef: both must agree (that pins the restatement).

Block fixtures: with the default initialisation the inner KAN layers see only a few of the 11 input regions (left of the grid, the 9 knot intervals,
right of it), so every KAN layer's base_weight and spline_scaler are multiplied by 6 and rbf = 1.5 randn(83, 8); the script ASSERTS that every region is
populated at every layer.  The backbone fixture keeps the default initialisation and the geometry's rbf (the realistic case).

Usage:  python tools/gen_golden_kan.py        (from the repo root; regenerates the three files byte-identically)
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import e3, gen_golden as GG, hamgnn_ref as R  # noqa: E402
from tests import kan_ref as K  # noqa: E402

MINI, SH = "8x0e+4x0o+4x1o+2x1e+2x2o+3x2e+2x3o", "0e+1o+2e+3o"
E_BLOCK, SCALE = 83, 6.0


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    return os.path.getsize(path)


def save(name, **groups):
    """<name>.npz (+ <name>.part1.npz ... while a file would exceed oracle.gen_golden.GOLD_PART_BYTES: no committed file is larger than 1 MiB), keys
    `group/key` in sorted order, read back as one fixture by tests/gpu_checks.load"""
    flat = {f"{g}/{k}": v for g, d in groups.items() for k, v in GG._np(d).items()}
    stem, tmp = os.path.join(GG.GOLD, name), os.path.join(GG.GOLD, name + ".tmp")
    parts, cur = [], {}
    for k in sorted(flat):
        trial = dict(cur, **{k: flat[k]})
        if cur and write_npz(tmp, trial) > GG.GOLD_PART_BYTES:
            parts.append(cur)
            cur = {k: flat[k]}
        else:
            cur = trial
    parts.append(cur)
    if os.path.exists(tmp):
        os.remove(tmp)
    for i, part in enumerate(parts):
        path = stem + (".npz" if i == 0 else f".part{i}.npz")
        print(f"  wrote tests/golden/{os.path.basename(path)}  ({write_npz(path, part) / 1024:.0f} KiB)")


def kan_modules(m):
    return [c for c in m.modules() if type(c).__name__ == "KAN"]


def settle_spline_weights(m):
    """the reference initialises spline_weight by a least-squares solve whose last bits differ from run to run (LAPACK): round them to fp32 -- what a
    checkpoint of the reference's fp32 training holds -- so that the same script writes the same bytes"""
    with torch.no_grad():
        for kan in kan_modules(m):
            for layer in kan.layers:
                layer.spline_weight.copy_(layer.spline_weight.float().double())


def assert_coverage(kan, rbf, what):
    x = rbf
    for li, layer in enumerate(kan.layers):
        h = K.regions(x.detach(), layer.grid)
        print(f"  {what} layer {li}: region counts {h.tolist()}")
        assert (h > 0).all(), (what, li, h)
        x = layer(x)


def main():
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(1)              # (the reference's KAN initialisation solves a least-squares problem: threaded LAPACK / BLAS sums differ in the last bit from run to run)
    GG.install_stubs()
    ref_mp = importlib.import_module("hamgnn.nn.message_passing")
    ref_conv = importlib.import_module("hamgnn.models.hamgnn_conv")
    D = e3.Irreps(MINI).dim

    for lite in (False, True):
        torch.manual_seed(21 + int(lite))
        ref = ref_mp.MessagePackBlock(MINI, MINI, SH, MINI, "8x0e", radial_MLP=[16, 16], lite_mode=lite, use_kan=True)
        settle_spline_weights(ref)
        with torch.no_grad():
            for kan in kan_modules(ref):
                for layer in kan.layers:
                    layer.base_weight.mul_(SCALE)
                    layer.spline_scaler.mul_(SCALE)
        rbf = 1.5 * torch.randn(E_BLOCK, 8, generator=torch.Generator().manual_seed(0))
        gen = torch.Generator().manual_seed(31 + int(lite))
        src, dst, ef = (torch.randn(E_BLOCK, D, generator=gen) for _ in range(3))
        n = torch.nn.functional.normalize(torch.randn(E_BLOCK, 3, generator=gen), dim=-1)
        sh = e3.spherical_harmonics([0, 1, 2, 3], n, True, "component")
        for kan in kan_modules(ref):
            assert_coverage(kan, rbf, f"lite={lite}")
        sd = dict(ref.state_dict())
        mine = K.swap_generators(R.MessagePackBlock(MINI, MINI, SH, MINI, "8x0e", radial_MLP=[16, 16], lite_mode=lite))
        res = mine.load_state_dict(sd, strict=False)
        assert not res.missing_keys, res.missing_keys
        yr = ref(src, dst, ef, sh, rbf)
        GG._check(mine(src, dst, ef, sh, rbf), yr, f"use_kan MessagePackBlock lite={lite}: swapped oracle vs reference", tol=1e-13)
        keep = {k: v for k, v in sd.items() if k in mine.state_dict()}
        save("kan_message_pack_block_lite" if lite else "kan_message_pack_block", weights=keep,
                 inputs=dict(src=src, dst=dst, edge_feats=ef, sh=sh, rbf=rbf), outputs=dict(out=yr))

    cfg = GG._EasyDict(HamGNN_pre=GG._EasyDict(
        num_types=20, irreps_edge_sh=SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False, cutoff=8.0,
        rbf_func="bessel", num_radial=8, num_layers=2, irreps_node_features=MINI, use_kan=True, radial_MLP=[16, 16], correlation=2,
        num_hidden_features=16, radius_type="openmx", use_corr_prod=False, legacy_edge_update=False, lite_mode=False))
    G = GG.tiny_graph(seed=3, n_atoms=3, zs=(14, 8, 14))
    torch.manual_seed(23)
    ref = ref_conv.HamGNNConvE3(cfg)
    settle_spline_weights(ref)
    mine = K.swap_generators(R.HamGNNConvE3(dict(cfg, HamGNN_pre=dict(cfg.HamGNN_pre, use_kan=False))))
    sd = dict(ref.state_dict())
    res = mine.load_state_dict(sd, strict=False)
    assert not res.missing_keys, res.missing_keys
    rep_ref, rep_mine = ref(GG.Graph(G)), mine(G)
    GG._check(rep_mine["node_attr"], rep_ref["node_attr"], "use_kan backbone node_attr: swapped oracle vs reference", tol=1e-12)
    GG._check(rep_mine["edge_attr"], rep_ref["edge_attr"], "use_kan backbone edge_attr: swapped oracle vs reference", tol=1e-12)
    keep = {k: v for k, v in sd.items() if k in mine.state_dict()}
    save("backbone_kan", weights=keep,
             graph={k: G[k] for k in ("z", "pos", "cell", "edge_index", "nbr_shift", "cell_shift", "inv_edge_idx", "batch", "node_counts")},
             outputs=dict(node_attr=rep_ref["node_attr"], edge_attr=rep_ref["edge_attr"]),
             meta=dict(cfg=np.array(json.dumps(dict(cfg["HamGNN_pre"])))))


if __name__ == "__main__":
    main()
