"""The split half-precision radial scale (csrc/tp_is.hip, emulated from the same table bytes by tests/emu.py with S_F16) over the RANGE of the hidden rows.
The program is the one of test_plan_emu.test_radial_scale_split_half_precision_twins_vs_oracle (64 hidden units, one 16-edge tile plus a ragged tail of 3);
the hidden rows are scaled directly, so every case compares the split form with the exact (fp32-table) form of the emulator AT THE SAME ROWS.  The bar is
the one that test uses for O(1) rows: wherever the exact form is finite, the split form is finite and rel(split, exact) < 2e-6 (whole-tensor max norm)."""
import numpy as np
import pytest

from hamgnn_amd import plan as P
from tests import emu

IRR, SH_ = "16x0e+12x0o+32x1o+4x1e+7x2e", "0e+1o+2e"
KS = (-30, -24, -20, -14, -10, -6, -3, 0, 3, 6, 8, 9, 10, 12, 14)
BOUND = 2e-6


@pytest.fixture(scope="module")
def case():
    import torch
    from oracle import hamgnn_ref as R
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = R.MessagePackBlock(IRR, IRR, SH_, IRR, "8x0e", radial_MLP=[64, 64])
        E = 19
        g = torch.Generator().manual_seed(1)
        src, dst, ef = (torch.randn(E, ref.irreps_node_feats.dim, generator=g) for _ in range(3))
        n = torch.nn.functional.normalize(torch.randn(E, 3, generator=g), dim=-1)
        rbf = torch.randn(E, 8, generator=g)
    finally:
        torch.set_default_dtype(prev)
    sd = {k: v.detach().numpy() for k, v in ref.state_dict().items()}
    lay = P.PlanarLayout(IRR)
    D = emu.edge_wigner_all(n.numpy(), 2)
    srcs = [emu.rotate_rows(lay.to_planar(t.numpy()), lay, D, 2) for t in (src, dst, ef)]
    hn = emu.radial_hidden(rbf.numpy(), P.radial_hidden_weights(sd, "node_weight_generator", emu.SILU_CST))
    he = emu.radial_hidden(rbf.numpy(), P.radial_hidden_weights(sd, "edge_weight_generator", emu.SILU_CST))
    prog = P.build_message_pack_program(sd, IRR, IRR, SH_, IRR, unrotate=True)
    sc = P.is_schedule(prog)
    assert prog.hidden_pad == 64 and prog.w3_split_ok and int(sc.part_table[0][12]) == 1
    assert 0.5 < np.abs(hn).max() < 16 and 0.5 < np.abs(he).max() < 16          # the unscaled rows are O(1): 2^k sets the range
    return {"prog": prog, "sc": sc, "srcs": srcs, "D": D, "hn": hn, "he": he}


def _both(case, hn, he):
    """(exact, split) outputs of the emulated launch at the hidden rows (hn, he), taken through float32 as the kernel reads them"""
    h2 = tuple(np.asarray(h, dtype=np.float32).astype(np.float64) for h in (hn, he))
    run = lambda: emu.run_program_is(case["prog"], case["sc"], case["srcs"], h2, case["D"], 2)
    with np.errstate(all="ignore"):
        assert not emu.S_F16
        exact = run()
        emu.S_F16 = True
        try:
            split = run()
        finally:
            emu.S_F16 = False
    return exact, split


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _assert_contract(exact, split, tag):
    assert np.isfinite(exact).all() and np.abs(exact).max() > 0, tag
    r = _rel(split, exact) if np.isfinite(split).all() else float("inf")
    print(tag, "finite", bool(np.isfinite(split).all()), "rel(split, exact)", r)
    assert np.isfinite(split).all(), f"{tag}: the split form is not finite where the exact form is"
    assert r < BOUND, (tag, r)
    return r


@pytest.mark.parametrize("k", KS)
def test_uniform_scale(case, k):
    c = 2.0 ** k
    exact, split = _both(case, c * case["hn"], c * case["he"])
    r = _assert_contract(exact, split, f"k={k} max|h|={c * max(np.abs(case['hn']).max(), np.abs(case['he']).max()):.3g}")
    if k == 0:
        assert r > 1e-9                                        # the split path is what ran


def test_mixed_scales_in_one_tile(case):
    """every edge its own 2^k: the whole list inside the first 16-edge tile, its two ends again in the ragged tail.  Asserted: the whole tensor in max norm;
    the worst edge row relative to ITSELF is printed only (a row 2^-30 of the launch's scale is below the contract)."""
    ks = np.array(list(KS) + [0] + [14, -30, 0])
    c = (2.0 ** ks)[:, None]
    exact, split = _both(case, c * case["hn"], c * case["he"])
    _assert_contract(exact, split, "mixed")
    with np.errstate(all="ignore"):
        rows = np.abs(split - exact).max(1) / np.abs(exact).max(1)
    print("mixed: worst edge row relative to itself", float(np.nanmax(rows)), "at k =", int(ks[int(np.nanargmax(rows))]))


@pytest.mark.parametrize("which", ["hn", "he"])
def test_single_outlier_unit(case, which):
    """one unit of one edge at 2^11, everything else O(1): on the node-fed generator's rows, then on the edge-fed one's"""
    h = {"hn": case["hn"].copy(), "he": case["he"].copy()}
    h[which][5, 37] = 2.0 ** 11
    exact, split = _both(case, h["hn"], h["he"])
    _assert_contract(exact, split, f"outlier on {which}")
