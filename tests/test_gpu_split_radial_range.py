"""-m gpu: the split half-precision radial scale of csrc/tp_is.hip over the RANGE of the hidden rows, kernel against the fp64 oracle.
The hidden rows are silu MLP outputs: data times weights, unbounded above, arbitrarily small for edges near the cutoff.  Scaling the radial basis rows by 2^k
moves them (through the bias-free generators roughly in proportion); every check reports the range actually reached.
The bar is no new number.  Wherever the fp32 form of the same build (ops.S_SPLIT_OFF) is finite and within G.TOL of the oracle, the default build is finite and
within G.TOL as well; the fp32 form itself has to pass at every scale from k = -20 to k = 14 (only at k = -30 and k = -24 may a case be excused, by
rel_err_fp32 >= TOL, and it says so)."""
import functools

import pytest
import torch

from tests import gpu_checks as G

pytestmark = pytest.mark.gpu

KS = (-30, -24, -20, -14, -10, -6, -3, 0, 3, 6, 8, 9, 10, 12, 14)
EXCUSABLE = (-30, -24)
E = 37


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rbf_scale(k):
    if k == "mixed":                                           # every edge its own 2^k: the whole list inside each 16-edge tile that is full
        return torch.tensor([2.0 ** KS[e % len(KS)] for e in range(E)], dtype=torch.float64)
    return 2.0 ** k


@functools.lru_cache(maxsize=None)
def _case(seed, parts, k):
    """one forward case, computed once: the parametrized test and the test of the bands read the same result"""
    import bench
    kw = dict(irr=bench.IRREPS[seed], sh=bench.SH, seed=7) if isinstance(seed, str) else dict(seed=seed)
    r = G.check_message_pack_random(radial=(64, 64), E=E, parts=parts, rbf_scale=_rbf_scale(k), **kw)
    print({"seed": seed, "parts": parts, "k": k, **r})
    return r


def _contract(k, finite, pairs, what):
    """pairs: (name, error of the default build, error of the fp32 form).  Returns True when the case took the exit for k in EXCUSABLE."""
    fp32_ok = all(e32 < G.TOL for _, _, e32 in pairs)
    if not fp32_ok:
        assert k in EXCUSABLE, f"{what}: the fp32 form of the same build misses the oracle at k = {k}: {pairs}"
        print(f"EXCUSED {what}: k = {k}, the fp32 form is not within TOL of the oracle: {pairs}")
        return True
    assert finite, f"{what}: not finite where the fp32 form is"
    for name, e, e32 in pairs:
        assert e < G.TOL, (what, name, e, e32)
    return False


@pytest.mark.parametrize("k", list(KS) + ["mixed"])
@pytest.mark.parametrize("parts", [1, None], ids=["single_part", "default_launch"])
@pytest.mark.parametrize("seed", [0, 3])
def test_message_pack_forward_over_the_hidden_rows_range(seed, parts, k):
    """random small irreps sets, 64 hidden units, E = 37 (two full tiles and a tail of 5), `tp_is_kernel<false, false>` (parts = 1: what the benchmark runs) and the
    default split launch.  mixed: asserted in the whole tensor's max norm; the worst edge row relative to itself is in the printed dict only (a row 2^-30 of the
    launch's scale is below the contract)"""
    r = _case(seed, parts, k)
    assert r["kernel"] == "is" and (parts is None or r["parts_used"] == 1), r
    assert (r["parts_used"] != 1) or parts == 1, r             # the default launch of 37 edges is a split launch
    _contract(0 if k == "mixed" else k, r["finite"], [("rel_err", r["rel_err"], r["rel_err_fp32"])], f"seed {seed} parts {parts} k {k}")


def test_the_scales_reach_the_ranges_they_are_there_for():
    """the hidden rows of the cases above on both sides of the edges of the fixed 2^6 exponent this code had: |h| < 1023 stayed finite, |h| < 2^-20 lost its hi half"""
    mx = {k: _case(0, 1, k)["hidden_max_abs"] for k in KS}
    print(mx)
    assert any(512 <= v < 1023 for v in mx.values()), mx
    assert any(1024 <= v < 16384 for v in mx.values()), mx
    assert any(v >= 16384 for v in mx.values()), mx
    assert any(v < 2.0 ** -20 for v in mx.values()), mx
    lo = _case(0, 1, "mixed")
    assert lo["hidden_max_abs"] >= 16384 and lo["hidden_min_row_max_abs"] < 2.0 ** -20, lo       # one launch, both ends


@pytest.mark.parametrize("k", [6, 7])
def test_message_pack_set_a_on_each_side_of_1023(k):
    """the benchmarked irreps set at E = 37, single-part: the two scales whose largest hidden unit lies just below and just above 1023"""
    r = _case("A", 1, k)
    assert r["kernel"] == "is" and r["parts_used"] == 1, r
    assert (512 <= r["hidden_max_abs"] < 1023) if k == 6 else (1024 <= r["hidden_max_abs"] < 4096), r
    _contract(k, r["finite"], [("rel_err", r["rel_err"], r["rel_err_fp32"])], f"set A k {k}")


@pytest.mark.parametrize("parts", [1, None], ids=["single_part", "default_launch"])
@pytest.mark.parametrize("generator", ["node_weight_generator", "edge_weight_generator"])
def test_large_rows_on_one_generator_at_a_time(generator, parts):
    """the node-fed class of phases (hbr_cls == 0) and the edge-fed one (hbr_cls == 1, A.h2[1]) hold their hidden rows in registers on separate paths: the last hidden
    layer of ONE generator times 2^11, the other generator's rows stay O(1)"""
    r = G.check_message_pack_random(radial=(64, 64), E=E, seed=0, parts=parts, gen_scale={generator: 2.0 ** 11})
    print({"generator": generator, "parts": parts, **r})
    assert r["kernel"] == "is" and r["hidden_max_abs"] >= 1024 and r["hidden_min_row_max_abs"] < 64, r
    _contract(11, r["finite"], [("rel_err", r["rel_err"], r["rel_err_fp32"])], f"{generator} x 2^11")


@pytest.mark.parametrize("k", [-20, 0, 9, 11])
def test_message_pack_backward_over_the_hidden_rows_range(k):
    """the adjoint programs run on the same kernel: the data gradients against autograd through the oracle"""
    r = G.check_message_pack_backward(radial=(64, 64), E=E, seed=0, rbf_scale=2.0 ** k)
    print({"k": k, **r})
    assert r["kernel"] == "is", r
    if k >= 9:
        assert r["hidden_max_abs"] >= 1024, r
    _contract(k, r["finite"], [(n, r[n + "_rel_err"], r[n + "_rel_err_fp32"]) for n in ("g_src", "g_dst", "g_edge")], f"backward k {k}")


def test_whole_model_with_one_conv_block_past_1024():
    """a 5-atom cell, every edge launch single-part: the ConvBlocks scatter onto the receivers in the edge kernel's epilogue, so a poisoned tile would spread into
    node rows and from there everywhere.  One generator of the first ConvBlock has its hidden rows past 1024."""
    r = G.oracle_vs_hip_random(radial=(64, 64), num_radial=64, n_atoms=5, parts=1, gen_scale=(0, "node_weight_generator", 2.0 ** 12))
    L = r.pop("launches")
    print(r)
    assert L and all(l["kernel"] == "is" and l["parts"] == 1 for l in L) and sum(l["reduce"] for l in L) >= 1, L
    assert r["hidden_max_abs"] >= 1024, r
    assert r["finite"] and r["H_rel_err"] < G.TOL and r["node_rel_err"] < G.TOL and r["edge_rel_err"] < G.TOL, r
