"""-m gpu: phases whose tensor-product items use BOTH radial generators (phase record [5], plan/schedule_is.py) keep both generators' hidden rows resident in
csrc/tp_is.hip, each set split into half-precision halves with the exponent of ITS OWN rows.
The mini block with 64 hidden units, scheduled as one such phase, on 24 edges (a full tile and a last tile of 8): the last hidden layer of one generator is scaled by 2^-10
and the other's by 16 (and the other way round): rows 2^14 apart, where an exponent shared by the two sets would push the smaller set's low halves into the
half-precision subnormals, which the matrix pipe flushes.
  * against the fp64 oracle: G.TOL, under the contract of tests/test_gpu_split_radial_range.py (the fp32 form of the same build has to be within G.TOL as well);
  * against the same launch with the fp32 radial scale (HG_S_SPLIT=0 = ops.S_SPLIT_OFF): G.SAME_MATH_TOL = 5e-6.
The first-layer model case of tests/test_centre_edge_model.py (set-A, 60-atom a-SiO2: the reduced programs, whose mixed phases this is for) runs again against the
complete programs (HG_STRUCT_ZEROS=0)."""
import contextlib

import pytest
import torch

from tests import centre_checks as C
from tests import gpu_checks as G
from tests.test_centre_edge_model import SET_A, SH_A

pytestmark = pytest.mark.gpu

SMALL, LARGE = 2.0 ** -10, 16.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def spy_phase_tables():
    """the phase table of the schedule every ops.tp_fused call inside the block launches"""
    from hamgnn_amd import ops
    seen, real = [], ops.tp_fused

    def spy(dp, srcs, rows, *a, **kw):
        if dp.sched is not None:
            seen.append(dp.is_tables(dp.is_parts_for(int(rows)))[0].phase_table.copy())
        return real(dp, srcs, rows, *a, **kw)

    ops.tp_fused = spy
    try:
        yield seen
    finally:
        ops.tp_fused = real


@pytest.mark.parametrize("parts", [1, None], ids=["single_part", "default_launch"])
@pytest.mark.parametrize("small", ["node_weight_generator", "edge_weight_generator"])
def test_mixed_phase_with_hidden_rows_far_apart(small, parts, monkeypatch):
    """single_part: `tp_is_two_kernel<false>` (one workgroup per tile, the benchmark's form) on the block's one-phase schedule -- with 64 hidden units is_schedule would pick the form with one generator per
    phase for a single-part launch of this block, so the mixed form (what it picks for the reduced first-layer programs) is asked for by name;
    default_launch: the split launch of 24 edges (`tp_is_two_kernel<true>`), whose schedules are always of the mixed form"""
    from hamgnn_amd import plan as P
    large = "edge_weight_generator" if small == "node_weight_generator" else "node_weight_generator"
    kept = {}
    real, real_schedule = G.split_and_fp32, P.is_schedule

    def keep(run):
        kept["split"], kept["fp32"] = real(run)
        return kept["split"], kept["fp32"]

    monkeypatch.setattr(G, "split_and_fp32", keep)
    if parts == 1:
        monkeypatch.setattr(P, "is_schedule", lambda prog, parts=1, separate_mlp=None: real_schedule(prog, parts, separate_mlp=False))
    with spy_phase_tables() as tables:
        r = G.check_message_pack_random(irr=G.MINI, sh=G.SH, radial=(64, 64), E=24, seed=1, parts=parts, gen_scale={small: SMALL, large: LARGE})
    same = G.rel(kept["split"], kept["fp32"].double().cpu())
    print({"small": small, **r, "rel_diff_vs_fp32_form": same, "phases": [t[:, 4:6].tolist() for t in tables[:1]]})
    assert r["kernel"] == "is" and (r["parts_used"] == 1) == (parts == 1), r
    if parts == 1:
        assert tables and all(t.shape[0] == 1 and int(t[0][4]) >= 0 and int(t[0][5]) == 1 for t in tables), tables      # one phase, both generators
    else:
        assert tables and all(t[:, 5].any() for t in tables), tables
    assert r["hidden_max_abs"] >= 2.0 ** 13 * r["hidden_min_row_max_abs"], r                                         # the sets are that far apart
    assert r["rel_err_fp32"] < G.TOL, r
    assert r["finite"] and r["rel_err"] < G.TOL, r
    assert same < G.SAME_MATH_TOL, same


def test_first_layer_model_set_a_against_the_complete_programs():
    from hamgnn_amd.data import synthetic as S
    r = C.check_centre_zeros(irr=SET_A, sh=SH_A, radial=(64, 64), num_radial=64, graph=S.amorphous_sio2(60, seed=1))
    print(r)
    assert all(k == "is" and p == "1" for k, p, _ in r["launches"]), r
    assert r["node_rel_err_vs_complete"] < G.SAME_MATH_TOL and r["edge_rel_err_vs_complete"] < G.SAME_MATH_TOL, r
