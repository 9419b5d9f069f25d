"""The row-streaming HIP kernels one by one against their fp64 twins (tests/row_kernel_refs.py), on the cases of tests/row_kernel_checks.py, through
hamgnn_amd.ops: hg_segment_sum, hg_gate, hg_gate_backward, hg_norm_act, hg_norm_act_backward, hg_add_rows, hg_to_planar, hg_from_planar, hg_embed_lookup
(csrc/row_ops.hip), hg_attn_logits, hg_attn_aggregate (csrc/attention.hip), hg_ham_merge, hg_ham_finish, hg_ham_readout, hg_block_mean, hg_soc_assemble
(csrc/head.hip).  The measure is row_kernel_checks.compare -- per row (per irrep copy for the norm activation), relative to the twin's sum of absolute terms --
and the bound is the project's contract gpu_checks.TOL.  Outputs without rounding freedom (copies, one or two fp32 adds, padding slots, structural zeros,
unread gradient columns, the list-order segment sum) are compared for equality, and every kernel is launched twice and has to repeat itself to the bit.
Every test prints `ROWK <entry point> <case> <err / TOL>` before it asserts.

Largest measured err / TOL per entry point on an MI355X, with the case (176 tests, all passing; no value above 0.3, so no thin margin to name):
    hg_segment_sum 0.011 (Dp1028; equal to the list-order fp32 sum on all six cases)      hg_gate 0.027 (hand_rows67)      hg_gate_backward 0.029 (hand_rows67)
    hg_norm_act 0.089 (l4_rows67)      hg_norm_act_backward 0.088 (l4_rows67_strided)      hg_add_rows, hg_to_planar, hg_from_planar, hg_embed_lookup: equal to the
    fp32 emulation on every case (against fp64: 0.006, 0, 0, 0.005)      hg_attn_logits 0.029 (Dp72_H8)      hg_attn_aggregate 0.051 (Dp1028_H8_hand)
    hg_ham_readout 0.011 (nao4_cw200_L2_onsite)      hg_ham_merge + hg_ham_finish 0.011 (nao4_cw200_L2_onsite)      hg_ham_finish alone 0.007 (window)
    hg_block_mean 0.007 (planner_nao19)      hg_soc_assemble 0.007 (soc_no_symmetrize)
hg_norm_act / hg_norm_act_backward by class of the irrep copy's norm n, before -> after the series branch below n = 0.1 (csrc/row_ops.hip:hg_ssp_over_n):
    clamped (n < 1e-8): 1e5 -> 0.0006 / 1e5 -> 0.0006 (the scale came out as 0 instead of 0.5: relative error 1)
    small (1e-8 <= n < 0.05): 1e5 -> 0.011 / 1.2e5 -> 0.016      regular (n >= 0.05): 0.19 -> 0.089 / 0.22 -> 0.088
"""
import pytest
import torch

from tests import row_kernel_checks as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def ops():
    from hamgnn_amd import ops
    return ops


def _cases(builder):
    return builder()                                           # (memoised by row_kernel_checks: built once, seeded, on the CPU)


def _report(entry, name, r, key="err"):
    print(f"ROWK {entry} {name} {r[key] / K.TOL:.4f}")


def _ok(entry, name, r):
    _report(entry, name, r)
    assert r["err"] < K.TOL and r["exact"] and r["repeat"], (entry, name, {k: v for k, v in r.items() if k != "logits"})


@pytest.mark.parametrize("name", sorted(K.segment_sum_cases()))
def test_segment_sum(ops, name):
    _ok("hg_segment_sum", name, K.check_segment_sum(_cases(K.segment_sum_cases)[name], ops, DEV))


@pytest.mark.parametrize("name", sorted(K.gate_cases()))
def test_gate(ops, name):
    _ok("hg_gate", name, K.check_gate(_cases(K.gate_cases)[name], ops, DEV))


@pytest.mark.parametrize("name", sorted(K.gate_cases()))
def test_gate_backward(ops, name):
    _ok("hg_gate_backward", name, K.check_gate(_cases(K.gate_cases)[name], ops, DEV, backward=True))


@pytest.mark.parametrize("name", sorted(K.norm_cases()))
def test_norm_act(ops, name):
    r = K.check_norm_act(_cases(K.norm_cases)[name], ops, DEV)
    for cls in ("clamped", "small", "regular"):
        _report("hg_norm_act[" + cls + "]", name, r, "err_" + cls)
    _ok("hg_norm_act", name, r)


@pytest.mark.parametrize("name", sorted(K.norm_cases()))
def test_norm_act_backward(ops, name):
    r = K.check_norm_act(_cases(K.norm_cases)[name], ops, DEV, backward=True)
    for cls in ("clamped", "small", "regular"):
        _report("hg_norm_act_backward[" + cls + "]", name, r, "err_" + cls)
    _ok("hg_norm_act_backward", name, r)


@pytest.mark.parametrize("name", sorted(K.exact_cases()))
def test_exact_ops(ops, name):
    case = _cases(K.exact_cases)[name]
    _ok("hg_" + case["op"], name, K.check_exact(case, ops, DEV))


@pytest.mark.parametrize("name", sorted(K.attn_cases()))
def test_attention_logits_then_aggregate(ops, name):
    """hg_attn_aggregate is compared with the twin of the soft-max and the weighted sum alone, started from the logits the kernel itself read"""
    case = _cases(K.attn_cases)[name]
    r = K.check_attn_logits(case, ops, DEV)
    _ok("hg_attn_logits", name, r)
    _ok("hg_attn_aggregate", name, K.check_attn_aggregate(case, ops, DEV, logits=r["logits"]))


def test_attention_logits_beyond_the_grid_cap(ops):
    _ok("hg_attn_logits", "wrap_262147_edges", K.check_attn_logits(K.attn_wrap_case(), ops, DEV))


@pytest.mark.parametrize("name", sorted(K.head_cases()))
def test_ham_readout(ops, name):
    _ok("hg_ham_readout", name, K.check_ham_readout(_cases(K.head_cases)[name], ops, DEV))


@pytest.mark.parametrize("name", sorted(K.head_cases()))
def test_ham_merge_then_finish(ops, name):
    _ok("hg_ham_merge+hg_ham_finish", name, K.check_ham_readout(_cases(K.head_cases)[name], ops, DEV, two_launches=True))


def test_ham_readout_persistent_loop(ops):
    (name, case), = K.head_cases(wrap=True).items()
    _ok("hg_ham_readout", name, K.check_ham_readout(case, ops, DEV))


@pytest.mark.parametrize("name", sorted(K.finish_cases()))
def test_ham_finish(ops, name):
    _ok("hg_ham_finish", name, K.check_ham_finish(_cases(K.finish_cases)[name], ops, DEV))


@pytest.mark.parametrize("name", sorted(K.soc_cases()))
def test_block_mean_and_soc_assemble(ops, name):
    case = _cases(K.soc_cases)[name]
    _ok("hg_" + case["op"], name, K.check_soc(case, ops, DEV))


def test_host_refusals_return_before_any_launch(ops):
    """each of these is refused on the host, with the kernel's message, before anything is launched"""
    import numpy as np
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    wide = (torch.zeros(0, 2, dtype=torch.int32, device=DEV), torch.zeros(9000, 2, dtype=torch.int32, device=DEV))      # 72 000 B of tables
    with pytest.raises(RuntimeError, match="row too wide for the LDS tables"):
        ops.gate(z(2, 16), wide, z(5))
    geo = K.attn_geo(torch.zeros(3, dtype=torch.long), torch.zeros(3, dtype=torch.long), torch.ones(3), DEV)
    with pytest.raises(RuntimeError, match="1..8 heads"):
        ops.attention_logits(z(2, 8), geo, z(8, dt=torch.int32), 9, 1, z(1), 6.0)
    with pytest.raises(RuntimeError, match="multiples of 4 floats"):
        ops.segment_sum(z(3, 6), torch.tensor([0, 1, 3], device=DEV), torch.tensor([0, 1, 2], device=DEV), 2)
    with pytest.raises(RuntimeError, match="multiple of the mask width"):
        ops.ham_finish(z(2, 36), None, None, z(3, 4), torch.zeros(2, dtype=torch.long, device=DEV), None, None, 6)
    nao = 40                                                   # 2 nao^2 + 1 table words alone are 12.8 KB; with 4 rows of nao^2 floats: 64 KB are exceeded
    slot = torch.zeros(nao * nao, 4, dtype=torch.int32, device=DEV)
    ptr = torch.arange(nao * nao + 1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="exceed 64 KB of LDS"):
        ops.ham_readout(z(2, 64), None, slot, ptr, torch.zeros(nao * nao, dtype=torch.int32, device=DEV), z(nao * nao), nao, None, None, None, None, None, None,
                        z(2, nao * nao), 0)
    with pytest.raises(RuntimeError, match="multiple of the mask width"):
        ops.ham_readout(z(2, 64), None, slot[:36], ptr[:37], torch.zeros(36, dtype=torch.int32, device=DEV), z(36), 6, None, None, z(3, 4),
                        torch.zeros(2, dtype=torch.long, device=DEV), None, None, z(2, 36), 0)
    assert np.isfinite(float(z(1).sum()))                      # the device is as it was: nothing was launched, nothing is pending
