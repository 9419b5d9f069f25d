"""The row-streaming kernels' cases without a GPU: (1) every case's coverage conditions hold -- computed from the inputs and the fp64 twins alone, so a case
that misses one is a broken test, not a skipped one; (2) the twins of tests/row_kernel_refs.py agree with the stand-ins of tests/cpu_ops.py on every case
(to 1e-6 by the comparison the GPU tests use, or to the bit where the stand-in is exact), which ties the operations the CPU suite runs to their definition;
(3) sharpness: for every operation a deliberately wrong twin is rejected by the same comparison at the bound the GPU tests apply."""
import numpy as np
import pytest
import torch

from tests import cpu_ops
from tests import row_kernel_checks as K
from tests import row_kernel_refs as R

TIE = 1e-6


def _cover(case):
    for k in case["require"]:
        assert case["cover"][k] > 0, (k, case["cover"])


def _ids(d):
    return sorted(d)


SEG, GATE, NORM, EXACT, ATTN, HEAD, FIN, SOC = (K.segment_sum_cases(), K.gate_cases(), K.norm_cases(), K.exact_cases(), K.attn_cases(), K.head_cases(), K.finish_cases(),
                                                 K.soc_cases())


# ------------------------------------------------------------------------------------------------ coverage + twin == stand-in
@pytest.mark.parametrize("name", _ids(SEG))
def test_segment_sum(name):
    case = SEG[name]
    _cover(case)
    assert set(case["cover"]["degrees"]) >= {0, 1, 3, 4, 5}
    r = K.check_segment_sum(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["repeat"], r


def test_segment_sum_fp32_emulation_is_the_list_order_sum():
    """the emulation the kernel is compared with for equality differs from another order of the same sum on these inputs (else equality would prove nothing)"""
    msg, rowptr, perm, N = SEG["Dp260"]["args"]
    fwd = K.segment_sum_fp32(msg, rowptr, perm)
    rev = torch.zeros_like(fwd)
    for n in range(N):
        for q in reversed(range(int(rowptr[n]), int(rowptr[n + 1]))):
            rev[n] = rev[n] + msg[perm[q]]
    assert not torch.equal(fwd, rev)
    assert K.compare(fwd, *R.segment_sum(msg, rowptr, perm)) < 1e-6


@pytest.mark.parametrize("name", _ids(GATE))
def test_gate_and_backward(name):
    case = GATE[name]
    _cover(case)
    assert case["cover"]["act_ids"] == case["want_ids"], case["cover"]
    for backward in (False, True):
        r = K.check_gate(case, cpu_ops, "cpu", backward=backward)
        assert r["err"] < TIE and r["exact"] and r["repeat"], (backward, r)


def test_gate_cases_reach_every_row_count():
    rows = {GATE[n]["args"][0].shape[0] for n in GATE}
    assert rows >= {1, 3, 4, 5, 67, 8197}
    assert GATE["plain_rows5"]["cover"]["nact"] == 0


@pytest.mark.parametrize("name", _ids(NORM))
def test_norm_act_and_backward(name):
    case = NORM[name]
    _cover(case)
    for backward in (False, True):
        r = K.check_norm_act(case, cpu_ops, "cpu", backward=backward)
        assert r["err"] < TIE and r["exact"] and r["repeat"], (backward, r)


def test_norm_cases_reach_l4():
    assert max(NORM[n]["cover"]["lmax"] for n in NORM) == 4


@pytest.mark.parametrize("name", _ids(EXACT))
def test_exact_ops(name):
    case = EXACT[name]
    _cover(case)
    r = K.check_exact(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["exact"] and r["repeat"], r


@pytest.mark.parametrize("name", _ids(ATTN))
def test_attention(name):
    case = ATTN[name]
    _cover(case)
    assert set(case["cover"]["degrees"]) >= {0, 1, 3, 4, 5, 127, 128, 129, 257} and case["cover"]["dominant_logit_gap"] > 20.0, case["cover"]
    r = K.check_attn_logits(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["exact"] and r["repeat"], r
    r = K.check_attn_aggregate(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["exact"] and r["repeat"], r


def test_attention_tables_reach_the_head_counts():
    hs = {ATTN[n]["args"][8] for n in ATTN}
    assert {1, 8} <= hs and any(h < 8 for h in hs)


def test_attention_wrap_case():
    case = K.attn_wrap_case()
    _cover(case)
    r = K.check_attn_logits(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["exact"], r


@pytest.mark.parametrize("name", _ids(HEAD))
def test_ham_readout_and_two_launch_route(name):
    case = HEAD[name]
    _cover(case)
    for two in (False, True):
        r = K.check_ham_readout(case, cpu_ops, "cpu", two_launches=two)
        assert r["err"] < TIE and r["exact"] and r["repeat"], (two, r)


def test_head_cases_reach_every_register_slot_boundary():
    """c_width <= 256, <= 512, > 512; nao^2 likewise; Wigner floats <= 256 and > 256 (HR_CJ, HR_HJ, HR_WJ of the read-out kernel)"""
    cov = [HEAD[n]["cover"] for n in HEAD]
    assert {c["c_width_slot"] for c in cov} == {0, 1, 2} and {c["nao2_slot"] for c in cov} == {0, 1, 2} and {c["nWuse_slot"] for c in cov} == {0, 1}
    assert any(c["empty_csr_rows"] > 0 for c in cov)


def test_head_wrap_case():
    (case,) = K.head_cases(wrap=True).values()
    _cover(case)
    assert case["cover"]["npairs"] == 2560 + 3
    r = K.check_ham_readout(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["exact"], r


@pytest.mark.parametrize("name", _ids(FIN))
def test_ham_finish(name):
    case = FIN[name]
    _cover(case)
    r = K.check_ham_finish(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["repeat"], r


@pytest.mark.parametrize("name", _ids(SOC))
def test_block_mean_and_soc_assemble(name):
    case = SOC[name]
    _cover(case)
    r = K.check_soc(case, cpu_ops, "cpu")
    assert r["err"] < TIE and r["repeat"], r


# ------------------------------------------------------------------------------------------------ sharpness: a wrong twin must not pass
SHARP = {
    "segment_sum_drops_tail_edge": lambda: K.check_segment_sum(SEG["Dp260"], None, "cpu", defect="drop_tail_edge"),
    "softmax_over_first_128_edges": lambda: K.check_attn_aggregate(ATTN["Dp260_H2"], None, "cpu", defect="softmax_first_chunk"),
    "two_heads_exchanged_logits": lambda: K.check_attn_logits(ATTN["Dp260_H2"], None, "cpu", defect="swap_heads"),
    "two_heads_exchanged_H8": lambda: K.check_attn_logits(ATTN["Dp1028_H8_hand"], None, "cpu", defect="swap_heads"),
    "clamp_ignored": lambda: K.check_norm_act(NORM["mini_rows67"], None, "cpu", defect="no_clamp"),
    "gate_activation_wrong_id": lambda: K.check_gate(GATE["planner_rows67"], None, "cpu", defect="gate_act_wrong_id"),
    "gate_activation_wrong_id_hand": lambda: K.check_gate(GATE["hand_rows5"], None, "cpu", defect="gate_act_wrong_id"),
    "sign_ignored": lambda: K.check_ham_readout(HEAD["planner_sign_minus"], None, "cpu", defect="ignore_sign"),
    "partner_not_transposed": lambda: K.check_ham_readout(HEAD["planner_default"], None, "cpu", defect="no_transpose"),
    "partner_not_transposed_hand": lambda: K.check_ham_readout(HEAD["nao23_cw600_L5_default"], None, "cpu", defect="no_transpose"),
    "H0_on_the_wrong_side_of_the_mask": lambda: K.check_ham_readout(HEAD["planner_h0_after_mask"], None, "cpu", defect="h0_wrong_side"),
    "H0_on_the_wrong_side_finish": lambda: K.check_ham_finish(FIN["su2_wrap"], None, "cpu", defect="h0_wrong_side"),
    "zero_diag_ignored": lambda: K.check_soc(SOC["soc_zero_diag"], None, "cpu", defect="ignore_zero_diag"),
    "mean_over_the_wrong_shell": lambda: K.check_soc(SOC["block_mean_planner_nao19"], None, "cpu", defect="wrong_shell"),
}


@pytest.mark.parametrize("name", sorted(SHARP))
def test_wrong_twin_is_rejected(name):
    """a case for which a listed wrong twin still passes is too weak: its builder is changed, not this bound"""
    assert SHARP[name]()["err"] > K.TOL, name


def test_compare_is_per_row():
    """what rel() lets through and compare() does not: an error in a row whose values are small next to the tensor's largest"""
    ref = torch.tensor([[1000.0, 1.0], [1e-3, 2e-3]], dtype=torch.float64)
    out = ref.clone()
    out[1, 0] *= 1.01
    assert K.G.rel(out, ref) < K.TOL and K.compare(out, ref, ref.abs()) > 100 * K.TOL
    assert K.compare(torch.tensor([[0.0, 1e-30]]), torch.zeros(1, 2), torch.zeros(1, 2)) == float("inf")
    assert K.compare(torch.tensor([[float("nan"), 0.0]]), torch.zeros(1, 2), torch.ones(1, 2)) == float("inf")
    assert K.compare(torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(1, 2)) == 0.0
