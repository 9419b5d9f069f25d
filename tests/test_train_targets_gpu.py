"""Training on `overlap` and `band_gap` targets on the GPU: hg_hk_assemble_adjoint (csrc/kspace.hip) alone against the fp64 torch adjoint, the head's backward
with ham_only=False and whole-model steps with `overlap` / `band_gap` / row-wise-metric losses against torch.autograd through the fp64 oracle.  Tolerances: the
project's contract gpu_checks.TOL against fp64; the bars of the existing band-energy tests for everything behind the complex64 eigensolver."""
import pytest
import torch

from tests import gpu_checks as G
from tests import train_targets_checks as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- the kernel alone
@pytest.mark.parametrize("name,nk", [("one_atom", 1), ("one_atom", 5), ("coh", 1), ("coh", 5), ("batch2", 5), ("far", 5), ("no_edges", 5)])
def test_hk_adjoint_kernel_vs_fp64(name, nk):
    r = T.check_adjoint_kernel("cuda", name, nk)
    print(r)
    if name == "one_atom":
        assert r["n"] == 1 and r["self_pairs"] == r["npairs"] > 0, r              # every edge a self image
    if name in ("coh", "far"):
        assert r["max_edges_per_pair"] >= 2 and r["absent_on"] > 0 and r["absent_off"] > 0, r      # several images of one pair; H lacks orbitals
    if name == "batch2":
        assert r["n0"] > 0 and r["e0"] > 0, r
    if name == "far":
        assert r["max_turns"] > 20.0, r
    if name == "no_edges":
        assert r["npairs"] == 0 and r["e"] == 0, r
    assert r["g_on_rel_err"] < G.TOL and r["g_off_rel_err"] < G.TOL, r
    assert r["absent_on_max"] == 0.0 and r["absent_off_max"] == 0.0, r
    assert r["relaunch_max_diff"] == 0.0 and r["entry_max_diff"] == 0.0, r        # fixed order, no atomics: two launches are bit-identical
    assert r["torch_path_on_rel"] < G.SAME_MATH_TOL and r["torch_path_off_rel"] < G.SAME_MATH_TOL, r     # HG_HK_ADJOINT=torch on the device


def test_hk_adjoint_identity_hip_vs_hip():
    r = T.check_adjoint_identity("cuda", "coh", 5)
    print(r)
    assert r["bound"] > 0 and r["diff"] <= r["bound"], r


def test_hk_adjoint_refuses_more_k_points_than_the_forward():
    from hamgnn_amd import ops
    case = T.adjoint_case("one_atom", 1)
    g, n0, n, e0, e, kv, nao, orank_all = case
    ptr, order, pij, orank, ooff, M = (t.cuda() if torch.is_tensor(t) else t for t in T._tables(case))
    nk = 65536
    Gd = torch.zeros(nk, M, M, dtype=torch.complex64, device="cuda")
    with pytest.raises(RuntimeError, match="hg_hk_assemble_adjoint"):
        ops.hk_assemble_adjoint(Gd, g.nbr_shift.cuda().float(), torch.zeros(nk, 3, device="cuda"), ptr, order, pij, n, e, nao, orank, ooff, M)


# ---- overlap
@pytest.mark.parametrize("basis", [None, "so3", "su2"], ids=["non_soc", "soc_so3", "soc_su2_abacus_13"])
def test_overlap_head_backward_vs_autograd(basis):
    r = T.check_head_backward_overlap("cuda", basis, n_atoms=6)
    print(r)
    assert r["overlap_groups_trained"] >= 4, r
    assert all(v < G.TOL for k, v in r.items() if k.endswith("rel_err")), r


def test_full_model_overlap_loss_vs_autograd():
    r = T.check_full_targets("cuda", "overlap")
    print(r)
    assert r["overlap_params"] > 0 and r["overlap_groups_trained"] == r["overlap_params"], r
    assert r["loss_rel_err"] < 1e-5 and r["max_rel_err"] < 2e-5, r


def test_full_model_plain_step_leaves_overlap_networks_at_zero():
    r = T.check_full_targets("cuda", "plain")
    print(r)
    assert r["overlap_params"] > 0 and r["overlap_grad_max"] == 0.0, r
    assert r["loss_rel_err"] < 1e-5 and r["max_rel_err"] < 2e-5 and r["vs_ham_only_max_rel"] <= G.SAME_MATH_TOL, r


def test_head_training_step_with_overlap_networks():
    r = T.check_head_training_step_overlap("cuda")
    assert r["all_set"] and r["overlap_grad_max"] == 0.0 and r["ham_grad_max"] > 0, r


# ---- band_gap
def test_band_gap_backward_vs_autograd():
    r = T.check_band_gap_backward("cuda")
    print(r)
    assert r["gap_isolated"], r
    assert r["g_on_rel_err"] < 1e-4 and r["g_off_rel_err"] < 1e-4, r              # the bar of test_band_energy_loss_backward (complex64 solver chain)


@pytest.mark.parametrize("zps", [False, True])
@pytest.mark.parametrize("kind", ["gap_bands", "gap"])
def test_full_model_band_gap_loss_vs_autograd(kind, zps):
    r = T.check_full_targets("cuda", kind, zps=zps)
    print(r)
    assert r["gap_isolated"], r                                                   # condition on the inputs, on the fp64 reference alone
    assert r["eig_chains_in_backward"] == 1, r
    assert r["loss_rel_err"] < 1e-4 and r["max_rel_err"] < 2e-3, r                # the bars of test_band_energy_loss_with_zero_point_shift


@pytest.mark.parametrize("what,match", [("overlap_ham_only", "ham_only"), ("gap_no_bands", "band_gap"), ("gap_soc", "band_gap")])
def test_target_refusals(what, match):
    with pytest.raises(ValueError, match=match):
        T.refusal("cuda", what)


# ---- metrics
def test_full_model_euclidean_loss_vs_autograd():
    r = T.check_full_targets("cuda", "euclid")
    print(r)
    assert r["loss_rel_err"] < G.TOL and r["max_rel_err"] < G.TOL, r
