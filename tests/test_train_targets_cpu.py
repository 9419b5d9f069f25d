"""Training on `overlap` and `band_gap` targets without a GPU: the host code end to end on the CPU stand-ins (tests/cpu_ops.py; the k-space adjoint takes its
torch path there), the numpy twin of hg_hk_assemble_adjoint against that torch path, and the row-wise metrics against autograd (pure torch)."""
import pytest
import torch

from tests import gpu_checks as G
from tests import train_targets_checks as T


@pytest.fixture
def cpu_backend(monkeypatch):
    from tests import cpu_ops
    cpu_ops.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    torch.set_num_threads(min(8, torch.get_num_threads()))


def test_new_entry_point_is_exported_and_wrapped():
    from hamgnn_amd import _lib, ops
    assert "hg_hk_assemble_adjoint" in _lib.EXPORTS and callable(ops.hk_assemble_adjoint)


# ---- the adjoint's numpy twin (the kernel's tables and loop structure) vs the torch path
@pytest.mark.parametrize("name,nk", [("one_atom", 1), ("one_atom", 5), ("coh", 1), ("coh", 5), ("batch2", 5), ("no_edges", 5)])
def test_adjoint_twin_matches_the_torch_path(name, nk):
    r = T.check_adjoint_twin(name, nk)
    assert r["g_on_rel_err"] < 1e-12 and r["g_off_rel_err"] < 1e-12, r


def test_adjoint_cases_have_the_structure_they_are_meant_to_test():
    case = T.adjoint_case("coh")
    ptr, order, pij, orank, ooff, M = T._tables(case)
    assert int((ptr[1:] - ptr[:-1]).max()) >= 2                                   # an atom pair with several images
    assert sorted(case[0].z.tolist()) == [1, 6, 8] and bool((orank < 0).any()) and bool((orank >= 0).all(1).any())     # H lacks orbitals, C / O have all 13
    one = T.adjoint_case("one_atom")
    pij1 = T._tables(one)[2]
    assert one[2] == 1 and one[4] > 0 and bool((pij1[:, 0] == pij1[:, 1]).all())  # every edge a self image
    b2 = T.adjoint_case("batch2")
    assert b2[1] > 0 and b2[3] > 0                                               # the second crystal: n0, e0 > 0
    assert T.adjoint_case("no_edges")[4] == 0 and T._tables(T.adjoint_case("no_edges"))[2].shape[0] == 0
    far = T.adjoint_case("far")
    assert float((far[5].double()[:, None, :] * far[0].nbr_shift.double()[None]).sum(-1).abs().max()) > 20.0


def test_adjoint_twin_turns_red_on_a_flipped_orank_entry():
    r = T.check_adjoint_twin("coh", 5, flip=True)
    assert max(r["g_on_rel_err"], r["g_off_rel_err"]) > 1e-3, r


# ---- metrics
@pytest.mark.parametrize("name", sorted(T.METRIC_FORMULAS))
def test_row_wise_metric_vs_autograd(name):
    r = T.check_metric(name)
    assert r["min_row_norm"] > 0 and r["min_diff_norm"] > 0, r                    # no row of zero norm (a condition on the inputs)
    assert r["loss_rel_err"] < 1e-12 and r["grad_rel_err"] < 1e-12, r


def test_sharded_loss_keeps_refusing_the_row_wise_metrics():
    from hamgnn_amd.training import _loss_and_grad_sharded
    with pytest.raises(ValueError, match="unsupported loss metric"):
        _loss_and_grad_sharded(torch.zeros(3, 4), torch.zeros(3, 4), "euclidean_loss", 1)


# ---- overlap
def test_overlap_loss_whole_model_on_cpu(cpu_backend):
    r = T.check_full_targets("cpu", "overlap")
    assert r["overlap_params"] > 0 and r["overlap_groups_trained"] == r["overlap_params"], r
    assert r["loss_rel_err"] < 1e-5 and r["max_rel_err"] < 2e-5, r


def test_plain_step_leaves_the_overlap_networks_at_zero_on_cpu(cpu_backend):
    r = T.check_full_targets("cpu", "plain")
    assert r["overlap_params"] > 0 and r["overlap_grad_max"] == 0.0, r
    assert r["loss_rel_err"] < 1e-5 and r["max_rel_err"] < 2e-5 and r["vs_ham_only_max_rel"] <= G.SAME_MATH_TOL, r


@pytest.mark.parametrize("basis", [None, "so3", "su2"])
def test_overlap_head_backward_on_cpu(cpu_backend, basis):
    r = T.check_head_backward_overlap("cpu", basis, n_atoms=3 if basis else 4)
    assert r["overlap_groups_trained"] >= 4, r
    assert all(v < G.TOL for k, v in r.items() if k.endswith("rel_err")), r


def test_head_training_step_with_overlap_networks_on_cpu(cpu_backend):
    r = T.check_head_training_step_overlap("cpu")
    assert r["all_set"] and r["overlap_grad_max"] == 0.0 and r["ham_grad_max"] > 0, r


# ---- band_gap
@pytest.mark.parametrize("zps", [False, True])
@pytest.mark.parametrize("kind", ["gap_bands", "gap"])
def test_band_gap_loss_whole_model_on_cpu(cpu_backend, kind, zps):
    r = T.check_full_targets("cpu", kind, zps=zps)
    assert r["gap_isolated"], r                                                   # condition on the inputs, on the fp64 reference alone
    assert r["eig_chains_in_backward"] == 1, r                                    # one eigen-chain per crystal and step for both k-space losses
    assert r["loss_rel_err"] < 1e-4 and r["max_rel_err"] < 2e-3, r


def test_band_gap_backward_alone_on_cpu(cpu_backend):
    r = T.check_band_gap_backward("cpu")
    assert r["gap_isolated"], r
    assert r["g_on_rel_err"] < 1e-4 and r["g_off_rel_err"] < 1e-4, r


@pytest.mark.parametrize("what,match", [("overlap_ham_only", "ham_only"), ("gap_no_bands", "band_gap"), ("gap_soc", "band_gap")])
def test_refusals_on_cpu(cpu_backend, what, match):
    with pytest.raises(ValueError, match=match):
        T.refusal("cpu", what)


def test_wavefunction_and_peak_stay_refused(cpu_backend):
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.training import training_step
    model = T._small_model()
    g = S.add_random_targets(S.random_cell(2, [6, 8, 1], seed=3, density=0.004), 13, seed=3)
    for pred in ("wavefunction", "peak"):
        with pytest.raises(ValueError, match="not built"):
            training_step(model, g, losses=[dict(metric="mae", prediction=pred)])


@pytest.mark.parametrize("shape", [(7,), (5, 4, 6)], ids=["1d", "3d"])
@pytest.mark.parametrize("name", sorted(T.METRIC_FORMULAS))
def test_row_wise_metric_axes_follow_the_reference(name, shape):
    """the reference's expressions verbatim (utils/losses.py:5-33: products / norms over dim=-1, sum_zero over dim=0 first) on a 1-D prediction
    (band_gap [n_crystals]) and a 3-D one; sum_zero beyond 2-D is not a scalar there and is refused"""
    from hamgnn_amd.training import _loss_and_grad
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(*shape, generator=gen, dtype=torch.float64).requires_grad_()
    t = torch.randn(*shape, generator=gen, dtype=torch.float64)
    if name == "sum_zero" and len(shape) > 2:
        with pytest.raises(ValueError, match="sum_zero"):
            _loss_and_grad(p.detach(), t, name)
        return
    want = {"cosine_similarity": lambda: torch.mean(1.0 - torch.sum(p * t, dim=-1) / (torch.norm(p, p=2, dim=-1) * torch.norm(t, p=2, dim=-1))),
            "euclidean_loss": lambda: torch.mean((p - t).pow(2).sum(dim=-1).sqrt()),
            "sum_zero": lambda: torch.sum(p, dim=0).pow(2).sum(dim=-1).sqrt()}[name]()
    want.backward()
    loss, grad = _loss_and_grad(p.detach(), t, name)
    assert abs(float(loss) - float(want.detach())) < 1e-12 * abs(float(want.detach())) and G.rel(grad, p.grad) < 1e-12
