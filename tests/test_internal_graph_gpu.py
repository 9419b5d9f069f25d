"""HamGNN_pre.build_internal_graph on the GPU: the periodic neighbour list of csrc/neighbour.hip (hg_neighbour_bin / _pairs / _decode) bit-equal to the host
statement of the same rule (synthetic.build_graph on the fp32-rounded numbers), both backbones with the switch on against the same weights with the switch off
on the host-built internal graph (no difference at all), against the fp64 oracle (gpu_checks.TOL), and one training step against autograd through the oracle
(the bound of the existing full-model gradient tests).  Crystals, references and the margin assertion: tests/internal_graph_checks.py."""
import pytest
import torch

from tests import gpu_checks as G
from tests import internal_graph_checks as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _assert_edge_list(r):
    assert r["E_internal"] == r["E_host"] > r["E_data"] > 0, r
    assert r["edge_index_equal"] and r["cell_shift_equal"] and r["nbr_shift_equal"], r
    assert r["match_reproduces_data"] and r["match_equals_host"], r


@pytest.mark.parametrize("name", ["si2", "skew5", "batch3"])
def test_edge_list_equals_host_build_graph(name):
    """si2: every neighbour an image, self images, two or more images per direction; skew5: skewed cell, three species; batch3: 1 + 2 + 5 atoms, cumulative
    offsets, a crystal with self images only"""
    r = IC.check_edge_list(name, "cuda")
    print(r)
    _assert_edge_list(r)
    if name in ("si2", "batch3"):
        assert r["self_images"] > 0 and r["max_image"] >= 2, r


def test_edge_list_with_wrap_around():
    """the smallest random cell at density 0.004 with three bins along every lattice vector: every centre visits bins across the cell boundary"""
    g, n, nb, rcut = IC.wrap_crystal()
    print({"n_atoms": n, "bins": nb.tolist(), "bin_width_at_least": rcut})
    assert nb.min() >= 3
    r = IC.check_edge_list("wrap", "cuda")
    print(r)
    _assert_edge_list(r)
    assert r["max_image"] == 1, r


def test_build_is_reproducible():
    from hamgnn_amd.internal_graph import build_internal_graph
    g = IC.crystal("batch3").to("cuda")
    a, b = build_internal_graph(g, "openmx", IC.SCALE), build_internal_graph(g, "openmx", IC.SCALE)
    assert all(torch.equal(a[k], b[k]) for k in ("edge_index", "cell_shift", "nbr_shift", "matching_edges"))


@pytest.mark.parametrize("transformer", [False, True], ids=["conv", "transformer"])
def test_model_switch_on_equals_switch_off_on_host_graph(transformer):
    r = IC.check_model_hip_vs_hip("cuda", transformer=transformer)
    print(r)
    assert r["E_internal"] > r["E_data"] and r["edge_rows"][0] == r["geometry_rows"] == r["edge_attr_rows"] == r["E_data"], r
    assert r["node_diff"] == 0.0 and r["edge_diff"] == 0.0 and r["H_diff"] == 0.0 and r["H_absmax"] > 0.0, r


def test_model_vs_oracle():
    r = IC.check_model_vs_oracle("cuda")
    print(r)
    assert r["node_rel_err"] < G.TOL and r["edge_rel_err"] < G.TOL and r["H_rel_err"] < G.TOL, r


@pytest.mark.parametrize("transformer", [False, True], ids=["conv", "transformer"])
def test_training_step_vs_autograd(transformer):
    """every parameter gradient of one training_step on the 5-atom crystal vs torch.autograd through the oracle chain in fp64; the bound of
    tests/test_gpu_parity.py::test_full_model_backward_vs_autograd"""
    r = IC.check_training("cuda", transformer=transformer)
    print(r)
    assert r["loss_rel_err"] < G.TOL and r["max_rel_err"] < G.TOL and r["n_params"] > 50, r


def test_cache_builds_once_and_rebuilds_after_inplace_change(monkeypatch):
    r = IC.check_cache("cuda", monkeypatch)
    assert r["once"] == (1, True) and r["after_inplace_change"] == (2, True) and r["other_scale"] == (3, True) and r["to_drops"] and r["shard_drops"], r


def test_errors_and_refusals():
    from hamgnn_amd.internal_graph import build_internal_graph
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.parallel import shard_graph
    g = IC.crystal("skew5")
    gd = g.to("cuda")
    with pytest.raises(ValueError, match="radius_scale"):
        build_internal_graph(gd, "openmx", 0.8)
    for drop in ("cell", "cell_shift"):
        with pytest.raises(ValueError, match=drop):
            build_internal_graph(type(gd)({k: v for k, v in gd.items() if k != drop}), "openmx", IC.SCALE)
    from hamgnn_amd.data import synthetic as S
    lone = S.random_cell(1, [1], seed=0, density=1e-6)          # one hydrogen in a 100 Bohr cell: no neighbour, no image in range
    with pytest.raises(ValueError, match="no edges"):
        build_internal_graph(lone.to("cuda"), "openmx", IC.SCALE)
    with pytest.raises(NotImplementedError, match="build_internal_graph"):
        HamGNNConvE3(IC.config(True, use_kan=True))
    _, _, on, _, _, gt, _ = IC.models("skew5")
    with pytest.raises(NotImplementedError, match="build_internal_graph"):
        on(shard_graph(gt, 0, 2).to("cuda"))
