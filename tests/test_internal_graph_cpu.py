"""HamGNN_pre.build_internal_graph without a GPU: the host logic of hamgnn_amd/internal_graph.py and of the backbones (cache, matching, restriction to the
data's edges, backward, errors, refusals) on the CPU stand-ins of tests/cpu_ops.py + the numpy twin of the neighbour-list kernels
(tests/internal_graph_checks.py, which follows their binning and loop structure).  The kernels themselves: tests/test_internal_graph_gpu.py."""
import pytest
import torch

from tests import gpu_checks as G
from tests import internal_graph_checks as IC


@pytest.fixture
def cpu_backend(monkeypatch):
    IC.install_cpu(monkeypatch)
    torch.set_num_threads(min(8, torch.get_num_threads()))


def _assert_edge_list(r):
    assert r["E_internal"] == r["E_host"] > r["E_data"] > 0, r
    assert r["edge_index_equal"] and r["cell_shift_equal"] and r["nbr_shift_equal"], r
    assert r["match_reproduces_data"] and r["match_equals_host"], r


@pytest.mark.parametrize("name", ["si2", "skew5", "batch3"])
def test_twin_edge_list_equals_host_build_graph(cpu_backend, name):
    r = IC.check_edge_list(name, "cpu")
    print(r)
    _assert_edge_list(r)
    if name in ("si2", "batch3"):
        assert r["self_images"] > 0 and r["max_image"] >= 2, r


def test_twin_edge_list_with_wrap_around(cpu_backend):
    g, n, nb, rcut = IC.wrap_crystal()
    print({"n_atoms": n, "bins": nb.tolist(), "bin_width_at_least": rcut})
    assert nb.min() >= 3
    _assert_edge_list(IC.check_edge_list("wrap", "cpu"))


def test_radii_table_scale_and_default():
    from hamgnn_amd.basis import atomic_radii
    from hamgnn_amd.internal_graph import DEFAULT_RADIUS, SYMBOLS, radius_table
    tab, src = radius_table("openmx", 1.5), atomic_radii("openmx")
    assert tab.dtype == torch.float64 and float(tab[14]) == 1.5 * src["Si"] and float(tab[8]) == 1.5 * src["O"]
    missing = [z for z, s in enumerate(SYMBOLS) if s not in src]
    assert missing and all(float(tab[z]) == 1.5 * DEFAULT_RADIUS for z in missing)


def test_config_rule():
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_transformer import HamGNNTransformer
    m = HamGNNConvE3(IC.config(True))
    assert m.build_internal_graph and m.radius_scale == IC.SCALE and m.radius_type == "openmx"
    cfg = IC.config(True)
    del cfg["radius_scale"]
    assert HamGNNConvE3(cfg).radius_scale == 1.0                # hamgnn_conv.py:90-91
    with pytest.raises(ValueError, match="radius_scale"):
        HamGNNConvE3(IC.config(True, radius_scale=1.0))         # :93
    with pytest.raises(ValueError, match="radius_scale"):
        HamGNNTransformer(IC.config(True, transformer=True, radius_scale=0.9))
    assert not HamGNNConvE3(IC.config(False, radius_scale=0.5)).build_internal_graph      # switch off: whatever the config carries still constructs
    assert HamGNNTransformer(IC.config(True, transformer=True)).build_internal_graph


def test_cache_builds_once_and_rebuilds_after_inplace_change(cpu_backend, monkeypatch):
    r = IC.check_cache("cpu", monkeypatch)
    assert r["once"] == (1, True) and r["after_inplace_change"] == (2, True) and r["other_scale"] == (3, True) and r["to_drops"] and r["shard_drops"], r


def test_value_errors(cpu_backend):
    from hamgnn_amd.internal_graph import build_internal_graph
    from hamgnn_amd.data import synthetic as S
    g = IC.crystal("skew5")
    with pytest.raises(ValueError, match="radius_scale"):       # a data edge without a match: the reference asserts "Please increase radius_scale factor!"
        build_internal_graph(g, "openmx", 0.8)
    for drop in ("cell", "cell_shift"):
        with pytest.raises(ValueError, match=drop):
            build_internal_graph(type(g)({k: v for k, v in g.items() if k != drop}), "openmx", IC.SCALE)
    lone = S.random_cell(1, [1], seed=0, density=1e-6)          # one hydrogen in a 100 Bohr cell: no neighbour, no image in range
    assert lone.num_edges == 0
    with pytest.raises(ValueError, match="no edges"):
        build_internal_graph(lone, "openmx", IC.SCALE)


def test_refusals_name_build_internal_graph(cpu_backend):
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.parallel import shard_graph
    with pytest.raises(NotImplementedError, match="build_internal_graph"):
        HamGNNConvE3(IC.config(True, use_kan=True))
    _, _, on, _, _, g, _ = IC.models("skew5")
    with pytest.raises(NotImplementedError, match="build_internal_graph"):
        on(shard_graph(g, 0, 2))


def test_model_switch_on_equals_switch_off_on_host_graph_cpu(cpu_backend):
    r = IC.check_model_hip_vs_hip("cpu", name="si2")
    print(r)
    assert r["E_internal"] > r["E_data"] and r["edge_rows"][0] == r["geometry_rows"] == r["edge_attr_rows"] == r["E_data"], r
    assert r["node_diff"] == 0.0 and r["edge_diff"] == 0.0 and r["H_diff"] == 0.0 and r["H_absmax"] > 0.0, r


def test_model_vs_oracle_cpu(cpu_backend):
    r = IC.check_model_vs_oracle("cpu", name="si2")
    print(r)
    assert r["node_rel_err"] < G.TOL and r["edge_rel_err"] < G.TOL and r["H_rel_err"] < G.TOL, r


@pytest.mark.parametrize("transformer", [False, True], ids=["conv", "transformer"])
def test_training_step_vs_autograd_cpu(cpu_backend, transformer):
    """(the 2-atom cell: the stand-ins are slow; the 5-atom crystal of the issue runs on the GPU)"""
    r = IC.check_training("cpu", name="si2", transformer=transformer)
    print(r)
    assert r["loss_rel_err"] < G.TOL and r["max_rel_err"] < G.TOL and r["n_params"] > 50, r
