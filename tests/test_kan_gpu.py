"""use_kan on the GPU: hg_kan_hidden (csrc/kan.hip) alone against the fp64 restatement, the message blocks and the backbone against the reference's own
use_kan outputs (tests/golden/kan_*.npz, backbone_kan.npz) and against the oracle with its generators swapped for KANs.  Tolerance: the project's contract
gpu_checks.TOL (relative to the largest reference value) against fp64, everywhere."""
import pytest
import torch

from tests import gpu_checks as G
from tests import kan_checks as KC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("E", [1, 17, 65, 83])
@pytest.mark.parametrize("name", sorted(KC.KERNEL_SHAPES))
def test_kan_hidden_kernel_vs_fp64(name, E):
    """E: a single edge, the 16-edge tile tail, the work-group tails (plain path 16, MFMA path 128 edges per work group), several work groups"""
    r = KC.check_kan_kernel("cuda", name, E)
    assert r["packed"] == name.endswith("mfma"), r
    if E == 83:
        assert r["min_region_count"] > 0, r                    # every region of every layer's knots is hit (a condition on the inputs, met by the fp64 reference alone)
    assert r["phi_rel_err"] < G.TOL and r["out_rel_err"] < G.TOL, r
    assert r["pad_contribution"] == 0.0, r


@pytest.mark.parametrize("E", [293, 2048 * 128 + 77], ids=["three_work_groups", "persistent_loop"])
def test_kan_hidden_mfma_path_beyond_one_work_group(E):
    """the MFMA path takes 128 edges per work group and at most 2048 work groups per generator: several work groups with a tail, and a launch whose waves
    go round the persistent loop (rows are independent: the fp64 reference is taken on the first rows, the rows around the wrap and the tail)"""
    from hamgnn_amd import ops, plan as P
    from tests import kan_ref as K
    refs = KC.make_generators("three_generators_mfma")
    gens = [ops.KanGenerator(P.kan_layers({"g." + n: v for n, v in K.state_dict_np(k).items()}, "g"), "cuda") for k in refs]
    rbf = 1.5 * torch.randn(E, 64, generator=torch.Generator().manual_seed(3))
    Phi = ops.kan_hidden_multi(rbf.cuda().contiguous(), gens)
    torch.cuda.synchronize()
    wrap = 2048 * 128
    idx = torch.unique(torch.cat([torch.arange(0, 40), torch.arange(wrap - 40, wrap + 40), torch.arange(E - 90, E)]).clamp(0, E - 1))
    for m, k in enumerate(refs):
        assert G.rel(Phi[m][idx.cuda()], k.features(rbf[idx].double())) < G.TOL, m


def test_kan_hidden_kernel_rejects_what_it_does_not_run():
    from hamgnn_amd import ops, plan as P
    from tests import kan_ref as K
    gen = ops.KanGenerator(P.kan_layers({"g." + n: v for n, v in K.state_dict_np(K.KANRef((8, 16, 16, 4))).items()}, "g"), "cuda")
    rbf = torch.zeros(5, 8, device="cuda")
    gen.packed = True                                          # fragment order claimed for a shape of the plain path
    with pytest.raises(RuntimeError, match="packed"):
        ops.kan_hidden(rbf, gen)


@pytest.mark.parametrize("schedule", ["seg", "is"])
def test_message_pack_block_golden_kan(schedule):
    r = KC.check_message_pack_kan("cuda", lite=False, schedule=schedule)
    assert r["hidden"] == 7 * 16 and r["message_pack_rel_err"] < G.TOL, r


def test_message_pack_block_lite_golden_kan():
    r = KC.check_message_pack_kan("cuda", lite=True)
    assert r["hidden"] == 7 * 16 and r["message_pack_rel_err"] < G.TOL, r


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_message_pack_random_irreps_vs_swapped_oracle_kan(seed):
    r = KC.check_message_pack_random_kan("cuda", seed=seed)
    assert r["hidden"] == 7 * 16 and r["rel_err"] < G.TOL, r


def test_message_pack_large_graph_launch_kan_64_64():
    """radial_MLP (64, 64) from 64 radial functions: the MFMA path of hg_kan_hidden, 448 hidden rows on the all-fp32 radial scale of the single-part launch"""
    r = KC.check_message_pack_random_kan("cuda", seed=1, radial=(64, 64), num_radial=64, parts=1)
    assert r["hidden"] == 448 and r["kernel"] == "is" and r["parts"] == 1 and r["rel_err"] < G.TOL, r


def test_backbone_golden_kan():
    r = KC.check_backbone_kan("cuda")
    assert r["generators"] == 9 and r["backbone_node_rel_err"] < G.TOL and r["backbone_edge_rel_err"] < G.TOL, r


def test_full_forward_vs_oracle_kan():
    r = KC.check_full_forward_kan("cuda", n_atoms=6, seed=0)
    assert r["node_rel_err"] < G.TOL and r["edge_rel_err"] < G.TOL and r["H_rel_err"] < G.TOL, r


def test_kan_backbone_forward_is_bit_reproducible():
    m, f = KC.kan_backbone_from_fixture()
    g = G.to_graph(f["graph"], "cuda")
    a, b = m(g), m(g)
    torch.cuda.synchronize()
    for k in ("node_attr", "edge_attr"):
        assert a[k].abs().max().item() > 0 and (a[k] - b[k]).abs().max().item() == 0.0, k


def test_refusals_name_use_kan_gpu():
    from hamgnn_amd import training
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_transformer import HamGNNTransformer
    from hamgnn_amd.models.model import Model
    with pytest.raises(NotImplementedError, match="use_kan"):
        HamGNNTransformer(KC.kan_config(num_heads=4))
    with pytest.raises(NotImplementedError, match="use_kan"):
        HamGNNConvE3(KC.kan_config(radial=(8, 16, 8, 16)))
    hip, head, g, *_ = KC.kan_model_and_graph("cuda", n_atoms=3, seed=1)
    with pytest.raises(NotImplementedError, match="use_kan"):
        training.training_step(Model(hip, head), g)
    rep = hip(g)
    with pytest.raises(NotImplementedError, match="use_kan"):
        hip.backward(g, rep, rep["_node_planar"], rep["_edge_planar_rot"])
