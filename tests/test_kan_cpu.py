"""use_kan (B-spline KAN weight generators) without a GPU: state-dict names, the W3' / blob packing against the fp64 restatement, the host logic end to end
on the CPU stand-ins (tests/cpu_ops.py + tests/kan_checks.kan_hidden_multi_cpu, which reads the packed blob the HIP kernel reads), and that the non-KAN
builders still emit what the parent's code path emits."""
import math

import numpy as np
import pytest
import torch

from tests import gpu_checks as G
from tests import kan_checks as KC
from tests import kan_ref as K


@pytest.fixture
def cpu_backend(monkeypatch):
    KC.install_cpu(monkeypatch)
    torch.set_num_threads(min(8, torch.get_num_threads()))


def test_state_dict_names_round_trip_a_reference_named_dict():
    """every parameter and every `grid` buffer of the reference's use_kan modules (names and shapes as in the fixtures the reference wrote) is taken and given back"""
    from hamgnn_amd import nn as hnn
    for lite, name in ((False, "kan_message_pack_block"), (True, "kan_message_pack_block_lite")):
        w = G.load(name)["weights"]
        m = hnn.MessagePackBlock(G.MINI, G.MINI, G.SH, G.MINI, 8, [16, 16], lite_mode=lite, use_kan=True)
        res = m.load_state_dict({k: torch.as_tensor(v) for k, v in w.items()}, strict=False)
        assert not res.missing_keys and not [k for k in res.unexpected_keys if "weight_generator" in k]      # (the reference's `.tp.weight` aliases are not slots here)
        sd = m.state_dict()
        gens = [k for k in sd if "weight_generator" in k]
        assert gens and all(k.split(".")[-1] in ("grid", "base_weight", "spline_weight", "spline_scaler") and ".layers." in k for k in gens)
        assert sum(k.endswith(".grid") for k in gens) == 3 * (1 if lite else 2)
        assert sum("weight_generator" in k for k in w) == len(gens)
        for k, v in sd.items():
            assert np.array_equal(v.double().numpy(), np.asarray(w[k], dtype=np.float32).astype(np.float64)), k
    m, f = KC.kan_backbone_from_fixture()
    sd = m.state_dict()
    kan = [k for k in sd if ".layers." in k]
    assert len({k.rsplit(".layers.", 1)[0] for k in kan}) == 9                                           # embedding + 2 x (2 + 2) generators
    assert set(kan) == {k for k in f["weights"] if "weight_generator" in k}                              # all covered, nothing of the reference's left over


@pytest.mark.parametrize("hs, gs", [((8, 16, 16, 156), 3), ((8, 12, 20, 40), 3), ((8, 16, 24), 3), ((64, 64, 64, 30), 3), ((8, 16, 16, 24), 5)],
                         ids=["8-16-16", "padded_12_20", "one_hidden", "64-64-64", "grid5"])
def test_w3_packing_matches_the_fp64_generator(hs, gs):
    """Phi_fp64 W3' == the fp64 generator output (1e-12), padded widths included: the rows of W3' follow the feature order of Phi, padded channels are zero rows"""
    from hamgnn_amd import plan as P
    k = K.KANRef(hs, gs, generator=torch.Generator().manual_seed(1)).scale_(6.0)
    sd = {"weight_generator." + n: v for n, v in K.state_dict_np(k).items()}
    assert P.is_kan(sd, "weight_generator") and not P.is_kan(sd, "weight_generator_combine")
    W3, H = P.kan_last_layer(sd, "weight_generator")
    hp = (hs[-2] + 15) // 16 * 16
    assert H == (gs + 4) * hp == W3.shape[0] and W3.shape[1] == hs[-1]
    x = 1.5 * torch.randn(83, hs[0], generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    assert G.rel(k.features(x) @ torch.from_numpy(W3), k(x)) < 1e-12
    pad = np.ones((gs + 4, hp), bool)
    pad[:, :hs[-2]] = False
    assert not W3[pad.reshape(-1)].any()
    w3s, Hs = P.message_pack._w3_scaled(sd, "weight_generator")          # the builders' seam: no 1 / sqrt(H) on a KAN
    assert Hs == H and np.array_equal(w3s, W3)


@pytest.mark.parametrize("name", sorted(KC.KERNEL_SHAPES))
def test_packed_blob_on_the_stand_in(name, cpu_backend):
    """the blob hg_kan_hidden reads (knot tables, W' plain and in fragment order) evaluated by the stand-in == the fp64 features; the inputs cover every region"""
    r = KC.check_kan_kernel("cpu", name, 83)
    assert r["packed"] == name.endswith("mfma")
    assert r["min_region_count"] > 0, r
    assert r["phi_rel_err"] < G.TOL and r["out_rel_err"] < G.TOL and r["pad_contribution"] == 0.0, r


@pytest.mark.parametrize("lite", [False, True], ids=["full", "lite"])
def test_message_pack_block_golden_kan_cpu(lite, cpu_backend):
    r = KC.check_message_pack_kan("cpu", lite=lite)
    assert r["hidden"] == 7 * 16 and r["message_pack_rel_err"] < G.TOL, r


def test_backbone_golden_kan_cpu(cpu_backend):
    r = KC.check_backbone_kan("cpu")
    assert r["generators"] == 9 and r["backbone_node_rel_err"] < G.TOL and r["backbone_edge_rel_err"] < G.TOL, r


def test_full_forward_vs_oracle_kan_cpu(cpu_backend):
    r = KC.check_full_forward_kan("cpu", n_atoms=4, seed=3)
    assert r["node_rel_err"] < G.TOL and r["edge_rel_err"] < G.TOL and r["H_rel_err"] < G.TOL, r


def test_refusals_name_use_kan(cpu_backend):
    from hamgnn_amd import training
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    from hamgnn_amd.models.hamgnn_transformer import HamGNNTransformer
    from hamgnn_amd.models.model import Model
    with pytest.raises(NotImplementedError, match="use_kan"):
        HamGNNTransformer(KC.kan_config(num_heads=4))
    with pytest.raises(NotImplementedError, match="use_kan"):
        HamGNNConvE3(KC.kan_config(radial=(8, 16, 8, 16)))
    with pytest.raises(NotImplementedError, match="build_internal_graph"):
        HamGNNConvE3(KC.kan_config(build_internal_graph=True))
    hip, head, g, *_ = KC.kan_model_and_graph("cpu", n_atoms=3, seed=1)
    with pytest.raises(NotImplementedError, match="use_kan"):
        training.training_step(Model(hip, head), g)
    with pytest.raises(NotImplementedError, match="use_kan"):
        hip(g, save_for_backward=True)
    rep = hip(g)
    with pytest.raises(NotImplementedError, match="use_kan"):
        hip.backward(g, rep, rep["_node_planar"], rep["_edge_planar_rot"])
    blk = hip.convolutions[0].conv_tp
    with pytest.raises(NotImplementedError, match="use_kan"):
        blk.backward_data(rep["_edge_planar_rot"], rep["_geometry"], True)
    with pytest.raises(NotImplementedError, match="use_kan"):
        hip.pair_embedding.backward(g.z, rep["_geometry"], rep["_edge_planar_rot"])


def _parent_w3(sd, prefix):
    """the parent's code path of the seam, restated: the last FullyConnectedNet layer divided by sqrt(H)"""
    ks = sorted(k for k in sd if k.startswith(prefix + ".layer") and k.endswith(".weight"))
    w3 = np.asarray(sd[ks[-1]], dtype=np.float64)
    return w3 / math.sqrt(w3.shape[0]), w3.shape[0]


def test_non_kan_programs_are_byte_identical_to_the_parent_code_path(monkeypatch):
    """use_kan=False: the tables and weight blobs of the MessagePackBlock (both modes) and embedding programs, built through the new seam, equal the ones built
    with the parent's `w3 / sqrt(H)` in its place"""
    from hamgnn_amd import plan as P
    from hamgnn_amd.plan import message_pack as MP
    f, fl, fb = G.load("message_pack_block"), G.load("message_pack_block_lite"), G.load("backbone")
    emb = {k[len("pair_embedding.conv_tp."):]: v for k, v in fb["weights"].items() if k.startswith("pair_embedding.conv_tp.")}
    build = lambda: [P.build_message_pack_program(f["weights"], G.MINI, G.MINI, G.SH, G.MINI, True),
                     P.build_message_pack_program(f["weights"], G.MINI, G.MINI, G.SH, G.MINI, False, merge_groups=P.choose_merge_groups(G.MINI, G.MINI, G.SH, G.MINI, 16)),
                     P.build_message_pack_program_lite(fl["weights"], G.MINI, G.MINI, G.SH, G.MINI, True),
                     P.build_message_pack_program_lite(fl["weights"], G.MINI, G.MINI, G.SH, G.MINI, False, fold=True),
                     P.build_embedding_program(emb, 20, G.SH, G.MINI)]
    new = build()
    monkeypatch.setattr(MP, "_w3_scaled", _parent_w3)
    old = build()
    for a, b in zip(new, old):
        assert a.hidden == b.hidden == 16
        for t in ("weights", "seg_table", "item_table"):
            x, y = getattr(a, t), getattr(b, t)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), t
