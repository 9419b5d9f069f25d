"""Centre-only edge sources at model level: what HamGNNConvE3 marks, that the embeddings' rows have the marked zeros (HG_CHECK_STRUCT_ZEROS=1 asserts it inside
the forward, and trips when one is violated), and the backbone with the one-column programs against the same model without them -- on the CPU stand-ins here
(tests/cpu_ops.py: the planner's tables through the emulator), through the HIP kernels in the `-m gpu` cases."""
import pytest
import torch

from tests import centre_checks as C
from tests import cpu_ops
from tests import gpu_checks as G

SET_A = "64x0e+64x0o+32x1o+16x1e+12x2o+25x2e+18x3o+9x3e+4x4o+9x4e+4x5o+4x5e+2x6e"
SH_A = "0e+1o+2e+3o+4e+5o"           # the spherical harmonics set-A ships with (bench.SH): five marked irreps, l = 1 ... 5


@pytest.fixture
def cpu_backend(monkeypatch):
    cpu_ops.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    torch.set_num_threads(min(8, torch.get_num_threads()))


def _assert_same_rows(r, legacy):
    # (a reduced program deals other items to the waves than the program it is compared with: another order of the same fp32 sums, G.SAME_MATH_TOL -- the bound of
    #  test_gpu_parity.test_structural_zero_inputs_of_the_first_layer)
    for k in ("node_rel_err_vs_irrep", "edge_rel_err_vs_irrep", "node_rel_err_vs_complete", "edge_rel_err_vs_complete"):
        assert r[k] < G.SAME_MATH_TOL, (k, r)
    # (two layers; a legacy layer-0 pair block keeps the embedding's edge rows: the marked block is the one of layer 1)
    marked, other = ("last_pair_mfma_ratio", "first_pair_mfma_ratio") if legacy else ("first_pair_mfma_ratio", "last_pair_mfma_ratio")
    assert r["first_conv_mfma_ratio"] < 1.0 and r[marked] < 1.0 and r[other] == 1.0, r
    assert r["centre_sets"][0] and not any(r["centre_sets_switched_off"]), r


def test_what_the_backbone_marks():
    """the irreps of the spherical harmonics with l > 0, for the first ConvBlock and the first PairInteractionBlock that rewrites the edge rows; with
    legacy_edge_update the layer-0 pair block keeps the embedding's rows and the marks carry over to layer 1"""
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    cfg = dict(num_types=96, irreps_edge_sh=G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False, cutoff=26.0, rbf_func="bessel",
               num_radial=8, num_layers=3, irreps_node_features=G.MINI, use_kan=False, radial_MLP=[16, 16], correlation=2, num_hidden_features=4, use_corr_prod=False)
    want = C.first_layer_sets(G.MINI, G.SH)[2]
    assert want
    m = HamGNNConvE3(dict(cfg, legacy_edge_update=False))
    assert [b.conv_tp._centre for b in m.convolutions] == [want, (), ()] and [b.conv_tp._centre for b in m.pair_interactions] == [want, (), ()]
    m = HamGNNConvE3(dict(cfg, legacy_edge_update=True))
    assert [b.conv_tp._centre for b in m.convolutions] == [want, want, ()] and [b.conv_tp._centre for b in m.pair_interactions] == [(), want, ()]
    assert [b.conv_tp._zeros[1] for b in m.convolutions] == [C.first_layer_sets(G.MINI, G.SH)[1]] * 2 + [()]


@pytest.mark.parametrize("legacy", [False, True])
def test_centre_only_programs_on_the_cpu_stand_ins(cpu_backend, legacy):
    r = C.check_centre_zeros("cpu", legacy=legacy, n_atoms=4)
    _assert_same_rows(r, legacy)


def test_debug_hook_trips_on_a_planted_entry(cpu_backend, monkeypatch):
    """HG_CHECK_STRUCT_ZEROS=1 passes on the rows the embeddings produce and raises when an m != 0 entry of a marked irrep is not zero"""
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    cfg = dict(num_types=96, irreps_edge_sh=G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False, cutoff=26.0, rbf_func="bessel",
               num_radial=8, num_layers=1, irreps_node_features=G.MINI, use_kan=False, radial_MLP=[16, 16], correlation=2, num_hidden_features=4, use_corr_prod=False,
               legacy_edge_update=False)
    torch.manual_seed(2)
    m = HamGNNConvE3(cfg)
    g = S.random_cell(3, [14, 8], seed=2, density=0.004)
    monkeypatch.setenv("HG_CHECK_STRUCT_ZEROS", "1")
    with torch.no_grad():
        m(g)                                                   # the real embeddings: every marked entry is zero
    i = m._centre_edge_set()[0]
    l, o, mp = m.layout.irreps[i][1], m.layout.off[i], m.layout.mulp[i]
    real = m._embed

    def planted(data):
        z, topo, geo, node, f = real(data)
        f = f.clone()
        f[0, o + (l + 1) * mp] = 1e-3                          # component m = +1 of the first marked irrep
        return z, topo, geo, node, f
    monkeypatch.setattr(m, "_embed", planted)
    with pytest.raises(AssertionError, match="centre-only edge irrep violated"), torch.no_grad():
        m(g)
    monkeypatch.setenv("HG_CHECK_STRUCT_ZEROS", "0")
    with torch.no_grad():
        m(g)                                                   # (the hook is a debug switch: off, nothing is checked)


# ---------------------------------------------------------------------------------------------- through the HIP kernels

@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(legacy=True), dict(charge=True)], ids=["mini", "mini_legacy", "mini_charge_doping"])
def test_centre_only_programs_mini_irreps(kw):
    """mini irreps, 9 atoms (296 edges: a last tile of 8 edges), two layers: split launches"""
    r = C.check_centre_zeros(**kw)
    print(r)
    _assert_same_rows(r, kw.get("legacy", False))
    assert r["tail_edges"] > 0 and all(k == "is" and p != "1" for k, p, _ in r["launches"]), r


@pytest.mark.gpu
def test_centre_only_programs_set_a_split_launches():
    """set-A with 64-wide radial layers (the radial scale on the half-precision matrix pipe) on the 2-atom Si cell: 172 edges, one work group per output segment"""
    from hamgnn_amd.data import synthetic as S
    r = C.check_centre_zeros(irr=SET_A, sh=SH_A, radial=(64, 64), num_radial=64, graph=S.si_diamond(primitive=True))
    print(r)
    _assert_same_rows(r, False)
    assert r["E"] == 172 and len(r["centre_sets"][0]) == 5 and r["tail_edges"] > 0 and all(k == "is" and p != "1" for k, p, _ in r["launches"]), r


@pytest.mark.gpu
def test_centre_only_programs_set_a_single_part_fused_scatter():
    """set-A on a 60-atom a-SiO2 cell (4 904 edges, 307 tiles: single-part launches, the ConvBlocks with the fused node scatter): the centre-only epilogue
    under the segmented scan, a last tile of 8 edges, receivers whose runs cross tile boundaries"""
    from hamgnn_amd.data import synthetic as S
    r = C.check_centre_zeros(irr=SET_A, sh=SH_A, radial=(64, 64), num_radial=64, graph=S.amorphous_sio2(60, seed=1))
    print(r)
    _assert_same_rows(r, False)
    assert r["tail_edges"] > 0 and r["straddling_receivers"] > 0, r
    assert all(k == "is" and p == "1" for k, p, _ in r["launches"]) and any(red for _, _, red in r["launches"]), r
