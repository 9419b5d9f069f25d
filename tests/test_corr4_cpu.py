"""`correlation: 4` on the CPU: the planner's nu = 4 tables and their transposes against the fp64 oracle (oracle/mace_ref.py) and autograd through it, and
the product's host logic -- CorrProductBlock, a whole HamGNNConvE3 with use_corr_prod, a whole HamGNNTransformer -- on the table-exact stand-ins of
tests/cpu_ops_corr.py.  The `-m gpu` twins (tests/test_corr4_gpu.py) run the same checks through the HIP kernels of csrc/sym_contraction.hip.
Bounds: the table-level checks run in float64 on fp32 coefficients and keep the 1e-6 of the nu <= 3 table tests (tests/test_plan_emu.py); everything
that goes through the product's fp32 rows is held to G.TOL, as every parity test here.
Every comparison with the oracle plans the nu = 4 table without the reference's natural-parity filter, as the oracle enumerates it (`oracle_paths`,
tests/corr4_checks.oracle_enumeration); the default, filtered table is checked against the reference's own block (corr_product_block_nu4.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from hamgnn_amd import plan as P
from tests import corr4_checks as K
from tests import cpu_ops_corr
from tests import gpu_checks as G


@pytest.fixture
def cpu_backend(monkeypatch):
    cpu_ops_corr.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.delenv("HG_CORR_KERNEL", raising=False)
    torch.set_num_threads(min(8, torch.get_num_threads()))


@pytest.fixture
def oracle_paths():
    with K.oracle_enumeration():
        yield


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("irr", K.IRREPS)
def test_nu4_tables_vs_oracle_einsum_chain_and_autograd(oracle_paths, irr):
    """sparse entry lists (nu = 1 ... 4) x concatenated weights == the oracle's dense einsum chain; the tables transposed by component and by kappa give
    the gradients autograd finds through that chain, per element and per node"""
    from oracle import mace_ref as M
    nh, N = 4, 6
    blk = K.oracle_block(irr, nh)
    sc = blk.prod.symmetric_contractions
    cons = sc.contractions
    for p in sc.parameters():
        p.grad = None
    hid = P.corr_hidden_irreps(irr, nh)
    tab = P.sym_contraction_tables(hid, 4)
    assert all(tab[f"K{nu}"] == [c.U(nu).shape[-1] for c in cons] for nu in (1, 2, 3, 4))
    assert int(tab["ptr4"][-1]) == {K.IRREPS[0]: 32625, K.IRREPS[1]: 7888}[irr]            # the non-zero U_4 entries of these irreps
    for nu in (1, 2, 3, 4):
        tab.update({f"{k}{nu}": v for k, v in P.sym_contraction_adjoint_tables(tab, nu).items()})
    lay = P.PlanarLayout(hid)
    rng = np.random.default_rng(11)
    h = torch.from_numpy(rng.standard_normal((N, sum(m * (2 * l + 1) for m, l, _ in hid)))).requires_grad_()
    z = torch.from_numpy(rng.choice([0, K.NEL - 1], size=N))
    out = sc(M.reshape_irreps(blk.irreps_hidden, h), torch.nn.functional.one_hot(z, K.NEL).double())
    Gm = torch.from_numpy(rng.standard_normal(tuple(out.shape)))
    (out * Gm).sum().backward()
    by_nu = lambda c, nu: c.weights_max if nu == 4 else c.weights[3 - nu]
    W = {nu: torch.cat([by_nu(c, nu).detach() for c in cons], 1).numpy() for nu in (1, 2, 3, 4)}
    hp, gp = lay.to_planar(h.detach().numpy()), lay.to_planar(Gm.numpy())
    got = np.zeros((N, lay.dim))
    for nu in (1, 2, 3, 4):
        low = got
        got = cpu_ops_corr.contraction_nu_np(tab, nu, hp, z.numpy(), W[nu], nh, got)
    assert rel(lay.from_planar(got), out.detach().numpy()) < 1e-6
    assert rel(got, low) > 1e-3                                                           # the nu = 4 term is not negligible in this check
    g_h = np.zeros_like(hp)
    for nu in (1, 2, 3, 4):
        gh, gW = cpu_ops_corr.contraction_nu_backward_np(tab, nu, hp, z.numpy(), W[nu], nh, gp, False)
        g_h += gh
        assert rel(gW, torch.cat([by_nu(c, nu).grad for c in cons], 1).numpy()) < 1e-6, nu
        ghn, gWn = cpu_ops_corr.contraction_nu_backward_np(tab, nu, hp, np.arange(N), W[nu][z.numpy()], nh, gp, True)     # per-node weight blocks
        acc = np.zeros_like(gW)
        np.add.at(acc, z.numpy(), gWn)
        assert rel(ghn, gh) < 1e-12 and rel(acc, gW) < 1e-12, nu
    assert rel(lay.from_planar(g_h), h.grad.numpy()) < 1e-6


def test_tables_of_correlation_1_2_3_are_byte_identical_to_the_recorded_ones(golden_dir):
    """digests recorded before the planner learnt nu = 4 (tools/gen_sym_table_digests.py): the correlation <= 3 tables have not moved by a byte"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_sym_table_digests", os.path.join(os.path.dirname(os.path.dirname(golden_dir)), "tools", "gen_sym_table_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(golden_dir, "sym_contraction_table_digests.json")) as f:
        want = json.load(f)
    got = mod.compute()
    assert set(want) == set(got) and len(want) == 7
    assert got == want
    t3 = P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 3), 3)               # and correlation 4 only ADDS keys to what correlation 3 returns
    t4 = P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 3), 4)
    assert set(t4) - set(t3) == {"ptr4", "ent4", "K4"}
    assert mod.digest({k: t4[k] for k in t3}) == mod.digest(t3)


def test_entry_cap_raises_and_names_the_count(monkeypatch):
    from hamgnn_amd.plan import tables
    monkeypatch.setattr(tables, "SYM4_ENTRY_CAP", 5000)
    with pytest.raises(NotImplementedError, match=r"at least \d+ entries"):
        P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 3), 4)                 # 16 033 entries
    assert "ptr3" in P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 3), 3)    # the cap concerns nu = 4 alone
    monkeypatch.setattr(tables, "SYM4_ENTRY_CAP", 16033)
    assert int(P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 3), 4)["ptr4"][-1]) == 16033


def test_default_enumeration_is_the_references_filtered_one():
    """correlation 4 as the reference builds it (cg.py:99-114): natural-parity coupling results only -- the path counts of its weights_max (recorded in the
    fixture) -- and no block at all for a target of unnatural parity; without the filter, the oracle's counts"""
    f = G.load("corr_product_block_nu4")
    tab = P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 4), 4)
    assert tab["K4"] == [46, 76, 85] == [int(v) for v in f["meta"]["K4"]]
    assert [f["weights"][f"prod.symmetric_contractions.contractions.{k}.weights_max"].shape[1] for k in range(3)] == tab["K4"]
    with pytest.raises(NotImplementedError, match="unnatural parity"):
        P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[1], 4), 4)
    with K.oracle_enumeration():
        assert P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 4), 4)["K4"] == [55, 124, 148]


def test_filtered_tables_transposed_reproduce_autograd():
    """the default (filtered) nu = 4 table: its transposes against autograd through the dense tensor the table itself spells out"""
    irr, nh, N = "2x0e+2x1o", 2, 4
    hid = P.corr_hidden_irreps(irr, nh)
    tab = P.sym_contraction_tables(hid, 4)
    tab.update({f"{k}4": v for k, v in P.sym_contraction_adjoint_tables(tab, 4).items()})
    E, Kt, ne = int(tab["ptr4"][-1]), sum(tab["K4"]), tab["num_ell"]
    ent = tab["ent4"][:E]
    U = torch.zeros(tab["nout"], ne, ne, ne, ne, Kt, dtype=torch.float64)
    o = np.repeat(np.arange(tab["nout"]), np.diff(tab["ptr4"]))
    U.index_put_(tuple(torch.from_numpy(a.astype(np.int64)) for a in (o, ent[:, 0], ent[:, 1], ent[:, 2], ent[:, 3], ent[:, 4])),
                 torch.from_numpy(np.ascontiguousarray(ent[:, 5]).view(np.float32).astype(np.float64)), accumulate=True)
    lay = P.PlanarLayout(hid)
    gen = torch.Generator().manual_seed(8)
    hp = torch.randn(N, lay.dim, generator=gen, dtype=torch.float64).requires_grad_()
    W = torch.randn(3, Kt, nh, generator=gen, dtype=torch.float64).requires_grad_()
    z = torch.tensor([2, 0, 0, 2])
    cols = torch.from_numpy(tab["ell_off"].astype(np.int64))[:, None] + torch.arange(nh)[None, :]
    ocols = torch.from_numpy(tab["out_off"].astype(np.int64))[:, None] + torch.arange(nh)[None, :]
    x = hp[:, cols]                                                                       # [N, ell, c]
    out = torch.einsum("oabdek,nkc,nac,nbc,ndc,nec->noc", U, W[z], x, x, x, x)
    gp = torch.zeros(N, lay.dim, dtype=torch.float64)
    gp[:, ocols.reshape(-1)] = torch.randn(N, ocols.numel(), generator=gen, dtype=torch.float64)
    (out * gp[:, ocols]).sum().backward()
    gh, gW = cpu_ops_corr.contraction_nu_backward_np(tab, 4, hp.detach().numpy(), z.numpy(), W.detach().numpy(), nh, gp.numpy(), False)
    assert rel(gh[:, cols.reshape(-1).numpy()], hp.grad[:, cols.reshape(-1)].numpy()) < 1e-12 and rel(gW, W.grad.numpy()) < 1e-12


def test_correlation_5_keeps_raising():
    from hamgnn_amd import nn as hnn
    with pytest.raises(NotImplementedError, match="correlation 1, 2"):
        hnn.CorrProductBlock(K.IRREPS[0], 3, 5, 3, True)
    with pytest.raises(AssertionError):
        P.sym_contraction_tables(P.corr_hidden_irreps(K.IRREPS[0], 3), 5)
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    cfg = dict(num_types=4, irreps_edge_sh=G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False, cutoff=26.0,
               rbf_func="bessel", num_radial=8, num_layers=1, irreps_node_features=K.IRREPS[0], use_kan=False, radial_MLP=[16, 16], correlation=5,
               num_hidden_features=3, use_corr_prod=True)
    with pytest.raises(NotImplementedError, match="correlation 1, 2"):
        HamGNNConvE3(cfg)


@pytest.mark.parametrize("doped", [False, True], ids=["element_weights", "doped"])
@pytest.mark.parametrize("irr", K.IRREPS)
def test_block_forward_and_gradients_vs_oracle(cpu_backend, oracle_paths, irr, doped):
    r = K.check_block("cpu", irr, 3, 5, doped=doped)
    assert r["max_rel_err"] < G.TOL and r["n"] >= 18, r


def test_unknown_corr_kernel_value_raises(cpu_backend, oracle_paths, monkeypatch):
    monkeypatch.setenv("HG_CORR_KERNEL", "fast")
    with pytest.raises(ValueError):
        K.check_block("cpu", K.IRREPS[0], 3, 2)


@pytest.mark.parametrize("name", ["corr_product_block", "corr_product_block_nu3", "corr_product_block_nu1"])
def test_generic_route_matches_default_route(cpu_backend, monkeypatch, name):
    """HG_CORR_KERNEL=nu: every term on the order-generic entry points; against the default route, and against the reference's outputs"""
    r = K.check_generic_vs_default("cpu", name, monkeypatch)
    assert r["max_rel_err"] < G.SAME_MATH_TOL, r
    assert os.environ.get("HG_CORR_KERNEL") == "nu"
    assert G.check_corr_product("cpu", name)["corr_product_rel_err"] < G.TOL


def test_correlation_4_block_under_the_generic_route(cpu_backend, oracle_paths, monkeypatch):
    monkeypatch.setenv("HG_CORR_KERNEL", "nu")
    r = K.check_block("cpu", K.IRREPS[1], 3, 5, doped=True)
    assert r["max_rel_err"] < G.TOL, r


def test_reference_fixture_correlation_4(cpu_backend):
    """the reference's own CorrProductBlock(correlation=4) (tools/gen_golden_corr4.py): inputs, weights, outputs"""
    f = G.load("corr_product_block_nu4")
    assert int(f["meta"]["correlation"]) == 4 and not any("U_matrix" in k for k in f["weights"])
    assert G.check_corr_product("cpu", "corr_product_block_nu4")["corr_product_rel_err"] < G.TOL


@pytest.mark.parametrize("kw", [
    dict(irr="4x0e+3x1o+2x2e"),                                           # HamGNNConvE3 with use_corr_prod
    dict(irr="4x0e+3x1o+2x2e", charge=True, crystals=2),                 # ... with doped node attributes: per-node nu = 4 weight mixtures
    dict(irr="4x0e+2x1o+2x2e", transformer=True),                        # HamGNNTransformer (two heads: even multiplicities)
], ids=["conv_e3", "conv_e3_doped", "transformer"])
def test_whole_model_correlation_4_vs_oracle(cpu_backend, oracle_paths, kw):
    """forward (the loss) and every parameter gradient of a whole model with `correlation: 4` against the oracle and autograd through it"""
    r = G.check_full_backward(device="cpu", n_atoms=2, seed=6, corr=4, nao=13, num_layers=1, **kw)
    assert r["loss_rel_err"] < G.TOL and r["max_rel_err"] < G.TOL and r["n_params"] >= 60, r
