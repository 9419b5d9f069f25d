"""-m gpu: `correlation: 4` through the order-generic HIP kernels of csrc/sym_contraction.hip (hg_sym_contraction_nu / hg_sym_contraction_nu_backward)
against the fp64 oracle and torch.autograd through it -- tolerance G.TOL (1e-5 relative, max-norm), the bound of every parity test here and of the
nu = 3 backward tests -- plus bit-reproducibility of two launches, the opt-in HG_CORR_KERNEL=nu route against the default kernels (two evaluation orders
of the same fp32 sums: G.SAME_MATH_TOL) and the reference's own correlation-4 block.  The CPU twins: tests/test_corr4_cpu.py.
Shapes: both small irreps (9 / 8 coupling components); N = 1, 5, 67 (one node; fewer nodes than elements' runs; three runs of 32 nodes per element walk);
3 hidden channels (a channel tail: 27 / 24 items split over 8 lanes each) and 16 (144 / 128 items: no split / split in two); element 1 has no node."""
import os

import pytest
import torch

from tests import corr4_checks as K
from tests import gpu_checks as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    monkeypatch.delenv("HG_CORR_KERNEL", raising=False)


@pytest.fixture
def oracle_paths():
    with K.oracle_enumeration():
        yield


@pytest.mark.parametrize("doped", [False, True], ids=["element_weights", "doped"])
@pytest.mark.parametrize("nh", [3, 16])
@pytest.mark.parametrize("N", [1, 5, 67])
@pytest.mark.parametrize("irr", K.IRREPS)
def test_corr4_block_forward_and_gradients_vs_oracle(oracle_paths, irr, N, nh, doped):
    """block forward, the gradient of the node rows and EVERY parameter gradient (doped: the gradient of the attributes too) against the oracle"""
    r = K.check_block("cuda", irr, nh, N, doped=doped)
    print(r)
    assert r["max_rel_err"] < G.TOL and r["n"] >= 18, r


@pytest.mark.parametrize("doped", [False, True], ids=["element_weights", "doped"])
def test_corr4_two_launches_are_bit_equal(oracle_paths, doped):
    assert K.check_two_launches("cuda", K.IRREPS[0], 16, 67, doped) == 0.0
    assert K.check_two_launches("cuda", K.IRREPS[1], 3, 67, doped) == 0.0


@pytest.mark.parametrize("name", ["corr_product_block", "corr_product_block_nu3", "corr_product_block_nu1"])
def test_corr_generic_route_matches_default_kernels(monkeypatch, name):
    """HG_CORR_KERNEL=nu at correlation 2, 3 and 1: forward and every gradient against the default kernels; the reference fixtures pass under the switch"""
    r = K.check_generic_vs_default("cuda", name, monkeypatch)
    print(r)
    assert r["max_rel_err"] < G.SAME_MATH_TOL, r
    assert os.environ.get("HG_CORR_KERNEL") == "nu"
    assert G.check_corr_product(name=name)["corr_product_rel_err"] < G.TOL


def test_corr4_block_on_the_generic_route_vs_oracle(oracle_paths, monkeypatch):
    """every term nu = 1 ... 4, forward and adjoint, on the generic kernels, per-node weights"""
    monkeypatch.setenv("HG_CORR_KERNEL", "nu")
    for doped in (False, True):
        r = K.check_block("cuda", K.IRREPS[1], 3, 67, doped=doped)
        print(r)
        assert r["max_rel_err"] < G.TOL, r


def test_corr_product_block_nu4_golden():
    """the reference's own CorrProductBlock(correlation=4) (tools/gen_golden_corr4.py): the default, natural-parity-filtered nu = 4 table"""
    r = G.check_corr_product(name="corr_product_block_nu4")
    print(r)
    assert r["corr_product_rel_err"] < G.TOL


def test_full_model_backward_transformer_correlation_4(oracle_paths):
    """training_step of a small HamGNNTransformer at `correlation: 4`: the loss and every parameter gradient against autograd through the oracle.
    The crystal, seed and depth are those of test_full_model_backward_transformer (tests/test_gpu_parity.py), the irreps narrowed to what a nu = 4 table can
    be planned for (even multiplicities: two heads).  A 2- or 3-atom crystal is NOT used: there the gradient of orb_transformers.0.residual.linear2.weight
    alone sits at 0.7 - 4.5e-5 of its largest value at EVERY correlation -- measured at correlation 2 and 3, on kernels this term does not touch
    (profiles/corr_nu.md) -- so such a graph says nothing about the nu = 4 term."""
    r = G.check_full_backward(n_atoms=5, seed=9, corr=4, nao=13, irr="4x0e+2x1o+2x2e", transformer=True)
    print(r)
    assert r["loss_rel_err"] < G.TOL and r["max_rel_err"] < G.TOL and r["n_params"] > 100, r


def test_full_model_backward_corr_product_correlation_4_doped(oracle_paths):
    """HamGNNConvE3 with use_corr_prod at `correlation: 4` and doped node attributes"""
    r = G.check_full_backward(n_atoms=2, seed=6, corr=4, nao=13, num_layers=1, irr="4x0e+3x1o+2x2e", charge=True, crystals=2)
    print(r)
    assert r["loss_rel_err"] < G.TOL and r["max_rel_err"] < G.TOL and r["n_params"] >= 60, r
