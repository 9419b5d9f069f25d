"""hg_kgrad_elements (csrc/spectra.hip) on the GPU through hamgnn_amd/velocity.py: against the fp64 statement inside the derived bound of
tests/velocity_checks.py, its structure (bit-reproducible, pairs independent of the launch, the edge split at both ends, exact zeros), the argument checks,
the torch path on the device, and band velocities / degenerate blocks on the eigenpairs of a small crystal solved on the host."""

import numpy as np
import pytest
import torch

from hamgnn_amd import velocity
from tests import bond_checks as BC
from tests import density_checks as DC
from tests import velocity_checks as VC

pytestmark = pytest.mark.gpu
NAOS = sorted(BC.HEADS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("npair", VC.NPAIRS)
@pytest.mark.parametrize("nao", NAOS)
def test_kernel_vs_fp64(nao, npair):
    """nao 13 / 19 / 27 / 40: one, two, two and three row tiles, rectangular blocks, an atom without edges, shifts out to +-30 cells; np: a lone pair over
    all edges, a partial tile, one tile, a second tile's first pair, three tiles; diagonal and off-diagonal pairs mixed; more than one chunk of edges"""
    assert VC.chunks(BC.case(nao).E) > 1
    assert VC.check_case("cuda", nao, npair, kernel=True) <= 1.0


def test_edge_split_ends_zero_column_and_no_edge():
    c = BC.case(19)
    E = c.E if c.E % VC.chunk_edges(c.E) else c.E - 3           # more than one chunk, the last one partial
    assert E % VC.chunk_edges(E) and VC.chunks(E) > 1
    assert VC.check_case("cuda", 19, 17, True, E=E) <= 1.0
    assert VC.check_case("cuda", 19, 3, True, E=5) <= 1.0       # a single chunk: no second pass, two waves without an edge
    for col in range(3):
        assert VC.check_case("cuda", 27, 17, True, zero_col=col) <= 1.0
    bra, ket = VC.pairs(c, 17)
    out = VC.run(c, "cuda", bra, ket, E=0)
    assert out.shape == (17, 3) and out.dtype == np.complex64 and not out.view(np.float32).any()
    assert VC.run(c, "cuda", bra[:0], ket[:0]).shape == (0, 3)


@pytest.mark.parametrize("nao", NAOS)
def test_launches_are_bit_identical_and_pairs_do_not_depend_on_the_launch(nao):
    c = BC.case(nao)
    bra, ket = VC.pairs(c, 33)
    a, b = VC.run(c, "cuda", bra, ket), VC.run(c, "cuda", bra, ket)
    assert np.array_equal(a.view(np.float32), b.view(np.float32))
    assert np.array_equal(VC.run(c, "cuda", bra[:5], ket[:5]).view(np.float32), a[:5].view(np.float32))
    assert np.array_equal(VC.run(c, "cuda", bra[16:], ket[16:]).view(np.float32), a[16:].view(np.float32))


def test_torch_path_on_the_device(monkeypatch):
    monkeypatch.setenv("HG_DOS", "torch")
    assert VC.check_case("cuda", 27, 33, kernel=False) <= 1.0


def test_arguments_are_checked_on_the_host():
    c = BC.case(13)
    t = VC.tables_of(c, "cuda")
    d = lambda a: DC.dev(a, "cuda")
    bra, ket = VC.pairs(c, 17)
    good = dict(C=d(c.C), bra=d(bra), ket=d(ket), kidx=d(c.kidx), kvec=d(c.kvec), X_off=d(c.Xoff), tables=t, rvec=d(VC.rvec_of(c)))
    assert tuple(velocity.kgrad_elements(**good).shape) == (17, 3)
    across = ket.copy()
    across[4] += 1                                             # the ket of pair 4 moves to the other k-point
    wide = d(np.concatenate([c.C, c.C], 1))
    for name, change in (("C", dict(C=d(c.C.astype(np.complex128)))), ("contiguous", dict(C=wide[:, :c.M])), ("ket", dict(ket=d(across))), ("ket", dict(ket=d(ket + c.ns))),
                         ("bra", dict(bra=d(-1 - bra))), ("bra", dict(bra=d(bra.astype(np.int64)))), ("ket", dict(ket=d(ket[:-1]))),
                         ("X_off", dict(X_off=d(c.Xoff.astype(np.float64)))), ("rvec", dict(rvec=d(VC.rvec_of(c)[:-1]))), ("rvec", dict(rvec=d(VC.rvec_of(c)).cpu())),
                         ("kidx", dict(kidx=d(c.kidx.astype(np.int64))))):
        with pytest.raises(ValueError, match=name):
            velocity.kgrad_elements(**{**good, **change})


def test_band_velocities_and_degenerate_blocks_on_host_solved_eigenpairs():
    """2 atoms, nao 13, the 2 x 2 x 2 grid + 4 random k-points solved in fp64 on the host; band_velocities through the kernel against the fp64
    Hellmann-Feynman statement within the composed bound of velocity_checks.velocity_tolerance; degenerate_tol joining the closest pair of levels gives the
    eigenvalues of the fp64 2 x 2 blocks and leaves every other state's bits alone"""
    s = VC.solved()
    K = VC.k_kernel(s.c)
    ref, bound = VC.hf_velocities(s)[0], VC.velocity_tolerance(s, K)
    v = VC.run_velocities(s, "cuda")
    r = float((np.abs(v - ref) / bound).max())
    print(f"K={K} max |v| = {np.abs(ref).max():.3f} err/bound={r:.3f}")
    assert r <= 1.0
    a, tol = VC.closest_pair(s)
    joined = VC.run_velocities(s, "cuda", degenerate_tol=tol)
    rest = np.ones(s.ns, dtype=bool)
    rest[a:a + 2] = False
    assert np.array_equal(v[rest], joined[rest])
    want = VC.degenerate_block_eigenvalues(s, a)
    assert (np.abs(joined[a:a + 2] - want) <= 4 * bound[a:a + 2].max(0)[None, :]).all() and (np.diff(joined[a:a + 2], axis=0) >= 0).all()
