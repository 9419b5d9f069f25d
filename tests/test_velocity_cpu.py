"""hamgnn_amd/velocity.py without a GPU: the torch path and the numpy twin of hg_kgrad_elements (tests/velocity_checks.py) against the fp64 statement, the
Hellmann-Feynman velocities against a central difference of solved energies, the gauges, degenerate blocks, the transport weight rows through dos.broaden,
the argument checks and the library's export."""
import dataclasses

import numpy as np
import pytest
import torch

from hamgnn_amd import dos, velocity
from tests import bond_checks as BC
from tests import density_checks as DC
from tests import velocity_checks as VC

NAOS = sorted(BC.HEADS)


def _odd_edge_count(c):
    """an edge count of more than one chunk that is no multiple of the chunk"""
    E = c.E if c.E % VC.chunk_edges(c.E) else c.E - 3
    assert E % VC.chunk_edges(E) and VC.chunks(E) > 1
    return E


@pytest.mark.parametrize("npair", VC.NPAIRS)
@pytest.mark.parametrize("nao", NAOS)
def test_torch_path_within_the_bound(nao, npair):
    assert VC.check_case("cpu", nao, npair, kernel=False) <= 1.0


@pytest.mark.parametrize("npair", VC.NPAIRS)
@pytest.mark.parametrize("nao", NAOS)
def test_twin_within_the_kernel_bound(nao, npair, monkeypatch):
    """the numpy twin installed in place of ops.kgrad_elements: velocity.kgrad_elements takes its kernel route"""
    VC.install_cpu(monkeypatch)
    assert VC.check_case("cpu", nao, npair, kernel=True) <= 1.0


@pytest.mark.parametrize("route", ["torch", "twin"])
def test_edge_split_ends_zero_column_and_no_edge(route, monkeypatch):
    """one pair over all edges; an edge count that is no multiple of the chunk; a single chunk; a zero column of rvec gives exactly 0; E = 0 gives zeros"""
    if route == "twin":
        VC.install_cpu(monkeypatch)
    kernel = route == "twin"
    c = BC.case(19)
    assert VC.chunks(c.E) > 1
    assert VC.check_case("cpu", 19, 1, kernel) <= 1.0
    assert VC.check_case("cpu", 19, 17, kernel, E=_odd_edge_count(c)) <= 1.0
    assert VC.check_case("cpu", 19, 3, kernel, E=5) <= 1.0
    for col in range(3):
        assert VC.check_case("cpu", 27, 17, kernel, zero_col=col) <= 1.0
    bra, ket = VC.pairs(c, 17)
    out = VC.run(c, "cpu", bra, ket, E=0)
    assert out.shape == (17, 3) and out.dtype == np.complex64 and not out.view(np.float32).any()
    none = VC.run(c, "cpu", bra[:0], ket[:0])
    assert none.shape == (0, 3) and none.dtype == np.complex64


@pytest.mark.parametrize("nao", NAOS)
def test_twin_is_reproducible_and_pairs_do_not_depend_on_the_launch(nao, monkeypatch):
    VC.install_cpu(monkeypatch)
    c = BC.case(nao)
    bra, ket = VC.pairs(c, 33)
    a, b = VC.run(c, "cpu", bra, ket), VC.run(c, "cpu", bra, ket)
    assert np.array_equal(a.view(np.float32), b.view(np.float32))
    assert np.array_equal(VC.run(c, "cpu", bra[:5], ket[:5]).view(np.float32), a[:5].view(np.float32))


@pytest.mark.parametrize("nao", NAOS)
def test_torch_path_in_double_is_the_statement(nao):
    c = BC.case(nao)
    bra, ket = VC.pairs(c, 33)
    t = VC.tables_of(c, "cpu")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rv = VC.rvec_of(c)
    got = velocity._kgrad_elements_torch(d(c.C.astype(np.complex128)), d(bra), d(ket), d(c.kidx), d(c.kvec.astype(np.float64)), d(c.Xoff.astype(np.float64)),
                                         t.erow, t.ecol, t.shift.double(), d(rv.astype(np.float64)), t.orank, t.ooff, max_elems=1 << 10)
    ref, T = VC.ref_case(c, 33)
    assert got.dtype == torch.complex128 and np.abs(got.numpy() - ref).max() <= 1e-12 * T.max()


def test_edge_vectors_gauges_and_checks():
    c = BC.case(13)
    lat = velocity.edge_vectors(c.cell, c.shift)
    assert lat.dtype == torch.float32 and tuple(lat.shape) == (c.E, 3)
    want = c.shift.astype(np.float64) @ c.cell                 # the rows of cell are the lattice vectors
    assert np.array_equal(lat.numpy(), want.astype(np.float32))
    assert np.array_equal(velocity.edge_vectors(torch.from_numpy(c.cell)[None], torch.from_numpy(c.shift)).numpy(), lat.numpy())
    at = velocity.edge_vectors(c.cell, c.shift, pos=c.pos, edge_index=c.ei)
    assert np.array_equal(at.numpy(), (want + c.pos[c.ei[1]] - c.pos[c.ei[0]]).astype(np.float32))
    for name, kw in (("integer", dict(cell_shift=c.shift + 0.25)), ("go together", dict(pos=c.pos)), ("edge_index", dict(pos=c.pos, edge_index=c.ei[:, :-1])),
                     ("cell_shift", dict(cell_shift=c.shift[:, :2]))):
        with pytest.raises(ValueError, match=name):
            velocity.edge_vectors(**{**dict(cell=c.cell, cell_shift=c.shift), **kw})


def test_arguments_are_checked_on_the_host():
    c = BC.case(13)
    t = VC.tables_of(c, "cpu")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    bra, ket = VC.pairs(c, 17)
    good = dict(C=d(c.C), bra=d(bra), ket=d(ket), kidx=d(c.kidx), kvec=d(c.kvec), X_off=d(c.Xoff), tables=t, rvec=d(VC.rvec_of(c)))
    assert tuple(velocity.kgrad_elements(**good).shape) == (17, 3)
    across = ket.copy()
    across[4] += 1                                             # the ket of pair 4 moves to the other k-point
    bad_idx = c.kidx.copy()
    bad_idx[5] = len(c.kvec)
    for name, change in (("C", dict(C=d(c.C.astype(np.complex128)))), ("orbital columns", dict(C=d(c.C[:, :-1]))), ("bra", dict(bra=d(across))),
                         ("ket", dict(ket=d(ket + c.ns))), ("bra", dict(bra=d(-1 - bra))), ("bra", dict(bra=d(bra.astype(np.int64)))),
                         ("ket", dict(ket=d(ket[:-1]))), ("bra", dict(bra=d(bra).reshape(1, -1))), ("kidx", dict(kidx=d(bad_idx))),
                         ("kidx", dict(kidx=d(c.kidx.astype(np.int64)))), ("X_off", dict(X_off=d(c.Xoff.astype(np.float64)))),
                         ("X_off", dict(X_off=d(c.Xoff[:-1]))), ("rvec", dict(rvec=d(VC.rvec_of(c).astype(np.float64)))),
                         ("rvec", dict(rvec=d(VC.rvec_of(c)[:, :2]))), ("kvec", dict(kvec=d(c.kvec[:, :2]))),
                         ("erow", dict(tables=dataclasses.replace(t, erow=t.erow + c.N)))):
        with pytest.raises(ValueError, match=name):
            velocity.kgrad_elements(**{**good, **change})
    with pytest.raises(ValueError, match="same k-point"):
        velocity.kgrad_elements(**{**good, "ket": d(across)})


# ------------------------------------------------------------------------------------------------ physics on the solved crystal
def test_hellmann_feynman_statement_against_a_central_difference_fp64():
    """fp64 only: v = Re c^+ (dH - eps dS) c at the 8 grid points and 4 seeded random k-points against (eps(k + h) - eps(k - h)) / 2 h, h = 1e-5 per Angstrom
    along each Cartesian axis, within 1e-6 max |v| (measured on these k-points: 1.0e-6 at max |v| = 5.99, a sixth of the bound; the rest is room for a
    different LAPACK).  A state is left out only if a neighbouring level is closer than 1e-3 of the band width, and at most 10 % may be (on this case
    none is: the smallest spacing is 0.33 % of the width)."""
    s = VC.solved()
    v, fd = VC.hf_velocities(s)[0], VC.fd_velocities(s, 1e-5)
    gaps = np.diff(s.eps, axis=1)
    near = np.minimum(np.pad(gaps, ((0, 0), (1, 0)), constant_values=np.inf), np.pad(gaps, ((0, 0), (0, 1)), constant_values=np.inf))
    keep = (near >= 1e-3 * (s.eps.max() - s.eps.min())).reshape(-1)
    assert keep.mean() >= 0.9
    scale = np.abs(v).max()
    worst = float(np.abs(v - fd)[keep].max())
    print(f"max |v| = {scale:.3f}, left out {int((~keep).sum())} of {s.ns}, worst |HF - FD| = {worst:.2e}, smallest spacing / width = {near.min() / (s.eps.max() - s.eps.min()):.4f}")
    assert scale > 1.0 and worst <= 1e-6 * scale


def test_velocities_do_not_depend_on_the_gauge_but_off_diagonal_elements_do_fp64():
    s = VC.solved()
    c = s.c
    at = (c.shift.astype(np.float64) @ c.cell + c.pos[c.ei[1]] - c.pos[c.ei[0]]).astype(np.float32)
    v_lat, v_at = VC.hf_velocities(s)[0], VC.hf_velocities(s, at)[0]
    assert np.abs(v_lat - v_at).max() <= 1e-5 * np.abs(v_lat).max()                                  # (rvec is fp32 in both: 2^-24 of the terms)
    view = VC.solved_view(s, s.C128)
    bra, ket = np.array([0, 1], dtype=np.int32), np.array([3, 4], dtype=np.int32)
    off_lat = VC.ref_kgrad_elements(view, bra, ket, c.Hoff, VC.lattice_rvec(c))[0]
    off_at = VC.ref_kgrad_elements(view, bra, ket, c.Hoff, at)[0]
    assert np.abs(off_lat - off_at).max() > 1e-3 * np.abs(off_lat).max()


def test_time_reversal_partners_cancel_fp64():
    """real rows: eps(-k) = eps(k), so v(-k) = -v(k); where the grid holds k and -k (modulo a reciprocal lattice vector: on the 2 x 2 x 2 grid every point is
    its own partner) the velocities of the pair sum to zero -- a wrong sign of i R or of the phase would double them instead"""
    s = VC.solved()
    v = VC.hf_velocities(s)[0].reshape(s.nk, s.nb, 3)
    kg = s.kvec[:s.nk_grid].astype(np.float64)
    found = 0
    for a in range(s.nk_grid):
        for b in range(s.nk_grid):
            if np.abs((kg[a] + kg[b]) - np.rint(kg[a] + kg[b])).max() < 1e-12:
                found += 1
                assert np.abs(v[a] + v[b]).max() <= 1e-9 * np.abs(v).max()
    assert found >= s.nk_grid and np.abs(v[s.nk_grid:]).max() > 1.0


@pytest.mark.parametrize("route", ["torch", "twin"])
def test_band_velocities_against_the_statement(route, monkeypatch):
    if route == "twin":
        VC.install_cpu(monkeypatch)
    s = VC.solved()
    K = VC.k_kernel(s.c) if route == "twin" else VC.k_products(s.c)
    v, ref = VC.run_velocities(s, "cpu"), VC.hf_velocities(s)[0]
    tol = VC.velocity_tolerance(s, K)
    r = float((np.abs(v - ref) / tol).max())
    print(f"route={route} K={K} max |v| = {np.abs(ref).max():.3f} err/bound={r:.3f}")
    assert r <= 1.0
    # an orthonormal basis: S_off = None skips the second call and is the Hamiltonian term alone
    dH = VC.ref_kgrad_elements(VC.solved_view(s, s.C128), np.arange(s.ns), np.arange(s.ns), s.c.Hoff, VC.lattice_rvec(s.c))[0].real
    assert (np.abs(VC.run_velocities(s, "cpu", with_S=False) - dH) <= tol).all()


@pytest.mark.parametrize("route", ["torch", "twin"])
def test_degenerate_tol_joins_one_pair_and_leaves_the_rest(route, monkeypatch):
    if route == "twin":
        VC.install_cpu(monkeypatch)
    s = VC.solved()
    a, tol = VC.closest_pair(s)
    assert velocity.degenerate_runs(s.eps.reshape(-1), s.kidx, tol) == [(a, a + 2)]
    plain, joined = VC.run_velocities(s, "cpu"), VC.run_velocities(s, "cpu", degenerate_tol=tol)
    rest = np.ones(s.ns, dtype=bool)
    rest[a:a + 2] = False
    if route == "twin":
        assert np.array_equal(plain[rest], joined[rest])        # (the twin's pairs do not depend on the launch; the einsum of the torch path may)
    K = VC.k_kernel(s.c) if route == "twin" else VC.k_products(s.c)
    bound = VC.velocity_tolerance(s, K)
    assert (np.abs(plain - joined)[rest] <= 2 * bound[rest]).all()
    want = VC.degenerate_block_eigenvalues(s, a)
    # an eigenvalue of a Hermitian matrix moves by at most the norm of the perturbation: the two diagonal bounds + twice the off-diagonal element's, which
    # has the magnitude sum sqrt(T_a T_b) at most (Cauchy-Schwarz); the larger of the two stands for it
    room = 4 * bound[a:a + 2].max(0)
    assert (np.abs(joined[a:a + 2] - want) <= room[None, :]).all() and (np.diff(joined[a:a + 2], axis=0) >= 0).all()
    with pytest.raises(ValueError, match="contiguous and ascending"):
        velocity.degenerate_runs(s.eps.reshape(-1)[::-1], s.kidx, tol)


def test_transport_weights_through_broaden():
    """W = transport_weights(v, wk) through dos.broaden (torch path): column 1 + c is sum_s wk v_a v_b g(E - eps_s) for (a, b) in the order xx, yy, zz, yz, xz,
    xy, within the bound tests/dos_checks.py holds dos.broaden to + one rounding of the fp32 weight rows (2^-24 T); column 0 the DOS, pad columns 0"""
    from tests import dos_checks as DOSC
    s = VC.solved()
    order = np.argsort(s.eps.reshape(-1).astype(np.float32), kind="stable")
    eps = s.eps.reshape(-1).astype(np.float32)[order]
    v = VC.hf_velocities(s)[0].astype(np.float32)[order]
    wk = np.full(s.ns, 1.0 / s.nk, dtype=np.float32)
    W = velocity.transport_weights(torch.from_numpy(v), torch.from_numpy(wk))
    assert W.dtype == torch.float32 and tuple(W.shape) == (s.ns, dos.padded_groups(6)) == (s.ns, 16) and velocity.PAIRS == ("xx", "yy", "zz", "yz", "xz", "xy")
    assert np.array_equal(W[:, 0].numpy(), wk) and not W[:, 7:].any()
    vd, wd = v.astype(np.float64), wk.astype(np.float64)
    cols = [wd] + [wd * vd[:, i] * vd[:, j] for i, j in ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))]
    for q, col in enumerate(cols):
        assert np.abs(W[:, q].numpy() - col).max() <= VC.U * np.abs(col).max()
    width = float(eps.max() - eps.min())
    sigma, ne = 0.1 * width, 37
    E0, dE = float(eps.min()) - sigma, (width + 2 * sigma) / (ne - 1)
    D = dos.broaden(torch.from_numpy(eps), W, E0, dE, ne, sigma).numpy().astype(np.float64)
    _, bound, _ = DOSC.broaden_bound(eps, W.numpy(), E0, dE, ne, sigma)
    A = DOSC.gauss(E0 + dE * np.arange(ne), eps, sigma)
    assert not D[:, 7:].any()
    for q, col in enumerate(cols):
        assert (np.abs(D[:, q] - A @ col) <= bound[:, q] + VC.U * (A @ np.abs(col))).all(), q
    small = velocity.transport_weights(torch.from_numpy(v), torch.from_numpy(wk), Gp=7)
    assert tuple(small.shape) == (s.ns, 7) and np.array_equal(small.numpy(), W[:, :7].numpy())
    for name, kw in (("Gp", dict(Gp=6)), ("wk", dict(wk=torch.from_numpy(wk[:-1])))):
        with pytest.raises(ValueError, match=name):
            velocity.transport_weights(**{**dict(v=torch.from_numpy(v), wk=torch.from_numpy(wk)), **kw})


def test_library_exports_the_entry_point_and_sizes_its_scratch():
    import ctypes as C
    from hamgnn_amd import _lib
    L = _lib.lib()
    assert "hg_kgrad_elements" in _lib.EXPORTS and hasattr(L, "hg_kgrad_elements")
    call = _lib.call
    for E in (0, 1, 8, 9, 16, 17, 2048, 2049, 100000):         # the edge split of the twin is the library's: part [chunks][np][6] floats, none for one chunk
        want = VC.chunks(E) * 33 * 6 * 4 if VC.chunks(E) > 1 else 0
        assert call("hg_scratch_bytes", b"hg_kgrad_elements", 33, E) == want, E
    assert VC.chunks(100000) <= 256 and VC.chunk_edges(17) == 8 and VC.chunks(17) == 3
    sizes = dict(ns=5, M=4, n_pairs=3, nk=1, n_edges=0, n_atoms=1, nao=13)      # NULL tensors only: none of these reaches a launch

    def run(**kw):
        a = {**sizes, **kw}
        return call("hg_kgrad_elements", None, a["ns"], a["M"], None, None, a["n_pairs"], None, None, a["nk"], None, None, None, None, None, a["n_edges"],
                    a["n_atoms"], a["nao"], None, None, None, None)
    assert run(n_pairs=0) is None                              # no pair: no launch
    for bad in (dict(nao=49), dict(nao=0), dict(M=0), dict(nk=0), dict(n_atoms=0), dict(ns=0), dict(n_edges=-1), dict(n_edges=2 ** 31), dict()):
        with pytest.raises(RuntimeError, match="hg_kgrad_elements"):
            run(**bad)
