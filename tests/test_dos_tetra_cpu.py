"""The linear tetrahedron method of hamgnn_amd/dos.py without a GPU: the grid's map and tetrahedra, the weight formulas on the fp64 twin of
tests/dos_tetra_checks.py (pinned values, subdivision invariance, sum rules, the flat rule), the Fermi level, the plain torch path against the twin under the
bound derived there, and the C ABI of hg_dos_tetra."""
import os
import re

import numpy as np
import pytest
import torch

from hamgnn_amd import _lib, dos, ops
from tests import dos_checks as DC
from tests import dos_tetra_checks as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOFLAT = 1e-9                                               # a grid step below every corner spread of the random cases: the flat rule stays out


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("grid", TC.GRIDS)
@pytest.mark.parametrize("shift", [(0, 0, 0), (0.5, 0.5, 0.5)])
@pytest.mark.parametrize("time_reversal", [True, False])
def test_monkhorst_pack_map_agrees_with_monkhorst_pack(grid, shift, time_reversal):
    k_full, _ = dos.monkhorst_pack(grid, shift, time_reversal=False)
    k_kept, w = dos.monkhorst_pack(grid, shift, time_reversal=time_reversal)
    m = dos.monkhorst_pack_map(grid, shift, time_reversal)
    assert m.dtype == np.int32 and m.shape == (int(np.prod(grid)),) and m.min() == 0 and m.max() == len(w) - 1
    same = np.abs((k_full - k_kept[m] + 0.5) % 1.0 - 0.5).max(1) < 1e-9
    minus = np.abs((k_full + k_kept[m] + 0.5) % 1.0 - 0.5).max(1) < 1e-9
    assert (same | minus).all() and (time_reversal or same.all())
    assert np.abs(np.bincount(m, minlength=len(w)) / len(k_full) - w).max() < 1e-14


@pytest.mark.parametrize("grid", TC.GRIDS)
def test_tetrahedra_count_and_corner_table(grid):
    nfull = int(np.prod(grid))
    tet = dos.tetrahedra(grid, TC.SKEW, time_reversal=False)
    assert tet.dtype == np.int32 and tet.shape == (6 * nfull, 4)
    assert (np.bincount(tet.reshape(-1), minlength=nfull) == 24).all()
    folded = dos.tetrahedra(grid, TC.SKEW, time_reversal=True)
    assert np.array_equal(folded, dos.monkhorst_pack_map(grid)[tet])
    nk = int(folded.max()) + 1
    ptr, kt_tet, kt_corner = dos.corner_table(folded, nk)
    assert ptr.dtype == kt_tet.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == 4 * len(folded) and len(ptr) == nk + 1
    assert sorted(zip(kt_tet.tolist(), kt_corner.tolist())) == [(t, c) for t in range(len(folded)) for c in range(4)]
    for k in range(nk):
        seg = slice(ptr[k], ptr[k + 1])
        assert (folded[kt_tet[seg], kt_corner[seg]] == k).all()
        pairs = list(zip(kt_tet[seg].tolist(), kt_corner[seg].tolist()))
        assert pairs == sorted(pairs)                           # ascending tetrahedron, then slot: the kernel's summation order
    with pytest.raises(ValueError):
        dos.corner_table(folded, nk - 1)


@pytest.mark.parametrize("cell", [np.eye(3), TC.SKEW], ids=["cubic", "skewed"])
def test_cell_is_cut_around_its_shortest_diagonal_into_six_equal_volumes(cell):
    grid = (4, 3, 2)
    off = dos.cell_tetrahedra(grid, cell)
    assert off.shape == (6, 4, 3) and off.min() == 0 and off.max() == 1
    step = np.linalg.inv(cell).T / np.asarray(grid, dtype=np.float64)[:, None]
    diagonals = [(np.array(a), 1 - np.array(a)) for a in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))]
    lengths = [np.linalg.norm((b - a) @ step) for a, b in diagonals]
    common = set(map(tuple, off[0]))
    for t in off[1:]:
        common &= set(map(tuple, t))
    assert len(common) == 2                                     # the six share one edge: the diagonal
    a, b = (np.array(c) for c in common)
    assert (a + b == 1).all() and np.linalg.norm((b - a) @ step) <= min(lengths) + 1e-15
    if cell is TC.SKEW:
        assert np.argmin(lengths) != 0                          # not the 000 - 111 diagonal: the choice is exercised
    cart = off.astype(np.float64) @ step
    vol = np.array([np.linalg.det(t[1:] - t[0]) / 6.0 for t in cart])
    assert np.abs(vol - vol[0]).max() < 1e-15 * abs(vol[0]) * 10 and abs(vol.sum() - np.linalg.det(step)) < 1e-14 * abs(vol.sum())
    mid = cart.mean(1)                                          # ... and they do not overlap: each one's centroid lies in no other
    for i, t in enumerate(cart):
        lam = np.linalg.solve(np.vstack([t.T, np.ones(4)]), np.vstack([mid.T, np.ones(6)]))
        assert [j for j in range(6) if lam[:, j].min() > 1e-12] == [i]


# ------------------------------------------------------------------------------------------------ the formulas, fp64
def test_pinned_values_of_one_tetrahedron():
    es = np.array([0.0, 1.0, 2.0, 3.0])
    for E, g in ((0.5, 0.125), (1.5, 0.75), (2.5, 0.125)):
        assert abs(TC.tetra_dos_total(es, E, 1.0) - g) < 1e-15
    c = TC.corner_weights(es, np.float64(0.5), 1.0, NOFLAT, -9.0, 9.0, 0)
    assert np.abs(c / 0.125 - np.array([25 / 36, 1 / 6, 1 / 12, 1 / 18])).max() < 1e-15
    t = dos._tetra_corner_weights(torch.from_numpy(es), torch.tensor(0.5, dtype=torch.float64), 1.0, NOFLAT, -9.0, 9.0, 0).numpy()
    assert np.abs(t - c).max() < 1e-16
    w = TC.corner_weights(es, np.float64(1.5), 1.0, NOFLAT, -9.0, 9.0, 1)                  # the mirror image e -> 3 - e: w_i + w_(5 - i) = v / 4
    assert abs(w[0] + w[3] - 0.25) < 1e-15 and abs(w[1] + w[2] - 0.25) < 1e-15 and w[0] > w[1] > w[2] > w[3] > 0


def _random_tetrahedra(n, seed):
    """corner energies [4, n] of n random tetrahedra (unsorted), one in four with two corners exactly equal at a random rank, + weights [4, n, 3]"""
    rng = np.random.default_rng(seed)
    e = rng.uniform(-1.0, 1.0, (4, n))
    for i in range(0, n, 4):
        s = np.sort(e[:, i])
        r = (i // 4) % 3
        s[r + 1] = s[r]                                         # e1 = e2, e2 = e3, e3 = e4 in turn
        e[:, i] = rng.permutation(s)
    return e, rng.normal(size=(4, n, 3))


def test_corner_weights_sum_to_the_total_dos():
    e, _ = _random_tetrahedra(400, 1)
    es = np.sort(e.T, axis=1)
    E = np.random.default_rng(2).uniform(-1.0, 1.0, 400)
    c, g = TC.corner_weights(es, E, 1.0, NOFLAT, -9.0, 9.0, 0), TC.tetra_dos_total(es, E, 1.0)
    assert g.max() > 1.0 and (c >= 0).all() and np.abs(c.sum(-1) - g).max() <= 1e-14 * g.max()
    t = dos._tetra_corner_weights(torch.from_numpy(es), torch.from_numpy(E), 1.0, NOFLAT, -9.0, 9.0, 0).numpy()
    assert np.abs(t - c).max() <= 1e-12 * g.max()               # the derivative form of the torch path and the kernel = the geometric centroid


@pytest.mark.parametrize("mode", [0, 1])
def test_subdivision_invariance(mode):
    """every tetrahedron split into 8 through its edge midpoints, energies and weights interpolated linearly: the DOS / PDOS (and the number of states) change
    by rounding only.  A wrong corner weight does not survive this."""
    e, w = _random_tetrahedra(240, 3)
    eps10, W10 = TC.with_midpoints(e), TC.with_midpoints(w)
    E0, dE, ne = -0.95, 0.0317, 60
    E = E0 + dE * np.arange(ne)
    D = [np.einsum("jkb,kbg->jg", TC.operand(eps10, tet, E, NOFLAT, -9.0, 9.0, mode), W10) for tet in (TC.COARSE, TC.FINE)]
    assert np.abs(D[0]).max() > 1.0 and np.abs(D[0] - D[1]).max() <= 1e-11 * np.abs(D[0]).max()
    per_band = [TC.operand(eps10, tet, E, NOFLAT, -9.0, 9.0, mode) for tet in (TC.COARSE, TC.FINE)]      # ... and band by band, the tied ones included
    tot = [np.einsum("jkb,kbg->jbg", a, W10) for a in per_band]
    assert np.abs(tot[0] - tot[1]).max() <= 1e-11 * np.abs(tot[0]).max()


def test_states_are_the_integral_of_the_dos():
    e, _ = _random_tetrahedra(40, 4)
    es = np.sort(e.T, axis=1)
    x, wq = np.polynomial.legendre.leggauss(12)
    for E in (-0.4, 0.1, 0.7):
        knots = np.sort(np.concatenate([es, np.full((40, 1), -1.0)], 1), axis=1)       # piecewise polynomial between the corner energies: Gauss is exact
        total = np.zeros((40, 4))
        for i in range(4):
            lo, hi = np.minimum(knots[:, i], E), np.minimum(knots[:, i + 1], E)
            for xx, ww in zip(x, wq):
                t = 0.5 * (lo + hi) + 0.5 * (hi - lo) * xx
                total += (0.5 * (hi - lo) * ww)[:, None] * TC.corner_weights(es, t, 1.0, NOFLAT, -9.0, 9.0, 0)
        assert np.abs(total - TC.corner_weights(es, np.full(40, E), 1.0, NOFLAT, -9.0, 9.0, 1)).max() < 1e-13


@pytest.mark.parametrize("grid", TC.GRIDS)
def test_sum_rule_and_monotony_of_the_number_of_states(grid):
    """mode 1 at any E >= max eps = sum_k sum_b W[k, b] / nk on the full grid (k-weights on the folded one), flat bands included; non-decreasing for W >= 0"""
    for tr in (False, True):
        tet, nk = TC.grid_case(grid, tr)
        eps, W = TC.bands(nk, 5, seed=1)
        W = np.abs(W[:, :, :4]).astype(np.float64)
        kw = dos.monkhorst_pack(grid, time_reversal=tr)[1]
        E0 = float(eps.max())
        top = TC.ref_terms(eps, W, tet, E0, 0.05, 3, 1)[0]
        want = (W * kw[:, None, None]).sum((0, 1))
        assert np.abs(top - want[None]).max() <= 1e-13 * want.max()
        N = TC.ref_terms(eps, W, tet, -0.1, 0.0173, 160, 1)[0]
        assert N[0].max() == 0.0 and (np.diff(N, axis=0) >= -1e-14).all() and np.abs(N[-1] - want).max() <= 1e-13 * want.max()


def test_flat_band_on_a_gamma_only_grid_sits_on_the_two_bracketing_energies():
    tet, nk = TC.grid_case((1, 1, 1))
    assert nk == 1 and tet.shape == (6, 4) and not tet.any()
    eps, W = np.array([[0.137, 0.9]]), np.array([[[1.0, 2.0], [1.0, -3.0]]])
    E0, dE, ne = 0.0, 0.05, 10                                  # 0.137 = 2.74 steps; 0.9 lies outside the grid [0, 0.45]
    D = TC.ref_terms(eps, W, tet, E0, dE, ne, 0)[0]
    assert np.flatnonzero(D[:, 0]).tolist() == [2, 3] and abs(D[2, 0] * dE - 0.26) < 1e-12 and abs(D[3, 0] * dE - 0.74) < 1e-12
    assert np.abs(D.sum(0) * dE - np.array([1.0, 2.0])).max() < 1e-12
    N = TC.ref_terms(eps, W, tet, E0, dE, ne, 1)[0]
    assert not N[:3].any() and np.abs(N[3:] - np.array([1.0, 2.0])).max() < 1e-15
    T = dos.tetra_dos(torch.tensor(eps, dtype=torch.float32), torch.tensor(W, dtype=torch.float32), tet, E0, dE, ne).double().numpy()
    assert np.flatnonzero(T[:, 0]).tolist() == [2, 3] and np.abs(T.sum(0) * dE - np.array([1.0, 2.0])).max() < 1e-5


@pytest.mark.parametrize("mode", [0, 1])
def test_time_reversal_on_and_off_give_the_same_result(mode):
    grid = (4, 3, 2)
    tet_f, nk_f = TC.grid_case(grid, False)
    tet_r, nk_r = TC.grid_case(grid, True)
    eps_r, W_r = TC.bands(nk_r, 5, seed=2)
    m = dos.monkhorst_pack_map(grid)
    a = TC.ref_terms(eps_r, W_r, tet_r, TC.E0_, TC.DE_, 37, mode)[0]
    b = TC.ref_terms(eps_r[m], W_r[m], tet_f, TC.E0_, TC.DE_, 37, mode)[0]
    assert nk_r < nk_f and np.abs(a).max() > 0.1 and np.abs(a - b).max() <= 1e-13 * np.abs(a).max()


def test_fermi_level_tetra():
    tet, nk = TC.grid_case((4, 3, 2))
    rng = np.random.default_rng(5)
    eps = np.sort(rng.uniform(-1.0, 1.0, (nk, 6)), axis=1)
    eps[:, 3:] += 3.0                                           # a gap between bands 2 and 3: (max of band 2, min of band 3)
    count = lambda mu: 2.0 * TC.ref_terms(eps, np.ones((nk, 6, 1)), tet, mu, NOFLAT, 1, 1)[0][0, 0]
    for nel in (0.7, 3.3, 5.9, 9.1):
        mu = dos.fermi_level_tetra(eps, tet, nel, 2)
        assert abs(count(mu) - nel) <= 1e-10, (nel, mu, count(mu))
    mu = dos.fermi_level_tetra(eps, tet, 6.0, 2)                # three full bands: the middle of the gap
    assert abs(mu - 0.5 * (eps[:, 2].max() + eps[:, 3].min())) < 1e-9
    assert abs(dos.fermi_level_tetra(eps, tet, 3.0, 1) - mu) < 1e-9
    with pytest.raises(ValueError):
        dos.fermi_level_tetra(eps, tet, 12.5, 2)


# ------------------------------------------------------------------------------------------------ the torch path against the twin
@pytest.mark.parametrize("grid", TC.GRIDS)
def test_torch_path_vs_fp64_on_the_random_cases(grid):
    assert TC.check_shapes(TC.run_dos, "cpu", grid) <= 1.0


@pytest.mark.parametrize("mode", [0, 1])
def test_torch_path_structure(mode):
    assert max(TC.check_structure("cpu", mode).values()) <= 1.0


@pytest.mark.parametrize("time_reversal,mode", [(True, 0), (False, 1)])
def test_torch_path_on_the_fixture_crystals(time_reversal, mode):
    assert TC.check_chain("cpu", time_reversal, mode) <= 1.0


# ------------------------------------------------------------------------------------------------ the C ABI and the wrapper
def test_abi_header_export_and_zero_scratch():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "hamgnn_hip.h")).read()
    assert "hg_dos_tetra" in set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", hdr)) and "hg_dos_tetra" in _lib.EXPORTS and callable(ops.dos_tetra)
    L = _lib.lib()
    L.hg_scratch_bytes.restype = C.c_int64
    L.hg_scratch_bytes.argtypes = [C.c_char_p, C.c_int64, C.c_int]
    assert L.hg_scratch_bytes(b"hg_dos_tetra", 1000, 0) == 0


def test_entry_point_checks_its_arguments_and_launches_nothing_for_empty_sizes():
    """every call passes NULL pointers only, and sizes that are either empty (0 before any launch) or refused whatever the pointers are: none can reach a launch"""
    import ctypes as C
    L = _lib.lib()
    null, d, i64 = C.c_void_p(0), C.c_double, C.c_int64

    def call(nk=4, nb=3, Gp=4, nt=6, dE=0.1, ne=10, mode=0):
        return L.hg_dos_tetra(null, null, nk, nb, Gp, null, i64(nt), null, null, null, null, null, d(0.0), d(dE), ne, mode, 0, null, null)
    assert call(ne=0) == 0                                     # no energy
    for bad in (dict(dE=0.0), dict(dE=-0.1), dict(mode=2), dict(mode=-1), dict(nt=-1), dict(Gp=0), dict()):       # the last: good sizes, NULL tensors
        assert call(**bad) == -2, bad
        assert b"hg_dos_tetra" in L.hg_last_error()


def test_wrapper_refuses_sliced_or_mistyped_tensors(monkeypatch):
    monkeypatch.setattr(ops, "_require_gpu", lambda t: None)
    nk, nb, Gp, nt = 2, 3, 4, 6
    good = dict(eps=torch.zeros(nk, nb), W=torch.zeros(nk, nb, Gp), tet=torch.zeros(nt, 4, dtype=torch.int32), kt_ptr=torch.zeros(nk + 1, dtype=torch.int32),
                kt_tet=torch.zeros(4 * nt, dtype=torch.int32), kt_corner=torch.zeros(4 * nt, dtype=torch.int32), lo=torch.zeros(nb), hi=torch.zeros(nb), D=torch.zeros(5, Gp))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        extra = {k: a.pop(k) for k in ("mode", "accumulate") if k in a}
        return ops.dos_tetra(a["eps"], a["W"], a["tet"], (a["kt_ptr"], a["kt_tet"], a["kt_corner"]), a["lo"], a["hi"], 0.0, 0.1, 5, D=a["D"], **extra)
    for bad in (dict(eps=torch.zeros(nk, 2 * nb)[:, ::2]), dict(W=torch.zeros(nk, nb, 2 * Gp)[:, :, ::2]), dict(D=torch.zeros(5, 2 * Gp)[:, :Gp]),
                dict(tet=torch.zeros(nt, 8, dtype=torch.int32)[:, ::2]), dict(kt_tet=torch.zeros(8 * nt, dtype=torch.int32)[::2]), dict(hi=torch.zeros(2 * nb)[::2])):
        with pytest.raises(ValueError, match="contiguous"):
            call(**bad)
    for bad in (dict(eps=torch.zeros(nk, nb, dtype=torch.float64)), dict(tet=torch.zeros(nt, 4, dtype=torch.int64)), dict(kt_corner=torch.zeros(4 * nt, dtype=torch.int8))):
        with pytest.raises(ValueError, match="float32"):
            call(**bad)
    for bad in (dict(eps=torch.zeros(nk, nb + 1)), dict(kt_ptr=torch.zeros(nk, dtype=torch.int32)), dict(lo=torch.zeros(nb + 1)), dict(tet=torch.zeros(nt, 3, dtype=torch.int32))):
        with pytest.raises(ValueError, match="shapes"):
            call(**bad)
    with pytest.raises(ValueError, match="mode"):
        call(mode=2)
    with pytest.raises(ValueError, match="D must be"):
        call(D=torch.zeros(4, Gp))
    with pytest.raises(ValueError, match="accumulate"):
        call(D=None, accumulate=True)
    with pytest.raises(ValueError):
        dos.tetra_dos(torch.zeros(nk, nb), torch.zeros(nk + 1, nb, Gp), np.zeros((nt, 4), dtype=np.int32), 0.0, 0.1, 5)
