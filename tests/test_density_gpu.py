"""hg_density_rows (csrc/spectra.hip) on the GPU through hamgnn_amd/density.py: against the fp64 statement inside the derived bound of tests/density_checks.py,
its structure (every element written, accumulate, bit-reproducible, members independent of the launch), against the bond-weight kernel, the sum rules on
the eigenpairs of a small crystal solved on the host, and the argument checks."""
import dataclasses

import numpy as np
import pytest
import torch

from hamgnn_amd import bonds, density, dos
from tests import bond_checks as BC
from tests import density_checks as DC

pytestmark = pytest.mark.gpu
NAOS = sorted(BC.HEADS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("ns", DC.NS)
@pytest.mark.parametrize("nao", NAOS)
def test_kernel_vs_fp64(nao, ns):
    """nao 13 / 19 / 27 / 40: one, two, two and three tiles of compact ranks, rectangular blocks, atoms lacking orbitals, an atom without edges, edge pairs
    moved +-30 cells out; ns: fewer states than waves, the 4-state tail, exact multiples, an uneven split over the waves; two k-points interleave; f has both
    signs.  Every element inside the kernel's bound, zeros exact."""
    c = BC.case(nao)
    assert (DC.weights(c) > 0).any() and (DC.weights(c) < 0).any()
    assert DC.check_rows(DC.run(c, "cuda", hi=ns), DC.ref_case(c, 0, ns), DC.k_kernel(ns), f"kernel nao={nao} ns={ns}") <= 1.0


def test_phase_of_a_k_point_beyond_the_tabulated_ones():
    """a k-list longer than the kernel's phase table (1024 k-points per member): the states sit at k-points 3 (tabulated) and 1029 (formed per state)"""
    c = BC.case(19)
    kvec = np.random.default_rng(11).uniform(-0.5, 0.5, size=(1030, 3)).astype(np.float32)
    kidx = np.where(np.arange(c.ns) % 2 == 1, 1029, 3).astype(np.int32)
    ref = DC.ref_density_rows(c, c.C, kidx, DC.weights(c), kvec=kvec)
    assert DC.check_rows(DC.run(c, "cuda", kidx=kidx, kvec=kvec), ref, DC.k_kernel(c.ns), "kernel nao=19 nk=1030") <= 1.0


@pytest.mark.parametrize("nao", NAOS)
def test_accumulate_adds_state_chunks(nao):
    """rows from the states [0, 17) then [17, 33) accumulated, against the fp64 statement of all 33 and against one launch over all 33, both within the sum of
    the two launches' bounds (the split changes the summation order: the difference to the one launch need not be 0); elements at missing orbitals are
    written by the first launch (0) and left alone by the second"""
    c = BC.case(nao)
    have = DC.tables_of(c, "cpu").orank.numpy() >= 0
    miss_on = ~(have[:, :, None] & have[:, None, :]).reshape(c.N, -1)
    miss_off = ~(have[c.ei[0]][:, :, None] & have[c.ei[1]][:, None, :]).reshape(c.E, -1)
    out = (torch.full((c.N, nao * nao), 7.0, device="cuda"), torch.full((c.E, nao * nao), 7.0, device="cuda"))
    DC.run(c, "cuda", hi=17, out=out)
    assert not out[0].cpu().numpy()[miss_on].any() and not out[1].cpu().numpy()[miss_off].any()
    out[0][torch.from_numpy(miss_on).cuda()] = 7.0
    DC.run(c, "cuda", lo=17, out=out, accumulate=True)
    got = (out[0].cpu().numpy(), out[1].cpu().numpy())
    assert (got[0][miss_on] == 7.0).all() and not got[1][miss_off].any()
    got[0][miss_on] = 0.0
    one = DC.run(c, "cuda")
    ref, r1, r2 = DC.ref_case(c, 0, c.ns), DC.ref_case(c, 0, 17), DC.ref_case(c, 17, c.ns)
    for g, o, want, Ta, Tb in ((got[0], one[0], ref[0], r1[2], r2[2]), (got[1], one[1], ref[1], r1[3], r2[3])):
        two = DC.bound(Ta, DC.k_kernel(17)) + DC.bound(Tb, DC.k_kernel(c.ns - 17))
        r_ref, r_one = DC.ratio(g, want, two), DC.ratio(g, o.astype(np.float64), two)
        print(f"nao={nao} accumulated vs fp64 err/bound={r_ref:.3f}, vs one launch={r_one:.3f}, differing elements={int((g != o).sum())}")
        assert r_ref <= 1.0 and r_one <= 1.0


@pytest.mark.parametrize("nao", NAOS)
def test_launches_are_bit_identical_and_members_do_not_depend_on_the_launch(nao):
    c = BC.case(nao)
    P1, P2 = DC.run(c, "cuda"), DC.run(c, "cuda")
    assert float(np.abs(P1[0] - P2[0]).max()) == 0.0 and float(np.abs(P1[1] - P2[1]).max()) == 0.0
    e = 0                                                       # edge 0 and its two atoms keep their columns of C, every other column is perturbed
    keep = np.zeros(c.M, dtype=bool)
    for i in (int(c.ei[0, e]), int(c.ei[1, e])):
        keep[c.off0[i]:c.off0[i + 1]] = True
    assert not keep.all()
    C2 = c.C.copy()
    C2[:, ~keep] += np.complex64(0.5 - 0.25j)
    P3 = DC.run(c, "cuda", C=C2)
    same_e = [q for q in range(c.E) if keep[c.off0[c.ei[0, q]]] and keep[c.off0[c.ei[1, q]]]]
    same_a = [i for i in range(c.N) if keep[c.off0[i]]]
    assert e in same_e and float(np.abs(P1[1][same_e] - P3[1][same_e]).max()) == 0.0 and float(np.abs(P1[0][same_a] - P3[0][same_a]).max()) == 0.0
    assert float(np.abs(P1[0] - P3[0]).max()) > 0.0            # (the other members did change)


@pytest.mark.parametrize("by", bonds.BY)
@pytest.mark.parametrize("nao", NAOS)
def test_bond_populations_agree_with_the_bond_weight_kernel(nao, by):
    """HIP vs HIP: sum_members sum_ab P X of the kernel's rows = sum_s of the columns of bonds.bond_weights(..., wk = f), within the bond kernel's bound summed
    over the states + sum_ab |X_ab| bound_P over the group's members.  Both sums (over ab and members here, over s there) are taken in fp64, so that
    only the two kernels' roundings enter."""
    import types
    c = BC.case(nao)
    f = DC.weights(c)
    groups = BC.groupings(c)[by]
    G = len(groups[0]) - 1
    Gp = dos.padded_groups(G)
    t = DC.tables_of(c, "cuda")
    d = lambda a: DC.dev(a, "cuda")
    W = bonds.bond_weights(d(c.C), d(c.kidx), d(c.kvec), d(c.Xon), d(c.Xoff), t, groups, d(f), Gp).cpu().numpy().astype(np.float64)
    P_on, P_off = density.density_rows(d(c.C), d(c.kidx), d(c.kvec), d(f), t)
    got = density.bond_populations(P_on.double(), P_off.double(), d(c.Xon).double(), d(c.Xoff).double(), groups).cpu().numpy()
    key = ("absf", nao)
    if key not in DC._FIX:                                      # the bond kernel's bound with wk = |f|
        DC._FIX[key] = types.SimpleNamespace(**{**vars(c), "wk": np.abs(f)})
    _, T, kp, kk = BC.ref_bond_weights(DC._FIX[key], groups, Gp)
    ref = DC.ref_case(c, 0, c.ns)
    bP = lambda T_: DC.bound(T_, DC.k_kernel(c.ns))
    m_on = (np.abs(c.Xon.astype(np.float64)) * bP(ref[2])).sum(1)
    m_off = (np.abs(c.Xoff.astype(np.float64)) * bP(ref[3])).sum(1)
    eptr, eidx, aptr, aidx = groups
    worst = 0.0
    for g in range(G):
        tol = BC.bound(T, np.minimum(kk, kp))[:, 1 + g].sum() + m_off[eidx[eptr[g]:eptr[g + 1]]].sum() + m_on[aidx[aptr[g]:aptr[g + 1]]].sum()
        worst = max(worst, abs(got[g] - W[:, 1 + g].sum()) / tol)
    print(f"nao={nao} by={by} G={G} density kernel vs bond kernel err/bound={worst:.3f}")
    assert got.shape == (G,) and worst <= 1.0


def test_sum_rules_on_host_solved_eigenpairs():
    """2 atoms, nao 13, 2 x 2 x 2, eigenpairs solved on the host in fp64, f = k_w occupations at dos.fermi_level's mu: over all members sum P . S = sum f and
    sum P . H = sum f eps (the energy-weighted call: f eps with overlap rows gives the same number), and populations(...)[0].sum() equals them.  The sums
    over ab and members are taken in fp64 (double tensors) so that only the kernel's bound is carried."""
    s = DC.solved_case()
    c = s.c
    d = lambda a: DC.dev(a, "cuda")
    t = DC.tables_of(c, "cuda")
    groups = bonds.bond_groups(c.ei, c.shift, c.z, by="pair", onsite=True)
    K = DC.k_kernel(len(s.f))
    assert abs(float((s.w * s.occ).sum()) - s.nel) <= 1e-10
    for name, f, Xon, Xoff, want in (("S", s.f, c.Son, c.Soff, float(s.f.astype(np.float64).sum())),
                                     ("H", s.f, c.Hon, c.Hoff, float((s.f.astype(np.float64) * s.eps.reshape(-1)).sum())),
                                     ("S, f eps", s.fe, c.Son, c.Soff, float(s.fe.astype(np.float64).sum()))):
        P_on, P_off = density.density_rows(d(s.C), d(s.kidx), d(c.kvec), d(f), t)
        args = (P_on.double(), P_off.double(), d(Xon).double(), d(Xoff).double())
        total = float(density.bond_populations(*args, groups).sum())
        per_atom, per_orb = density.populations(*args, t)
        tol = DC.sum_rule_tolerance(c, s.C128, s.kidx, f, Xon, Xoff, K, want)
        print(f"rows={name} sum over members={total:.8f} populations={float(per_atom.sum()):.8f} want={want:.8f} err/tol={abs(total - want) / tol:.3f}")
        assert tuple(per_atom.shape) == (c.N,) and tuple(per_orb.shape) == (c.N, c.nao)
        assert abs(total - want) <= tol and abs(float(per_atom.sum()) - want) <= tol
        a32, _ = density.populations(P_on, P_off, d(Xon), d(Xoff), t)      # the fp32 sums the user gets: fixed order, bit-identical from call to call
        assert a32.dtype == torch.float32 and torch.equal(a32, density.populations(P_on, P_off, d(Xon), d(Xoff), t)[0])


def test_no_state_gives_zero_rows_and_accumulate_leaves_them():
    c = BC.case(13)
    out = (torch.full((c.N, 169), 7.0, device="cuda"), torch.full((c.E, 169), 7.0, device="cuda"))
    DC.run(c, "cuda", hi=0, out=out, accumulate=True)
    assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all())
    DC.run(c, "cuda", hi=0, out=out)
    assert not bool(out[0].any()) and not bool(out[1].any())


def test_arguments_are_checked_on_the_host():
    c = BC.case(13)
    t = DC.tables_of(c, "cuda")
    d = lambda a: DC.dev(a, "cuda")
    good = dict(C=d(c.C), kidx=d(c.kidx), kvec=d(c.kvec), f=d(DC.weights(c)), tables=t)
    on, off = density.density_rows(**good)
    assert tuple(on.shape) == (c.N, 169) and tuple(off.shape) == (c.E, 169)
    bad_idx = c.kidx.copy()
    bad_idx[5] = len(c.kvec)
    wide = d(np.concatenate([c.C, c.C], 1))
    for name, change in (("C", dict(C=d(c.C.astype(np.complex128)))), ("C", dict(C=wide[:, :c.M])), ("orbital columns", dict(C=d(c.C[:, :-1]))),
                         ("kidx", dict(kidx=d(bad_idx))), ("kidx", dict(kidx=d(-1 - c.kidx))), ("kidx", dict(kidx=d(c.kidx.astype(np.int64)))),
                         ("f", dict(f=d(DC.weights(c).astype(np.float64)))), ("f", dict(f=d(DC.weights(c)[:-1]))), ("f", dict(f=DC.dev(DC.weights(c), "cpu"))),
                         ("kvec", dict(kvec=d(c.kvec[:, :2]))), ("erow", dict(tables=dataclasses.replace(t, erow=t.erow + c.N))),
                         ("ecol", dict(tables=dataclasses.replace(t, ecol=t.ecol.long()))), ("orank", dict(tables=dataclasses.replace(t, ooff=t.ooff + 1))),
                         ("accumulate", dict(accumulate=True)), ("P_off", dict(out=(on, off[:-1]))), ("P_on", dict(out=(on.double(), off)))):
        with pytest.raises(ValueError, match=name):
            density.density_rows(**{**good, **change})
