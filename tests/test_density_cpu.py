"""hamgnn_amd/density.py without a GPU: the torch path and the numpy twin of hg_density_rows (tests/density_checks.py) against the fp64 statement, the
occupations against dos.fermi_level, populations / bond_populations against loops, and the Hellmann-Feynman convention against the adjoint of the assembly."""
import dataclasses
import types

import numpy as np
import pytest
import torch

from hamgnn_amd import bonds, density, dos
from tests import bond_checks as BC
from tests import density_checks as DC

NAOS = sorted(BC.HEADS)


@pytest.mark.parametrize("ns", DC.NS)
@pytest.mark.parametrize("nao", NAOS)
def test_torch_path_within_the_bound(nao, ns):
    c = BC.case(nao)
    assert DC.check_rows(DC.run(c, "cpu", hi=ns), DC.ref_case(c, 0, ns), DC.k_products(ns), f"torch nao={nao} ns={ns}") <= 1.0


@pytest.mark.parametrize("ns", DC.NS)
@pytest.mark.parametrize("nao", NAOS)
def test_twin_within_the_kernel_bound(nao, ns, monkeypatch):
    """the numpy twin installed in place of ops.density_rows: density.density_rows takes its kernel route"""
    DC.install_cpu(monkeypatch)
    c = BC.case(nao)
    assert DC.check_rows(DC.run(c, "cpu", hi=ns), DC.ref_case(c, 0, ns), DC.k_kernel(ns), f"twin nao={nao} ns={ns}") <= 1.0


@pytest.mark.parametrize("route", ["torch", "twin"])
def test_accumulate_adds_state_chunks_and_leaves_missing_orbitals_alone(route, monkeypatch):
    if route == "twin":
        DC.install_cpu(monkeypatch)
    c = BC.case(19)
    K = DC.k_products if route == "torch" else DC.k_kernel
    t = DC.tables_of(c, "cpu")
    have = t.orank.numpy() >= 0
    miss_on = ~(have[:, :, None] & have[:, None, :]).reshape(c.N, -1)
    miss_off = ~(have[c.ei[0]][:, :, None] & have[c.ei[1]][:, None, :]).reshape(c.E, -1)
    out = (torch.full((c.N, c.nao ** 2), 7.0), torch.full((c.E, c.nao ** 2), 7.0))
    DC.run(c, "cpu", hi=17, out=out)                             # accumulate = False into a given out: every element written
    assert not out[0].numpy()[miss_on].any() and not out[1].numpy()[miss_off].any()
    out[0][torch.from_numpy(miss_on)] = 7.0
    DC.run(c, "cpu", lo=17, out=out, accumulate=True)
    assert (out[0].numpy()[miss_on] == 7.0).all()               # accumulate: elements at missing orbitals stay as they are
    out[0][torch.from_numpy(miss_on)] = 0.0
    ref, r1, r2 = DC.ref_case(c, 0, c.ns), DC.ref_case(c, 0, 17), DC.ref_case(c, 17, c.ns)
    for got, want, Ta, Tb in ((out[0], ref[0], r1[2], r2[2]), (out[1], ref[1], r1[3], r2[3])):
        assert DC.ratio(got.numpy(), want, DC.bound(Ta, K(17)) + DC.bound(Tb, K(c.ns - 17))) <= 1.0


def test_no_state_gives_zero_rows():
    c = BC.case(13)
    on, off = DC.run(c, "cpu", hi=0)
    assert on.shape == (c.N, 169) and off.shape == (c.E, 169) and not on.any() and not off.any()


def test_occupations_are_the_count_fermi_level_bisects_on():
    s = DC.solved_case()
    assert s.occ.dtype == np.float64 and s.occ.shape == s.eps.shape and (s.occ >= 0).all() and (s.occ <= 2).all()
    assert abs(float((s.w * s.occ).sum()) - s.nel) <= 1e-10
    t = density.occupations(torch.from_numpy(s.eps), s.mu, s.sigma)
    assert t.dtype == torch.float64 and np.array_equal(t.numpy(), s.occ)
    assert np.array_equal(density.occupations(s.eps, s.mu, s.sigma, deg=1), 0.5 * s.occ)


@pytest.mark.parametrize("nao", [13, 27])
def test_populations_against_loops(nao):
    c = BC.case(nao)
    rng = np.random.default_rng(3)
    Pon, Poff = rng.normal(size=c.Xon.shape), rng.normal(size=c.Xoff.shape)
    t = DC.tables_of(c, "cpu")
    per_atom, per_orb = density.populations(*(torch.from_numpy(a) for a in (Pon, Poff, c.Xon.astype(np.float64), c.Xoff.astype(np.float64))), t)
    want = np.zeros((c.N, nao))
    for i in range(c.N):
        want[i] += (Pon[i] * c.Xon[i]).reshape(nao, nao).sum(1)
    for e in range(c.E):
        want[c.ei[0, e]] += (Poff[e] * c.Xoff[e]).reshape(nao, nao).sum(1)
    assert np.abs(per_orb.numpy() - want).max() <= 1e-12 * np.abs(want).max() and np.abs(per_atom.numpy() - want.sum(1)).max() <= 1e-12 * np.abs(want).max()
    with pytest.raises(ValueError, match="populations"):
        density.populations(torch.from_numpy(Pon), torch.from_numpy(Poff[:-1]), torch.from_numpy(c.Xon), torch.from_numpy(c.Xoff), t)
    for name, groups in BC.groupings(c).items():
        got = density.bond_populations(*(torch.from_numpy(a) for a in (Pon, Poff, c.Xon.astype(np.float64), c.Xoff.astype(np.float64))), groups).numpy()
        eptr, eidx, aptr, aidx = groups
        loop = np.array([sum(float((Poff[e] * c.Xoff[e]).sum()) for e in eidx[eptr[g]:eptr[g + 1]]) + sum(float((Pon[i] * c.Xon[i]).sum()) for i in aidx[aptr[g]:aptr[g + 1]])
                         for g in range(len(eptr) - 1)])
        assert got.shape == loop.shape and np.abs(got - loop).max(initial=0.0) <= 1e-11 * max(1.0, np.abs(loop).max(initial=0.0)), name


@pytest.mark.parametrize("nao", NAOS)
def test_rows_are_the_adjoint_of_the_assembly_in_double(nao):
    """the Hellmann-Feynman convention: (P_on, P_off) = kspace.assemble_k_adjoint(G) for G_k[p, q] = sum_{s at k} f_s C[s, p] conj(C[s, q]), in complex128 on
    the torch paths of both"""
    from hamgnn_amd import kspace
    c = BC.case(nao)
    C, f = torch.from_numpy(c.C.astype(np.complex128)), torch.from_numpy(DC.weights(c).astype(np.float64))
    t = DC.tables_of(c, "cpu")
    kv = torch.from_numpy(c.kvec.astype(np.float64))
    got = density._density_rows_torch(C, torch.from_numpy(c.kidx), kv, f, t.erow, t.ecol, t.shift.double(), t.orank, t.ooff)
    G = torch.stack([torch.einsum("s,sp,sq->pq", f[c.kidx == k].to(C.dtype), C[c.kidx == k], C[c.kidx == k].conj()) for k in range(len(c.kvec))])
    want = kspace._assemble_k_adjoint_torch(G, t, kv)
    ref = DC.ref_case(c, 0, c.ns)
    for a, b, r, T in zip(got, want, ref[:2], ref[2:]):
        assert a.dtype == torch.float64 and tuple(a.shape) == tuple(b.shape)
        assert float((a - b).abs().max()) <= 1e-12 * T.max() and np.abs(a.numpy() - r).max() <= 1e-12 * T.max()


def test_defining_identities_on_the_solved_crystal_fp64():
    """the fp64 statement on host-solved eigenpairs: sum over all members of P . S = sum f and of P . H = sum f eps (to 1e-10), and
    sum_ab X_off[e] P_off[e] = sum_s f_s t_e(s) with t_e of bonds.py"""
    s = DC.solved_case()
    c = s.c
    f = (s.w * s.occ).reshape(-1)
    Pon, Poff, _, _ = DC.ref_density_rows(c, s.C128, s.kidx, f)
    d = lambda a: a.astype(np.float64)
    assert abs((Pon * d(c.Son)).sum() + (Poff * d(c.Soff)).sum() - f.sum()) <= 1e-10 * abs(f.sum())
    want = (f * s.eps.reshape(-1)).sum()
    assert abs((Pon * d(c.Hon)).sum() + (Poff * d(c.Hoff)).sum() - want) <= 1e-10 * max(1.0, abs(want))
    c2 = types.SimpleNamespace(**{**vars(c), "C": s.C128, "kidx": s.kidx, "ns": len(f), "wk": np.ones(len(f)), "Xon": c.Hon, "Xoff": c.Hoff})
    t, o = BC.member_terms(c2, c.Hon, c.Hoff)[:2]
    assert np.abs((Poff * d(c.Hoff)).sum(1) - t @ f).max() <= 1e-10 and np.abs((Pon * d(c.Hon)).sum(1) - o @ f).max() <= 1e-10


def test_arguments_are_checked_on_the_host():
    c = BC.case(13)
    t = DC.tables_of(c, "cpu")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    good = dict(C=d(c.C), kidx=d(c.kidx), kvec=d(c.kvec), f=d(DC.weights(c)), tables=t)
    on, off = density.density_rows(**good)
    assert tuple(on.shape) == (c.N, 169) and tuple(off.shape) == (c.E, 169)
    bad_idx = c.kidx.copy()
    bad_idx[5] = len(c.kvec)
    bad_row = dataclasses.replace(t, erow=t.erow + c.N)
    for name, change in (("C", dict(C=d(c.C.astype(np.complex128)))), ("orbital columns", dict(C=d(c.C[:, :-1]))), ("kidx", dict(kidx=d(bad_idx))),
                         ("kidx", dict(kidx=d(-1 - c.kidx))), ("kidx", dict(kidx=d(c.kidx.astype(np.int64)))), ("f", dict(f=d(DC.weights(c).astype(np.float64)))),
                         ("f", dict(f=d(DC.weights(c)[:-1]))), ("kvec", dict(kvec=d(c.kvec[:, :2]))), ("erow", dict(tables=bad_row)),
                         ("accumulate", dict(accumulate=True)), ("P_off", dict(out=(on, off[:-1]))), ("P_on", dict(out=(on.double(), off)))):
        with pytest.raises(ValueError, match=name):
            density.density_rows(**{**good, **change})


def test_library_exports_the_entry_point_and_needs_no_scratch():
    import ctypes as C
    from hamgnn_amd import _lib
    L = _lib.lib()
    assert "hg_density_rows" in _lib.EXPORTS and hasattr(L, "hg_density_rows")
    L.hg_scratch_bytes.restype, L.hg_scratch_bytes.argtypes = C.c_int64, [C.c_char_p, C.c_int64, C.c_int]
    assert L.hg_scratch_bytes(b"hg_density_rows", 1000, 0) == 0
    call = _lib.call                                            # NULL tensors only: none of these reaches a launch
    sizes = dict(ns=5, M=4, nk=1, n_edges=0, n_atoms=1, nao=13)
    run = lambda **kw: call("hg_density_rows", None, {**sizes, **kw}["ns"], {**sizes, **kw}["M"], None, None, {**sizes, **kw}["nk"], None, None, None, None,
                            {**sizes, **kw}["n_edges"], {**sizes, **kw}["n_atoms"], {**sizes, **kw}["nao"], None, None, 0, None, None)
    for bad in (dict(nao=49), dict(nao=0), dict(M=0), dict(nk=0), dict(n_atoms=0), dict(n_edges=-1), dict(n_edges=2 ** 31), dict()):      # the last: good sizes, NULL tensors
        with pytest.raises(RuntimeError, match="hg_density_rows"):
            run(**bad)
