"""hg_bond_weights (csrc/spectra.hip) on the GPU through hamgnn_amd/bonds.py: against the fp64 statement inside the derived bound of tests/bond_checks.py,
its structure (every element written, bit-reproducible, rows independent of the launch), against the Mulliken kernel, the argument checks, and the chain
into dos.tetra_states on the eigenpairs of a small crystal solved on the host."""

import numpy as np
import pytest
import torch

from hamgnn_amd import bonds, dos
from tests import bond_checks as BC

pytestmark = pytest.mark.gpu
NAOS = sorted(BC.HEADS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _gps(G):
    return sorted({1 + G, dos.padded_groups(G)})               # without and with pad columns


@pytest.mark.parametrize("ns", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("nao", NAOS)
def test_kernel_vs_fp64(nao, ns):
    """nao 13 / 19 / 27: orbital counts below 16, between 16 and 32, off the 4-wide steps; ns: one state, the tile's tail, one tile, a second tile's first state,
    three tiles; two k-points interleave inside every tile; groups of one member, of many (pairs over several images), of none, G = 0, edges in no group"""
    c = BC.case(nao)
    for name, groups in BC.groupings(c).items():
        G = len(groups[0]) - 1
        for Gp in _gps(G):
            assert BC.check_weights(BC.run(c, groups, Gp, "cuda", ns=ns), c, groups, Gp, ns=ns, kernel=True) <= 1.0, (name, Gp)


@pytest.mark.parametrize("nao", NAOS)
def test_launches_are_bit_identical_and_rows_do_not_depend_on_the_launch(nao):
    c = BC.case(nao)
    for name, groups in BC.groupings(c).items():
        Gp = dos.padded_groups(len(groups[0]) - 1)
        W1, W2 = BC.run(c, groups, Gp, "cuda"), BC.run(c, groups, Gp, "cuda")
        assert float(np.abs(W1 - W2).max()) == 0.0, name
        halves = np.concatenate([BC.run(c, groups, Gp, "cuda", rows=slice(0, 17)), BC.run(c, groups, Gp, "cuda", rows=slice(17, c.ns))])
        assert float(np.abs(W1 - halves).max()) == 0.0, name      # (the second half starts in the middle of a tile of the whole launch)


@pytest.mark.parametrize("nao", NAOS)
def test_row_atom_groups_agree_with_the_mulliken_kernel(nao):
    """HIP vs HIP: every directed edge grouped by its row atom + the atom's on-site block is the atom's Mulliken population, ops.mulliken_weights(C, S(k) C) with
    S(k) from kspace.assemble_k and S(k) C from one bmm: within the sum of the two kernels' bounds (the Mulliken kernel's: (m_g + 4) 2^-24 wk sum |terms|,
    tests/dos_checks.py, on the S(k) C rows the device formed)"""
    from hamgnn_amd import kspace, ops
    c = BC.case(nao)
    ns = 32                                                     # 16 states per k-point: one rectangular bmm
    groups = BC.row_atom_groups(c)
    Gp = dos.padded_groups(c.N)
    Wb = BC.run(c, groups, Gp, "cuda", ns=ns)
    ref, T, kp, kk = BC.ref_bond_weights(c, groups, Gp)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tables = bonds.bond_tables(c.head, c.z, c.ei, c.shift, "cuda")
    Sk, M = kspace.assemble_k(dev(c.Xon), dev(c.Xoff), tables, dev(c.kvec)), tables.M
    assert M == c.M
    Cd = dev(c.C[:ns])
    Ck = Cd.reshape(ns // 2, 2, M).transpose(0, 1)              # [k, state, M]: the states interleave the two k-points
    SC = torch.bmm(Sk, Ck.transpose(1, 2)).transpose(1, 2).transpose(0, 1).reshape(ns, M).contiguous()
    perm, gptr, _ = dos.group_map(c.head, c.z, "atom")
    Wm = ops.mulliken_weights(Cd, SC, dev(perm), dev(gptr), dev(c.wk[:ns]), Gp).cpu().numpy().astype(np.float64)
    SCh = SC.cpu().numpy()
    terms = np.abs(c.C[:ns].real.astype(np.float64) * SCh.real) + np.abs(c.C[:ns].imag.astype(np.float64) * SCh.imag)
    worst = 0.0
    for g in range(c.N):
        mu = perm[gptr[g]:gptr[g + 1]]
        bnd = BC.bound(T[:ns], np.minimum(kk, kp))[:, 1 + g] + (len(mu) + 4) * BC.U * c.wk[:ns] * terms[:, mu].sum(1)
        worst = max(worst, float((np.abs(Wb[:, 1 + g] - Wm[:, 1 + g]) / bnd).max()))
    print(f"nao={nao} bond kernel vs Mulliken kernel err/bound={worst:.3f}")
    assert np.array_equal(Wb[:, 0], Wm[:, 0].astype(np.float32)) and worst <= 1.0


def test_arguments_are_checked_on_the_host():
    c = BC.case(13)
    groups = BC.groupings(c)["pair"]
    G = len(groups[0]) - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tables = bonds.bond_tables(c.head, c.z, c.ei, c.shift, "cuda")
    good = dict(C=dev(c.C), kidx=dev(c.kidx), kvec=dev(c.kvec), X_on=dev(c.Xon), X_off=dev(c.Xoff), tables=tables, groups=groups, wk=dev(c.wk), Gp=1 + G)
    assert tuple(bonds.bond_weights(**good).shape) == (c.ns, 1 + G)
    wide = dev(np.concatenate([c.C, c.C], 1))
    bad_idx = c.kidx.copy()
    bad_idx[5] = len(c.kvec)
    for name, change in (("C", dict(C=dev(c.C.astype(np.complex128)))), ("C", dict(C=wide[:, :c.M])), ("Gp", dict(Gp=G)), ("kidx", dict(kidx=dev(bad_idx))),
                         ("kidx", dict(kidx=dev(-1 - c.kidx))), ("kidx", dict(kidx=dev(c.kidx.astype(np.int64)))), ("X_off", dict(X_off=dev(c.Xoff.astype(np.float64)))),
                         ("wk", dict(wk=dev(c.wk[:-1]))), ("eidx", dict(groups=(groups[0], groups[1] + c.E, groups[2], groups[3]))),
                         ("eptr", dict(groups=(groups[0][::-1].copy(), groups[1], groups[2], groups[3])))):
        with pytest.raises(ValueError, match=name):
            bonds.bond_weights(**{**good, **change})


@pytest.mark.parametrize("rows", ["H", "S"])
def test_chain_into_tetra_states_on_host_solved_eigenpairs(rows):
    """2 atoms, nao 13, 2 x 2 x 2: H(k), S(k) from kspace.assemble_k read back, solved in fp64 numpy; eps and C -> bond_weights (by="pair", onsite) ->
    dos.tetra_states at an energy above the spectrum.  The sum over the group columns is sum_k w_k sum_b eps_kb with Hamiltonian rows and the number of bands
    with overlap rows, within tetra_states' bound (tests/dos_tetra_checks.py) on the weights the device formed + the weights' bound carried through the sum.
    The weights' bound is the issue's K = 4 sum n_i n_j here: what it has over the kernel's chain (asserted below: at least members + 3) covers the rounding
    of C to complex64 (2 x 2^-24 T) and of the assembled H(k) the host solved ((members + 1) 2^-24 T), which the eigenvalues carry and the rows do not."""
    from hamgnn_amd import kspace
    from tests import dos_tetra_checks as TC
    c = BC.solvable_case()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tables = bonds.bond_tables(c.head, c.z, c.ei, c.shift, "cuda")
    asm = lambda on, off: kspace.assemble_k(dev(on), dev(off), tables, dev(c.kvec)).cpu().numpy()
    eps, C = BC.solve_host(asm(c.Hon, c.Hoff), asm(c.Son, c.Soff))
    nk, nb = eps.shape
    assert (nk, nb) == (8, c.M) and np.abs(np.einsum("kbm,kbm->kb", C.conj(), C @ BC.dense_xk(c, c.Son, c.Soff, c.kvec[0]).T)[0] - 1.0).max() < 1e-5
    c.C, c.ns = C.reshape(nk * nb, c.M).astype(np.complex64), nk * nb
    c.kidx, c.wk = np.repeat(np.arange(nk), nb).astype(np.int32), np.ones(nk * nb, dtype=np.float32)
    Xon, Xoff = (c.Hon, c.Hoff) if rows == "H" else (c.Son, c.Soff)
    eptr, eidx, aptr, aidx, labels = bonds.bond_groups(c.ei, c.shift, c.z, by="pair", onsite=True)
    G, Gp = len(labels), dos.padded_groups(len(labels))
    W = BC.run(c, (eptr, eidx, aptr, aidx), Gp, "cuda", Xon=Xon, Xoff=Xoff)
    _, T, kp, kk = BC.ref_bond_weights(c, (eptr, eidx, aptr, aidx), Gp, Xon, Xoff)
    members = np.concatenate([[0], np.diff(eptr) + np.diff(aptr), np.zeros(Gp - 1 - G)])
    assert ((kp - kk)[1:1 + G] >= members[1:1 + G] + 3).all()
    e32 = eps.astype(np.float32)
    E0 = float(e32.max()) + 1.0
    Nst = dos.tetra_states(dev(e32), dev(W).reshape(nk, nb, Gp), c.tet, E0, 1.0, 2).cpu().numpy().astype(np.float64)
    ref, bnd, _ = TC.ref_tetra(e32, W.reshape(nk, nb, Gp), c.tet, E0, 1.0, 2, 1)
    assert abs(ref[0, 0] - nb) < 1e-9 * nb                      # above the spectrum every state counts with its k-weight 1 / nk
    carried = (BC.bound(T, kp) / nk).sum(0)                     # sum_{k, b} A bound_W, A = 1 / nk above the spectrum
    want = float((c.k_w[:, None] * (eps if rows == "H" else np.ones_like(eps))).sum())
    err, tol = abs(Nst[0, 1:1 + G].sum() - want), float(bnd[0, 1:1 + G].sum() + carried[1:1 + G].sum()) + 1e-10 * abs(want)
    print(f"rows={rows} sum over bonds={Nst[0, 1:1 + G].sum():.6f} want={want:.6f} err/bound={err / tol:.3f}")
    assert not Nst[:, 1 + G:].any() and err <= tol
