"""Checks of hamgnn_amd/bonds.py and the kernel hg_bond_weights of csrc/spectra.hip, shared by tests/test_bonds_gpu.py (the HIP kernel) and
tests/test_bonds_cpu.py (host logic, the torch path, and the numpy twin below in place of the kernel).

The exact statement is `ref_bond_weights`: the formulas of bonds.py's docstring in complex128 numpy with a loop over the members of every group,
  t_e(s) = Re(exp(2 pi i k_s . shift_e) sum_{a, b} conj(C[s, mu(i, a)]) X_off[e][a, b] C[s, mu(j, b)]),  o_i(s) the same on X_on[i] without a phase,
  W[s, 0] = wk[s],  W[s, 1 + g] = wk[s] (sum of t_e over the edges of g + sum of o_i over its atoms),  pad columns 0,
on the compact orbital lists written out here from the head's basis_def (not through bond_tables).  The twin `bond_weights_np` follows the kernel's
structure in fp32: per member the masked nao x nao block times Re C_j and Im C_j, conj(C_i) . T summed per lane quarter (rows 4 q .. 4 q + 3 of every
16-row tile) and the quarters added as (q0 + q1) + (q2 + q3), the phase from double rounded once, members dealt to 4 waves in contiguous quarters and added
in order, ((w0 + w1) + w2) + w3, then wk; the order inside one matrix product is numpy's.

The bound, per element:  |W - W_ref| <= (K + 32) 2^-24 T,  T[s, g] = wk sum_members sum_{a, b} |c_a| |X_ab| |c_b| in fp64.
  The issue's K = 4 sum_{members} n_i n_j counts the real products of an element and holds for any order of summation (`k_products`: used for the torch path,
  whose einsum order is the library's).
  The kernel's chain is shorter and K is tightened for it (`k_kernel`).  A real product phase x c_i x X x c_j passes through at most d roundings on its way
  into W: n_j fused multiply-adds of the MFMA chain over b (the predicated zeros add nothing and round nothing), 2 per row of the lane's 4 ceil(nao / 16) rows
  (conj(c_i) T: two fmas each for the real and the imaginary sum), 2 shuffle additions, 3 for the phase (cos / sin rounded from double, one product, one fma),
  ceil(members / 4) additions of the wave's running sum, 3 of the waves' sums and 1 product with wk:  d = n_j + 8 ceil(nao / 16) + ceil(members / 4) + 9.
  The four real products of one (a, b) sum in magnitude to at most (|cos| + |sin|) |c_a| |X_ab| |c_b| <= sqrt(2) |c_a| |X_ab| |c_b|, so the error is below
  sqrt(2) d 2^-24 T to first order;  K = 2 (max n_j + 8 ceil(nao / 16) + ceil(members / 4)) with the issue's + 32 covers sqrt(2) (d) and the second order.
  The kernel is held to min(k_kernel, k_products).  Inputs are fp32 / complex64 on both sides (k . shift is formed in double from the same fp32 values), so
  they add nothing.  Where T = 0 (an empty group, a pad column) the result must be exactly 0.
Nothing here reads the reference tree."""
import types

import numpy as np
import torch

U = 2.0 ** -24
WAVES = 4
# elements of 5 / 13 / 13, 5 / 13 / 19, 5 / 13 / 27 and 5 / 21 / 34 orbitals: one, two, two and three row tiles of 16 (the kernel's three instantiations)
HEADS = {13: ("openmx", (1, 6, 8)), 19: ("openmx", (1, 14, 34)), 27: ("abacus", (1, 14, 22)), 40: ("abacus", (1, 13, 73))}
_FIX = {}


# ------------------------------------------------------------------------------------------------ fixtures
def head(nao):
    """the read-out head of the basis (its basis tables are all bonds.py reads)"""
    if ("head", nao) not in _FIX:
        from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
        _FIX["head", nao] = HamGNNPlusPlusOut("1x0e", "1x0e", nao_max=nao, ham_type=HEADS[nao][0], ham_only=True, calculate_sparsity=False)
    return _FIX["head", nao]


def compact(h, z):
    """(orbs [N] sorted orbital lists, off0 [N + 1] first compact index of every atom) from the head's basis_def"""
    orbs = [sorted(h.basis_def[int(Z)]) for Z in z]
    return orbs, np.concatenate([[0], np.cumsum([len(o) for o in orbs])]).astype(np.int64)


def case(nao, ns=33, n_atoms=3, seed=0):
    """one crystal of `n_atoms` atoms (at least two elements with different orbital counts: orank holds -1 entries, blocks are rectangular) with random
    seeded rows and eigenvector rows: a namespace of z, pos, cell, ei [2, E], shift int [E, 3] (some edge / inverse pairs moved out to +-30 cells), Xon, Xoff
    fp32, C complex64 [ns, M], kvec fp32 [2, 3] reduced, kidx (the two k-points interleave inside every 16-state tile), wk.  An atom without any edge is
    appended (an on-site block only)."""
    key = ("case", nao, ns, n_atoms, seed)
    if key in _FIX:
        return _FIX[key]
    from hamgnn_amd.data.synthetic import random_cell
    zs = HEADS[nao][1]
    for s2 in range(seed, seed + 50):                          # (a seed whose draw holds at least two elements, the largest among them)
        g = random_cell(n_atoms, zs, seed=s2, density=0.004)
        zz = g.z.numpy()
        if len(set(zz.tolist())) >= 2 and zs[-1] in zz:
            break
    rng = np.random.default_rng(1000 + 7 * nao + seed)
    ei, shift, inv = g.edge_index.numpy().copy(), g.cell_shift.numpy().copy(), g.inv_edge_idx.numpy()
    for e in rng.choice(ei.shape[1], size=min(6, ei.shape[1]), replace=False):
        d = rng.integers(-30, 31, size=3)
        d[rng.integers(0, 3)] = 30
        if inv[e] == e:
            continue
        shift[e], shift[inv[e]] = shift[e] + d, shift[inv[e]] - d
    z = np.concatenate([zz, [zs[0]]])                           # the last atom has no edge
    pos = np.concatenate([g.pos.numpy().astype(np.float64), [[1.0, 2.0, 3.0]]])
    h = head(nao)
    orbs, off0 = compact(h, z)
    M, N, E = int(off0[-1]), len(z), ei.shape[1]
    c = types.SimpleNamespace(nao=nao, z=z, pos=pos, cell=g.cell.numpy()[0].astype(np.float64), ei=ei, shift=shift, N=N, E=E, M=M, ns=ns,
                              Xon=rng.normal(size=(N, nao * nao)).astype(np.float32), Xoff=rng.normal(size=(E, nao * nao)).astype(np.float32),
                              C=(rng.normal(size=(ns, M)) + 1j * rng.normal(size=(ns, M))).astype(np.complex64),
                              kvec=rng.uniform(-0.5, 0.5, size=(2, 3)).astype(np.float32), kidx=(np.arange(ns) % 2).astype(np.int32),
                              wk=rng.uniform(0.1, 1.0, ns).astype(np.float32), orbs=orbs, off0=off0, head=h)
    _FIX[key] = c
    return c


def groupings(c):
    """{name: (eptr, eidx, aptr, aidx)}: the three `by` of bond_groups with on-site groups; "mixed": pairs within a radius that leaves edges in no group, no
    on-site groups but one atom group, an EMPTY group in the middle and one at the end; "single": one group of one edge; "none": G = 0"""
    key = ("groupings", id(c))
    if key in _FIX:
        return _FIX[key]
    from hamgnn_amd import bonds
    out = {by: bonds.bond_groups(c.ei, c.shift, c.z, by=by, onsite=True)[:4] for by in bonds.BY}
    length = np.linalg.norm(c.pos[c.ei[1]] + c.shift @ c.cell - c.pos[c.ei[0]], axis=1)
    eptr, eidx, aptr, aidx, _ = bonds.bond_groups(c.ei, c.shift, c.z, by="pair", onsite=False, pos=c.pos, cell=c.cell, rmax=float(np.median(length)))
    G, mid = len(eptr) - 1, (len(eptr) - 1) // 2
    assert 0 < len(eidx) < c.E and G >= 2
    eptr = np.concatenate([eptr[:mid + 1], eptr[mid:], eptr[-1:], eptr[-1:]]).astype(np.int32)      # + an empty group after `mid`, an atom group, an empty group
    aptr = np.concatenate([np.zeros(G + 2, dtype=np.int32), [2, 2]]).astype(np.int32)
    out["mixed"] = (eptr, eidx, aptr, np.array([c.N - 1, 0], dtype=np.int32))
    z1, i0 = np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    out["single"] = (np.array([0, 1], dtype=np.int32), np.array([c.E - 1], dtype=np.int32), np.zeros(2, dtype=np.int32), i0)
    out["none"] = (z1, i0, z1, i0)
    _FIX[key] = out
    return out


def row_atom_groups(c):
    """every directed edge grouped by its row atom, plus that atom's on-site block: the Mulliken population of the atom when the rows are the overlap's"""
    order = np.argsort(c.ei[0], kind="stable")
    eptr = np.concatenate([[0], np.cumsum(np.bincount(c.ei[0], minlength=c.N))]).astype(np.int32)
    return eptr, order.astype(np.int32), np.arange(c.N + 1, dtype=np.int32), np.arange(c.N, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the fp64 statement
def member_terms(c, Xon=None, Xoff=None):
    """per member, fp64: (t [E, ns], o [N, ns], Tt [E, ns], To [N, ns], nn_e [E], nn_a [N], nj_e [E], nj_a [N]): the terms of the docstring, their magnitude sums
    sum |c_a| |X_ab| |c_b|, and the products n_i n_j / the column counts n_j"""
    key = ("terms", id(c)) if Xon is None and Xoff is None else None       # (the case's own rows: computed once, shared by every grouping)
    if key in _FIX:
        return _FIX[key]
    Xon, Xoff = c.Xon if Xon is None else Xon, c.Xoff if Xoff is None else Xoff
    C = c.C.astype(np.complex128)
    k = c.kvec.astype(np.float64)[c.kidx]                      # [ns, 3]
    block = lambda rows, r, i, j: rows[r].astype(np.float64).reshape(c.nao, c.nao)[np.ix_(c.orbs[i], c.orbs[j])]
    cols = lambda i: C[:, c.off0[i]:c.off0[i + 1]]
    t, Tt = np.zeros((c.E, c.ns)), np.zeros((c.E, c.ns))
    for e in range(c.E):
        i, j = int(c.ei[0, e]), int(c.ei[1, e])
        X = block(Xoff, e, i, j)
        phase = np.exp(2j * np.pi * (k @ c.shift[e].astype(np.float32).astype(np.float64)))
        t[e] = (phase * np.einsum("sa,ab,sb->s", cols(i).conj(), X, cols(j))).real
        Tt[e] = np.einsum("sa,ab,sb->s", np.abs(cols(i)), np.abs(X), np.abs(cols(j)))
    o, To = np.zeros((c.N, c.ns)), np.zeros((c.N, c.ns))
    for i in range(c.N):
        X = block(Xon, i, i, i)
        o[i] = np.einsum("sa,ab,sb->s", cols(i).conj(), X, cols(i)).real
        To[i] = np.einsum("sa,ab,sb->s", np.abs(cols(i)), np.abs(X), np.abs(cols(i)))
    n = np.array([len(v) for v in c.orbs])
    out = (t, o, Tt, To, n[c.ei[0]] * n[c.ei[1]], n * n, n[c.ei[1]], n)
    if key is not None:
        _FIX[key] = out
    return out


def ref_bond_weights(c, groups, Gp, Xon=None, Xoff=None):
    """(W_ref [ns, Gp], T [ns, Gp], k_products [Gp], k_kernel [Gp]) in fp64: a loop over the groups and over their members, in the lists' order"""
    eptr, eidx, aptr, aidx = groups[:4]
    t, o, Tt, To, nn_e, nn_a, nj_e, nj_a = member_terms(c, Xon, Xoff)
    G = len(eptr) - 1
    wk = c.wk.astype(np.float64)
    W, T = np.zeros((c.ns, Gp)), np.zeros((c.ns, Gp))
    kp, kk = np.zeros(Gp), np.zeros(Gp)
    W[:, 0] = wk
    for g in range(G):
        acc, mag, prod, njmax, nm = np.zeros(c.ns), np.zeros(c.ns), 0, 0, 0
        for e in eidx[eptr[g]:eptr[g + 1]]:
            acc, mag, prod, njmax, nm = acc + t[e], mag + Tt[e], prod + int(nn_e[e]), max(njmax, int(nj_e[e])), nm + 1
        for i in aidx[aptr[g]:aptr[g + 1]]:
            acc, mag, prod, njmax, nm = acc + o[i], mag + To[i], prod + int(nn_a[i]), max(njmax, int(nj_a[i])), nm + 1
        W[:, 1 + g], T[:, 1 + g] = wk * acc, wk * mag
        kp[1 + g], kk[1 + g] = 4 * prod, 2 * (njmax + 8 * -(-c.nao // 16) + -(-nm // WAVES))
    return W, T, kp, kk


def bound(T, K):
    return (np.asarray(K)[None, :] + 32) * U * T


def ratio(W, ref, bnd):
    """the largest err / bound; where the bound is 0 (pad columns, empty groups) the result must be exactly 0"""
    W = np.asarray(W, dtype=np.float64)
    assert W.shape == ref.shape and np.isfinite(W).all()
    err = np.abs(W - ref)
    assert not err[bnd == 0].any(), float(err[bnd == 0].max(initial=0.0))
    return float((err[bnd > 0] / bnd[bnd > 0]).max(initial=0.0))


def check_weights(W, c, groups, Gp, ns=None, kernel=True, Xon=None, Xoff=None):
    """W [ns, Gp] of the first ns states of the case against the fp64 statement: inside the bound element-wise and finite, column 0 = wk exactly, pad columns
    and empty groups exactly 0 -> the largest err / bound"""
    ns = c.ns if ns is None else ns
    ref, T, kp, kk = ref_bond_weights(c, groups, Gp, Xon, Xoff)
    W = np.asarray(W)
    G = len(groups[0]) - 1
    assert W.shape == (ns, Gp) and W.dtype == np.float32 and np.isfinite(W).all()
    assert np.array_equal(W[:, 0], c.wk[:ns]) and not W[:, 1 + G:].any()
    empty = [g for g in range(G) if groups[0][g] == groups[0][g + 1] and groups[2][g] == groups[2][g + 1]]
    assert not W[:, [1 + g for g in empty]].any()
    bnd = bound(T[:ns], np.minimum(kk, kp) if kernel else kp)
    bnd[:, 0] = 0.0
    r = ratio(W, ref[:ns], bnd)
    print(f"nao={c.nao} ns={ns} G={G} Gp={Gp} kernel={kernel} err/bound={r:.3f}")
    return r


# ------------------------------------------------------------------------------------------------ the numpy twin of the kernel
def bond_weights_np(C, kidx, kvec, Xon, Xoff, erow, ecol, shift, orank, ooff, eptr, eidx, aptr, aidx, wk, Gp):
    C = np.asarray(C, dtype=np.complex64)
    ns, M = C.shape
    N, nao = orank.shape
    G = len(eptr) - 1
    nt = -(-nao // 16)
    pad = lambda a: np.concatenate([a, np.zeros((ns, 16 * nt - nao), dtype=np.float32)], 1)
    have = orank >= 0
    comp = np.where(have, ooff[:, None] + orank, M)
    CA = np.concatenate([C, np.zeros((ns, 1), dtype=np.complex64)], 1)[:, comp]                      # [ns, N, nao], 0 where the atom lacks the orbital
    k = np.asarray(kvec, dtype=np.float64)[np.asarray(kidx, dtype=np.int64)]
    W = np.zeros((ns, Gp), dtype=np.float32)
    wk = np.asarray(wk, dtype=np.float32)
    W[:, 0] = wk

    def member(X, i, j, e):
        Xm = np.where(have[i][:, None] & have[j][None, :], np.asarray(X, dtype=np.float32).reshape(nao, nao), np.float32(0))
        tr, ti = CA[:, j].real @ Xm.T, CA[:, j].imag @ Xm.T                                           # [ns, nao]: T = X c_j
        ci = CA[:, i]
        lanes = lambda v: pad(v).reshape(ns, nt, 4, 4).transpose(0, 2, 1, 3).reshape(ns, 4, 4 * nt).sum(-1, dtype=np.float32)   # [ns, quarter]
        quarters = lambda q: (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
        pr = quarters(lanes(ci.real * tr) + lanes(ci.imag * ti))
        pi = quarters(lanes(ci.real * ti) - lanes(ci.imag * tr))
        if e is None:
            return pr
        ph = 6.283185307179586 * (k @ np.asarray(shift[e], dtype=np.float32).astype(np.float64))
        return np.cos(ph).astype(np.float32) * pr - np.sin(ph).astype(np.float32) * pi

    for g in range(G):
        mem = [(Xoff[e], int(erow[e]), int(ecol[e]), int(e)) for e in eidx[eptr[g]:eptr[g + 1]]] + \
              [(Xon[i], int(i), int(i), None) for i in aidx[aptr[g]:aptr[g + 1]]]
        chunk = -(-len(mem) // WAVES)
        total = None
        for w in range(WAVES):
            s = np.zeros(ns, dtype=np.float32)
            for m in mem[w * chunk:(w + 1) * chunk]:
                s = s + member(*m)
            total = s if total is None else total + s           # ((w0 + w1) + w2) + w3
        W[:, 1 + g] = wk * total
    return W


def bond_weights_cpu(C, kidx, kvec, X_on, X_off, erow, ecol, shift, orank, ooff, eptr, eidx, aptr, aidx, wk, Gp):
    n = lambda t: t.numpy()
    return torch.from_numpy(bond_weights_np(n(C), n(kidx), n(kvec), n(X_on), n(X_off), n(erow), n(ecol), n(shift), n(orank), n(ooff), n(eptr), n(eidx),
                                            n(aptr), n(aidx), n(wk), Gp))


def install_cpu(monkeypatch):
    """the numpy twin in place of the HIP wrapper; bonds.bond_weights then takes its kernel route on CPU tensors"""
    from hamgnn_amd import dos, ops
    monkeypatch.setattr(ops, "bond_weights", bond_weights_cpu)
    monkeypatch.setattr(dos, "_use_kernels", lambda t: True)


# ------------------------------------------------------------------------------------------------ running bonds.bond_weights on a case
def run(c, groups, Gp, device, ns=None, Xon=None, Xoff=None, C=None, rows=None):
    """bonds.bond_weights on the first ns states of the case (or on the slice `rows` of them), through bond_tables -> W as numpy"""
    from hamgnn_amd import bonds
    rows = slice(0, c.ns if ns is None else ns) if rows is None else rows
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tables = bonds.bond_tables(c.head, c.z, c.ei, c.shift, device)
    assert tables.M == c.M
    W = bonds.bond_weights(dev((c.C if C is None else C)[rows]), dev(c.kidx[rows]), dev(c.kvec), dev(c.Xon if Xon is None else Xon),
                           dev(c.Xoff if Xoff is None else Xoff), tables, groups, dev(c.wk[rows]), Gp)
    return W.cpu().numpy()


def solvable_case(seed=0):
    """a 2-atom cell (H and C of the 13-orbital OpenMX basis: 5 + 13 orbitals) on the 2 x 2 x 2 grid with Hermitian-consistent random Hamiltonian rows
    (data.synthetic.add_random_targets) and overlap rows = 1 on the site diagonals + small Hermitian-consistent noise, positive definite at every k-point
    (checked in fp64).  C, kidx, wk, ns are filled by the test that solves it.  The rows are random in ALL nao^2 positions, the orbitals an atom lacks too."""
    key = ("solvable", seed)
    if key in _FIX:
        return _FIX[key]
    from hamgnn_amd import dos
    from hamgnn_amd.data.synthetic import add_random_targets, random_cell
    nao = 13
    for s2 in range(seed, seed + 50):
        g = random_cell(2, (1, 6), seed=s2, density=0.004)
        if len(set(g.z.tolist())) == 2:
            break
    add_random_targets(g, nao, seed=seed)
    rng = np.random.default_rng(77 + seed)
    N, E = g.num_nodes, g.num_edges
    inv = g.inv_edge_idx.numpy()
    A = rng.normal(0, 0.3 / (nao * max(1, E // N)), size=(E, nao, nao)).astype(np.float32)
    Soff = (0.5 * (A + A[inv].transpose(0, 2, 1))).reshape(E, nao * nao)
    B = rng.normal(0, 0.02, size=(N, nao, nao)).astype(np.float32)
    Son = (np.eye(nao, dtype=np.float32)[None] + 0.5 * (B + B.transpose(0, 2, 1))).reshape(N, nao * nao)
    z = g.z.numpy()
    h = head(nao)
    orbs, off0 = compact(h, z)
    k_red, k_w = dos.monkhorst_pack((2, 2, 2))
    cell = g.cell.numpy()[0].astype(np.float64)
    c = types.SimpleNamespace(nao=nao, z=z, pos=g.pos.numpy().astype(np.float64), cell=cell, ei=g.edge_index.numpy(), shift=g.cell_shift.numpy(), N=N, E=E,
                              M=int(off0[-1]), Hon=g["Hon"].numpy(), Hoff=g["Hoff"].numpy(), Son=Son, Soff=Soff, Xon=None, Xoff=None,
                              kvec=k_red.astype(np.float32), k_w=k_w, tet=dos.tetrahedra((2, 2, 2), cell), orbs=orbs, off0=off0, head=h)
    assert len(k_w) == 8 and np.array_equal(c.kvec.astype(np.float64), k_red)
    smin = min(float(np.linalg.eigvalsh(dense_xk(c, Son, Soff, k)).min()) for k in k_red)
    assert smin > 0.3, smin
    _FIX[key] = c
    return c


def solve_host(Hk, Sk):
    """(eps [nk, M] ascending, C [nk, band, M] with c^+ S c = 1) in complex128 numpy from the dense matrices: Cholesky factor of S(k), eigh of L^-1 H L^-H"""
    eps, Cs = [], []
    for H, S in zip(np.asarray(Hk, dtype=np.complex128), np.asarray(Sk, dtype=np.complex128)):
        H, S = 0.5 * (H + H.conj().T), 0.5 * (S + S.conj().T)
        Li = np.linalg.inv(np.linalg.cholesky(S))
        ev, y = np.linalg.eigh(Li @ H @ Li.conj().T)
        eps.append(ev)
        Cs.append((Li.conj().T @ y).T)
    return np.asarray(eps), np.asarray(Cs)


def dense_xk(c, Xon, Xoff, k):
    """X(k) [M, M] complex128 at the reduced k-point k: the assembly restated densely (on-site blocks on the diagonal, phase x block per directed edge)"""
    X = np.zeros((c.M, c.M), dtype=np.complex128)
    sl = lambda i: slice(int(c.off0[i]), int(c.off0[i + 1]))
    for i in range(c.N):
        X[sl(i), sl(i)] += Xon[i].astype(np.float64).reshape(c.nao, c.nao)[np.ix_(c.orbs[i], c.orbs[i])]
    for e in range(c.E):
        i, j = int(c.ei[0, e]), int(c.ei[1, e])
        X[sl(i), sl(j)] += np.exp(2j * np.pi * float(np.asarray(k, dtype=np.float64) @ c.shift[e])) * \
            Xoff[e].astype(np.float64).reshape(c.nao, c.nao)[np.ix_(c.orbs[i], c.orbs[j])]
    return X
