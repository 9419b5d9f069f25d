"""Checks of hamgnn_amd/density.py and the kernel hg_density_rows of csrc/spectra.hip, shared by tests/test_density_gpu.py (the HIP kernel) and
tests/test_density_cpu.py (host logic, the torch path, and the numpy twin below in place of the kernel).  The crystals are those of tests/bond_checks.py.

The exact statement is `ref_density_rows`: the formulas of density.py's docstring in complex128 numpy, member by member,
  P_off[e][a, b] = sum_s f_s Re(exp(2 pi i k_s . shift_e) conj(C[s, mu(i, a)]) C[s, mu(j, b)]),  P_on[i][a, b] the same with j = i and no phase,
on the compact orbital lists written out from the head's basis_def (bond_checks.compact, not through bond_tables), 0 where an atom lacks the orbital.
The twin `density_rows_np` follows the kernel's structure in fp32: the row operand scaled by f, the column operand rotated by the phase (cos / sin from
double, rounded once), the 4-state steps dealt to 4 waves in contiguous quarters, one product over each wave's states, the partial blocks added as
((w0 + w1) + w2) + w3, the scatter from the compact ranks to the nao layout, and the accumulate addition; the order inside one matrix product is numpy's.

The bound, per element:  |P - P_ref| <= (K + 32) 2^-24 T,  T[a, b] = sum_s |f_s| |c_a| |c_b| in fp64.
  K_products = 6 ns holds for any order of summation: an element has 4 ns real products (f x_a cos x_b, f x_a sin y_b, f y_a sin x_b, f y_a cos y_b per
  state) whose magnitudes sum to at most |f| (|x_a| + |y_a|) |c_b| <= sqrt(2) |f| |c_a| |c_b| per state (Cauchy-Schwarz on (|cos|, |sin|) . (|x_b|, |y_b|)),
  and n additions of such terms err by at most n 2^-24 times that sum: sqrt(2) 4 ns < 6 ns.  The torch path is held to it (`k_products`).
  The kernel's chain is shorter (`k_kernel`).  One real product passes, on its way into P, at most d roundings: 1 of the operand scaling f x; 3 of the rotation
  (cos or sin rounded from double, one product, one fused multiply-add); 2 n_w of the MFMA chain over the wave's states, n_w = min(ns, 4 ceil(ceil(ns / 4) / 4))
  the states of the fullest wave (a state adds two fused multiply-adds to an accumulator, the x and the y chain; the predicated zeros add nothing and round
  nothing); 3 of the wave additions; 1 of the accumulate addition:  d = 2 n_w + 8, and the error is below sqrt(2) d 2^-24 T to first order.  K_kernel = 3 n_w:
  with the + 32, 3 n_w + 32 >= sqrt(2) (2 n_w + 8) + 20, which leaves the second order and the twin's unfused products their room.  The kernel and the twin
  are held to min(K_kernel, K_products).  Two launches that accumulate are held to the sum of their bounds.  Inputs are fp32 / complex64 on both sides
  (k . shift is formed in double from the same fp32 values), so they add nothing.  Where T = 0 or an orbital is missing the result must be exactly 0.
Nothing here reads the reference tree."""
import types

import numpy as np
import torch

from tests import bond_checks as BC

U = BC.U
WAVES = 4
NS = (1, 3, 4, 5, 16, 17, 33)
_FIX = {}


# ------------------------------------------------------------------------------------------------ fixtures
def weights(c, seed=0):
    """one real weight per state of the case, mixed signs, fp32"""
    key = ("f", id(c), seed)
    if key not in _FIX:
        _FIX[key] = (c, np.random.default_rng(500 + 3 * c.nao + seed).normal(size=c.ns).astype(np.float32))
    return _FIX[key][1]


def k_products(ns):
    return 6 * ns


def k_kernel(ns):
    nw = min(ns, 4 * -(-(-(-ns // 4)) // WAVES))
    return min(3 * nw, k_products(ns))


# ------------------------------------------------------------------------------------------------ the fp64 statement
def ref_density_rows(c, C, kidx, f, kvec=None):
    """(P_on [N, nao^2], P_off [E, nao^2], T_on, T_off) in fp64 from the rows C [ns, M] (any complex dtype; taken as they are), kidx [ns], f [ns] and the
    geometry of the case c: a loop over the members"""
    C = np.asarray(C).astype(np.complex128)
    f = np.asarray(f).astype(np.float64)
    k = np.asarray(c.kvec if kvec is None else kvec).astype(np.float64)[np.asarray(kidx, dtype=np.int64)]      # [ns, 3]
    nao = c.nao
    cols = lambda i: C[:, c.off0[i]:c.off0[i + 1]]
    Pon, Ton = np.zeros((c.N, nao, nao)), np.zeros((c.N, nao, nao))
    Poff, Toff = np.zeros((c.E, nao, nao)), np.zeros((c.E, nao, nao))
    for i in range(c.N):
        ci = cols(i)
        Pon[i][np.ix_(c.orbs[i], c.orbs[i])] = np.einsum("s,sa,sb->ab", f, ci.conj(), ci).real
        Ton[i][np.ix_(c.orbs[i], c.orbs[i])] = np.einsum("s,sa,sb->ab", np.abs(f), np.abs(ci), np.abs(ci))
    for e in range(c.E):
        i, j = int(c.ei[0, e]), int(c.ei[1, e])
        phase = np.exp(2j * np.pi * (k @ np.asarray(c.shift[e]).astype(np.float32).astype(np.float64)))
        Poff[e][np.ix_(c.orbs[i], c.orbs[j])] = np.einsum("s,sa,sb->ab", f * phase, cols(i).conj(), cols(j)).real
        Toff[e][np.ix_(c.orbs[i], c.orbs[j])] = np.einsum("s,sa,sb->ab", np.abs(f), np.abs(cols(i)), np.abs(cols(j)))
    r = lambda a: a.reshape(a.shape[0], nao * nao)
    return r(Pon), r(Poff), r(Ton), r(Toff)


def ref_case(c, lo, hi):
    """the fp64 statement of the states [lo, hi) of a bond_checks.case with its `weights`: computed once, shared, never changed"""
    key = ("ref", id(c), lo, hi)
    if key not in _FIX:
        out = ref_density_rows(c, c.C[lo:hi], c.kidx[lo:hi], weights(c)[lo:hi])
        for a in out:
            a.setflags(write=False)
        _FIX[key] = (c, out)
    return _FIX[key][1]


def bound(T, K):
    return (K + 32) * U * T


def ratio(P, ref, bnd):
    """the largest err / bound; where the bound is 0 (a missing orbital, T = 0) the result must be exactly 0"""
    P = np.asarray(P, dtype=np.float64)
    assert P.shape == ref.shape and np.isfinite(P).all()
    err = np.abs(P - ref)
    assert not err[bnd == 0].any(), float(err[bnd == 0].max(initial=0.0))
    return float((err[bnd > 0] / bnd[bnd > 0]).max(initial=0.0))


def check_rows(P, ref, K, what=""):
    """(P_on, P_off) fp32 against the fp64 statement ref = (P_on, P_off, T_on, T_off): inside (K + 32) 2^-24 T element-wise, zeros exact -> the largest err / bound"""
    worst = 0.0
    for got, want, T in ((P[0], ref[0], ref[2]), (P[1], ref[1], ref[3])):
        got = np.asarray(got)
        assert got.dtype == np.float32
        worst = max(worst, ratio(got, want, bound(T, K)))
    print(f"{what} K={K} err/bound={worst:.3f}")
    return worst


# ------------------------------------------------------------------------------------------------ the numpy twin of the kernel
def density_rows_np(C, kidx, kvec, f, erow, ecol, shift, orank, ooff, P_on=None, P_off=None, accumulate=False):
    C = np.asarray(C, dtype=np.complex64)
    ns, M = C.shape
    N, nao = orank.shape
    E = len(erow)
    f = np.asarray(f, dtype=np.float32)
    k = np.asarray(kvec, dtype=np.float64)[np.asarray(kidx, dtype=np.int64)]
    nsteps = -(-ns // 4)
    chunk = -(-nsteps // WAVES)
    new_on, new_off = np.zeros((N, nao, nao), dtype=np.float32), np.zeros((E, nao, nao), dtype=np.float32)

    def member(i, j, e):
        oi, oj = np.nonzero(orank[i] >= 0)[0], np.nonzero(orank[j] >= 0)[0]       # orbitals in rank order (orank ascends over an atom's valid set)
        ci, cj = C[:, ooff[i] + orank[i][oi]], C[:, ooff[j] + orank[j][oj]]
        ax, ay = f[:, None] * ci.real, f[:, None] * ci.imag
        bx, by = cj.real, cj.imag
        if e is not None:
            ph = 6.283185307179586 * (k @ np.asarray(shift[e], dtype=np.float32).astype(np.float64))
            cf, sf = np.cos(ph).astype(np.float32)[:, None], np.sin(ph).astype(np.float32)[:, None]
            bx, by = cf * cj.real - sf * cj.imag, sf * cj.real + cf * cj.imag
        total = None
        for w in range(WAVES):
            s = slice(4 * w * chunk, min(ns, 4 * (w + 1) * chunk))
            p = ax[s].T @ bx[s] + ay[s].T @ by[s] if s.start < s.stop else np.zeros((len(oi), len(oj)), dtype=np.float32)
            total = p if total is None else total + p           # ((w0 + w1) + w2) + w3
        return oi, oj, total.astype(np.float32)

    have = orank >= 0
    for i in range(N):
        oi, oj, blk = member(i, i, None)
        new_on[i][np.ix_(oi, oj)] = blk
    for e in range(E):
        oi, oj, blk = member(int(erow[e]), int(ecol[e]), e)
        new_off[e][np.ix_(oi, oj)] = blk
    new_on, new_off = new_on.reshape(N, nao * nao), new_off.reshape(E, nao * nao)
    if not accumulate:
        return new_on, new_off
    mask_on = (have[:, :, None] & have[:, None, :]).reshape(N, nao * nao)
    mask_off = (have[erow][:, :, None] & have[ecol][:, None, :]).reshape(E, nao * nao)
    return np.where(mask_on, P_on + new_on, P_on).astype(np.float32), np.where(mask_off, P_off + new_off, P_off).astype(np.float32)


def density_rows_cpu(C, kidx, kvec, f, erow, ecol, shift, orank, ooff, out=None, accumulate=False):
    from hamgnn_amd import ops
    ops.density_rows_check(C, kidx, kvec, f, erow, ecol, shift, orank, ooff, out, accumulate)
    n = lambda t: t.numpy()
    old = (n(out[0]), n(out[1])) if accumulate else (None, None)
    on, off = density_rows_np(n(C), n(kidx), n(kvec), n(f), n(erow), n(ecol), n(shift), n(orank), n(ooff), *old, accumulate=accumulate)
    if out is None:
        return torch.from_numpy(on), torch.from_numpy(off)
    out[0].copy_(torch.from_numpy(on)), out[1].copy_(torch.from_numpy(off))
    return out[0], out[1]


def install_cpu(monkeypatch):
    """the numpy twin in place of the HIP wrapper; density.density_rows then takes its kernel route on CPU tensors"""
    from hamgnn_amd import dos, ops
    monkeypatch.setattr(ops, "density_rows", density_rows_cpu)
    monkeypatch.setattr(dos, "_use_kernels", lambda t: True)


# ------------------------------------------------------------------------------------------------ running density.density_rows on a case
def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def tables_of(c, device):
    from hamgnn_amd import bonds
    t = bonds.bond_tables(c.head, c.z, c.ei, c.shift, device)
    assert t.M == c.M
    return t


def run(c, device, lo=0, hi=None, C=None, kidx=None, kvec=None, f=None, out=None, accumulate=False):
    """density.density_rows on the states [lo, hi) of the case (its C, kidx, kvec and `weights` unless given), through bond_tables -> (P_on, P_off) as numpy,
    or the tensors written into when `out` is given"""
    from hamgnn_amd import density
    hi = c.ns if hi is None else hi
    pick = lambda given, own: (own if given is None else given)[lo:hi]
    P = density.density_rows(dev(pick(C, c.C), device), dev(pick(kidx, c.kidx), device), dev(c.kvec if kvec is None else kvec, device),
                             dev(pick(f, weights(c)), device), tables_of(c, device), out=out, accumulate=accumulate)
    return P if out is not None else (P[0].cpu().numpy(), P[1].cpu().numpy())


def solved_case():
    """bond_checks.solvable_case() solved on the host (fp64, from the dense restatement of the assembly: nothing runs on a GPU): a namespace with eps [nk, nb],
    C complex64 [nk nb, M] S-normalised rows, C128 the same in complex128, kidx, sigma, mu = dos.fermi_level at half filling (deg 2, nel = M), occ =
    density.occupations there, f = k_w occ as fp32 and fe = k_w occ eps as fp32"""
    if "solved" in _FIX:
        return _FIX["solved"]
    from hamgnn_amd import density, dos
    c = BC.solvable_case()
    kd = c.kvec.astype(np.float64)
    eps, Cs = BC.solve_host([BC.dense_xk(c, c.Hon, c.Hoff, k) for k in kd], [BC.dense_xk(c, c.Son, c.Soff, k) for k in kd])
    nk, nb = eps.shape
    w = np.repeat(c.k_w, nb).reshape(nk, nb)
    sigma, nel = 0.05 * float(eps.max() - eps.min()), float(c.M)
    mu = dos.fermi_level(eps.reshape(-1), w.reshape(-1), nel, sigma, 2)
    occ = density.occupations(eps, mu, sigma, deg=2)
    s = types.SimpleNamespace(c=c, eps=eps, nk=nk, nb=nb, w=w, sigma=sigma, nel=nel, mu=mu, occ=occ, C128=Cs.reshape(nk * nb, c.M),
                              C=Cs.reshape(nk * nb, c.M).astype(np.complex64), kidx=np.repeat(np.arange(nk), nb).astype(np.int32),
                              f=(w * occ).reshape(-1).astype(np.float32), fe=(w * occ * eps).reshape(-1).astype(np.float32))
    _FIX["solved"] = s
    return s


def sum_rule_tolerance(c, C, kidx, f, Xon, Xoff, K, want):
    """what the sum over all members of sum_ab P X may differ from `want` by: the carried bound sum |X| bound_P, the rounding of C to complex64
    (4 x 2^-24 sum_s |f_s| sum_ab |c_a| |X_ab| |c_b|) and 1e-10 |want| for the fp64 side"""
    _, _, Ton, Toff = ref_density_rows(c, C, kidx, f)
    mag = float((np.abs(Xon.astype(np.float64)) * Ton).sum() + (np.abs(Xoff.astype(np.float64)) * Toff).sum())      # sum_s |f| sum_ab |c_a| |X_ab| |c_b|
    return (K + 32) * U * mag + 4 * U * mag + 1e-10 * abs(want)
