"""Checks of hamgnn_amd/velocity.py and the kernel hg_kgrad_elements of csrc/spectra.hip, shared by tests/test_velocity_gpu.py (the HIP kernel) and
tests/test_velocity_cpu.py (host logic, the torch path, and the numpy twin below in place of the kernel).  The crystals are those of tests/bond_checks.py.

The exact statement is `ref_kgrad_elements`: the formula of velocity.py's docstring in complex128 numpy, edge by edge,
  out[p, alpha] = sum_e i rvec[e, alpha] exp(2 pi i k_p . shift_e) sum_{a, b} conj(C[bra_p, mu(i, a)]) X_off[e][a, b] C[ket_p, mu(j, b)],
on the compact orbital lists written out from the head's basis_def (bond_checks.compact, not through bond_tables).  The twin `kgrad_elements_np` follows
the kernel's structure in fp32: per edge the masked nao x nao block times Re C_ket and Im C_ket, conj(C_bra) . T summed per lane quarter (rows 4 q .. 4 q + 3
of every 16-row tile) and the quarters added as (q0 + q1) + (q2 + q3), the phase from double rounded once as a complex product, the three components added
to the wave's running sums, the chunk of `chunk_edges(E)` edges dealt to 4 waves in contiguous quarters, ((w0 + w1) + w2) + w3, and the chunks added in
ascending order.  Every sum of the twin is taken row by row (no BLAS call), so a pair's bits do not depend on the other pairs, as in the kernel.

The bound, per element, on the real and on the imaginary part:  |out - ref| <= (K + 32) 2^-24 T,
  T[p, alpha] = sum_e |rvec[e, alpha]| sum_{a, b} |c_bra,a| |X_ab| |c_ket,b| in fp64.
  Any order (`k_products`, the torch path):  the real (or imaginary) part of an element is a sum of n = 4 sum_e n_i n_j real products r x (cos or sin) x
  (x or y of c_bra) x X x (x or y of c_ket).  The four products of one (e, a, b) sum in magnitude to at most (|cos| + |sin|) |r| |c_a| |X_ab| |c_b| <=
  sqrt(2) |r| |c_a| |X_ab| |c_b| (Cauchy-Schwarz on (|x_a|, |y_a|) . (|x_b|, |y_b|) for each of the cos and the sin pair), so all of them to at most sqrt(2) T,
  and n additions in any order err by at most n 2^-24 times that:  sqrt(2) 4 sum_e n_i n_j < K_products = 6 sum_e n_i n_j.  The + 32 holds the roundings
  of the factors of one product (cos / sin from double, four multiplications: sqrt(2) x 5 < 8) and the second order.
  The kernel's chain is shorter (`k_kernel`).  One real product passes, on its way into out, at most d roundings: n_j fused multiply-adds of the MFMA
  chain over b (the predicated zeros add nothing and round nothing); 2 per row of the lane's 4 ceil(nao / 16) rows (conj(c_bra) T: two fmas each for the real
  and the imaginary sum); 2 shuffle additions; 3 for the phase (cos / sin rounded from double, one product, one fma); ceil(chunk / 4) fmas of the wave's
  running sum (the product with rvec is fused into them); 3 additions of the waves' sums; n_chunks additions of the second pass:
  d = n_j + 8 ceil(nao / 16) + ceil(chunk / 4) + n_chunks + 8, and the error is below sqrt(2) d 2^-24 T to first order.
  K_kernel = 2 (max n_j + 8 ceil(nao / 16) + ceil(chunk / 4) + n_chunks):  K_kernel + 32 >= sqrt(2) d + 20, which leaves the second order and the twin's
  unfused products their room.  The kernel and the twin are held to min(K_kernel, K_products).  Inputs are fp32 / complex64 on both sides (k . shift is
  formed in double from the same fp32 values), so they add nothing.  Where T = 0 (a zero column of rvec, no edge) the result must be exactly 0.

Physics (`solved`): bond_checks.solvable_case() solved on the host in fp64 at its 8 grid points and at 4 seeded random k-points; `hf_velocities` is the
Hellmann-Feynman statement v = Re c^+ (dH - eps dS) c in fp64, `fd_velocities` a central difference of bond_checks.solve_host energies.
Nothing here reads the reference tree."""
import types

import numpy as np
import torch

from tests import bond_checks as BC
from tests import density_checks as DC

U = BC.U
WAVES = 4
NPAIRS = (1, 3, 16, 17, 33)
_FIX = {}


def chunk_edges(E):
    """edges per chunk of the kernel's edge split (csrc/hg_common.h): 8 ceil(E / 2048), 8 at least"""
    return 8 * max(1, -(-E // 2048))


def chunks(E):
    return -(-E // chunk_edges(E)) if E > 0 else 0


# ------------------------------------------------------------------------------------------------ fixtures
def pairs(c, npair):
    """(bra, ket) int32 [npair]: diagonal pairs (s, s) at the even slots, off-diagonal (s, s + 2) at the odd ones -- kidx = s % 2 in bond_checks.case, so the
    two states share a k-point.  The first m pairs of a longer list are the list of length m."""
    p = np.arange(npair)
    bra = (p % (c.ns - 2)).astype(np.int32)
    return bra, (bra + 2 * (p % 2)).astype(np.int32)


def rvec_of(c, E=None, zero_col=None):
    """velocity.edge_vectors(cell, shift) of the case's first E edges as numpy fp32, column zero_col set to 0"""
    from hamgnn_amd import velocity
    r = velocity.edge_vectors(c.cell, c.shift[:E]).numpy().copy()
    if zero_col is not None:
        r[:, zero_col] = 0.0
    return r


def k_products(c, E=None):
    n = np.array([len(v) for v in c.orbs])
    E = c.E if E is None else E
    return 6 * int((n[c.ei[0, :E]] * n[c.ei[1, :E]]).sum())


def k_kernel(c, E=None):
    n = np.array([len(v) for v in c.orbs])
    E = c.E if E is None else E
    if E == 0:
        return 0
    return min(k_products(c, E), 2 * (int(n[c.ei[1, :E]].max()) + 8 * -(-c.nao // 16) + -(-chunk_edges(E) // WAVES) + chunks(E)))


# ------------------------------------------------------------------------------------------------ the fp64 statement
def ref_kgrad_elements(c, bra, ket, Xoff, rvec, C=None, kidx=None, kvec=None, E=None):
    """(out [np, 3] complex128, T [np, 3]) in fp64 from the rows C [ns, M] (any complex dtype, taken as they are; the case's by default), kidx, kvec and the
    geometry of the case c: a loop over the first E edges"""
    C = np.asarray(c.C if C is None else C).astype(np.complex128)
    kidx = np.asarray(c.kidx if kidx is None else kidx, dtype=np.int64)
    k = np.asarray(c.kvec if kvec is None else kvec).astype(np.float64)[kidx[np.asarray(ket, dtype=np.int64)]]      # [np, 3]
    E = c.E if E is None else E
    rv = np.asarray(rvec).astype(np.float64)
    cols = lambda rows, i: C[np.asarray(rows, dtype=np.int64), c.off0[i]:c.off0[i + 1]]
    out, T = np.zeros((len(ket), 3), dtype=np.complex128), np.zeros((len(ket), 3))
    for e in range(E):
        i, j = int(c.ei[0, e]), int(c.ei[1, e])
        X = Xoff[e].astype(np.float64).reshape(c.nao, c.nao)[np.ix_(c.orbs[i], c.orbs[j])]
        phase = np.exp(2j * np.pi * (k @ np.asarray(c.shift[e]).astype(np.float32).astype(np.float64)))
        z = phase * np.einsum("pa,ab,pb->p", cols(bra, i).conj(), X, cols(ket, j))
        out += 1j * z[:, None] * rv[e][None, :]
        T += np.einsum("pa,ab,pb->p", np.abs(cols(bra, i)), np.abs(X), np.abs(cols(ket, j)))[:, None] * np.abs(rv[e])[None, :]
    return out, T


def ratio(out, ref, T, K):
    """the largest err / bound over the real and the imaginary parts; where the bound is 0 the result must be exactly 0"""
    out = np.asarray(out)
    assert out.shape == ref.shape and out.dtype == np.complex64 and np.isfinite(out.view(np.float32)).all()
    bnd = (K + 32) * U * T
    worst = 0.0
    for err in (np.abs(out.real.astype(np.float64) - ref.real), np.abs(out.imag.astype(np.float64) - ref.imag)):
        assert not err[bnd == 0].any(), float(err[bnd == 0].max(initial=0.0))
        worst = max(worst, float((err[bnd > 0] / bnd[bnd > 0]).max(initial=0.0)))
    return worst


def ref_case(c, npair, E=None, zero_col=None):
    """the fp64 statement of `pairs(c, npair)` on the case's own rows with `rvec_of`: computed once, shared, never changed"""
    key = ("ref", id(c), npair, E, zero_col)
    if key not in _FIX:
        bra, ket = pairs(c, npair)
        out = ref_kgrad_elements(c, bra, ket, c.Xoff, rvec_of(c, E, zero_col), E=E)
        for a in out:
            a.setflags(write=False)
        _FIX[key] = (c, out)
    return _FIX[key][1]


# ------------------------------------------------------------------------------------------------ the numpy twin of the kernel
def kgrad_elements_np(C, bra, ket, kidx, kvec, Xoff, erow, ecol, shift, rvec, orank, ooff):
    C = np.asarray(C, dtype=np.complex64)
    ns, M = C.shape
    N, nao = orank.shape
    E, npair = len(erow), len(ket)
    nt = -(-nao // 16)
    f32 = np.float32
    have = orank >= 0
    comp = np.where(have, ooff[:, None] + orank, M)
    CA = np.concatenate([C, np.zeros((ns, 1), dtype=np.complex64)], 1)[:, comp]                      # [ns, N, nao], 0 where the atom lacks the orbital
    CB, CK = CA[np.asarray(bra, dtype=np.int64)], CA[np.asarray(ket, dtype=np.int64)]
    k = np.asarray(kvec, dtype=np.float64)[np.asarray(kidx, dtype=np.int64)[np.asarray(ket, dtype=np.int64)]]
    pad = lambda a: np.concatenate([a, np.zeros((npair, 16 * nt - nao), dtype=f32)], 1)
    lanes = lambda v: pad(v).reshape(npair, nt, 4, 4).transpose(0, 2, 1, 3).reshape(npair, 4, 4 * nt).sum(-1, dtype=f32)      # [np, quarter]
    quarters = lambda q: (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])

    def edge(e):
        i, j = int(erow[e]), int(ecol[e])
        Xm = np.where(have[i][:, None] & have[j][None, :], np.asarray(Xoff[e], dtype=f32).reshape(nao, nao), f32(0))
        cj, ci = CK[:, j], CB[:, i]
        tr = (cj.real[:, None, :] * Xm[None]).sum(-1, dtype=f32)                                     # [np, nao]: T = X c_ket, row by row
        ti = (cj.imag[:, None, :] * Xm[None]).sum(-1, dtype=f32)
        pr = quarters(lanes(ci.real * tr) + lanes(ci.imag * ti))
        pi = quarters(lanes(ci.real * ti) - lanes(ci.imag * tr))
        ph = 6.283185307179586 * (k @ np.asarray(shift[e], dtype=f32).astype(np.float64))
        cf, sf = np.cos(ph).astype(f32), np.sin(ph).astype(f32)
        zr, zi = cf * pr - sf * pi, cf * pi + sf * pr
        r = np.asarray(rvec[e], dtype=f32)
        return np.stack([v for al in range(3) for v in (-r[al] * zi, r[al] * zr)], 1)              # [np, 6]: (re, im) of the three components

    out = np.zeros((npair, 6), dtype=f32)
    ce = chunk_edges(E)
    for ch in range(chunks(E)):
        eb, ee = ch * ce, min(E, (ch + 1) * ce)
        quarter = -(-(ee - eb) // WAVES)
        total = None
        for w in range(WAVES):
            s = np.zeros((npair, 6), dtype=f32)
            for e in range(eb + w * quarter, min(ee, eb + (w + 1) * quarter)):
                s = s + edge(e)
            total = s if total is None else total + s           # ((w0 + w1) + w2) + w3
        out = out + total                                      # the chunks in ascending order
    return np.ascontiguousarray(out).view(np.complex64).reshape(npair, 3)


def kgrad_elements_cpu(C, bra, ket, kidx, kvec, X_off, erow, ecol, shift, rvec, orank, ooff):
    from hamgnn_amd import ops
    ops.kgrad_elements_check(C, bra, ket, kidx, kvec, X_off, erow, ecol, shift, rvec, orank, ooff)
    n = lambda t: t.numpy()
    return torch.from_numpy(kgrad_elements_np(n(C), n(bra), n(ket), n(kidx), n(kvec), n(X_off), n(erow), n(ecol), n(shift), n(rvec), n(orank), n(ooff)))


def install_cpu(monkeypatch):
    """the numpy twin in place of the HIP wrapper; velocity.kgrad_elements then takes its kernel route on CPU tensors"""
    from hamgnn_amd import dos, ops
    monkeypatch.setattr(ops, "kgrad_elements", kgrad_elements_cpu)
    monkeypatch.setattr(dos, "_use_kernels", lambda t: True)


# ------------------------------------------------------------------------------------------------ running velocity.kgrad_elements on a case
def tables_of(c, device, E=None):
    from hamgnn_amd import bonds
    t = bonds.bond_tables(c.head, c.z, c.ei[:, :E], c.shift[:E], device)
    assert t.M == c.M
    return t


def run(c, device, bra, ket, E=None, zero_col=None, Xoff=None, rvec=None, C=None, kidx=None, kvec=None):
    """velocity.kgrad_elements on the pairs (bra, ket) of the case's rows and first E edges (its C, kidx, kvec, Xoff and `rvec_of` unless given), through
    bond_tables -> out [np, 3] complex64 as numpy"""
    from hamgnn_amd import velocity
    dev = lambda a: DC.dev(a, device)
    E = c.E if E is None else E
    out = velocity.kgrad_elements(dev(c.C if C is None else C), dev(bra), dev(ket), dev(c.kidx if kidx is None else kidx), dev(c.kvec if kvec is None else kvec),
                                  dev((c.Xoff if Xoff is None else Xoff)[:E]), tables_of(c, device, E), dev(rvec_of(c, E, zero_col) if rvec is None else rvec))
    return out.cpu().numpy()


def check_case(device, nao, npair, kernel, E=None, zero_col=None):
    """run + ratio on `pairs(case(nao), npair)` -> the largest err / bound (printed)"""
    c = BC.case(nao)
    bra, ket = pairs(c, npair)
    ref, T = ref_case(c, npair, E, zero_col)
    K = k_kernel(c, E) if kernel else k_products(c, E)
    out = run(c, device, bra, ket, E=E, zero_col=zero_col)
    if zero_col is not None:
        assert not out[:, zero_col].real.any() and not out[:, zero_col].imag.any()
    r = ratio(out, ref, T, K)
    print(f"nao={nao} np={npair} E={c.E if E is None else E} chunks={chunks(c.E if E is None else E)} kernel={kernel} K={K} err/bound={r:.3f}")
    return r


# ------------------------------------------------------------------------------------------------ physics: the solved crystal
def solved():
    """density_checks.solved_case() (the 2 x 2 x 2 grid, M = 18) extended by 4 seeded random k-points (fp32-representable), solved on the host in fp64: a
    namespace with c, kvec fp32 [12, 3], eps [12, nb], C128 / C complex [12 nb, M] S-normalised rows, kidx, ns, nk_grid = 8"""
    if "solved" in _FIX:
        return _FIX["solved"]
    s0 = DC.solved_case()
    c = s0.c
    extra = np.random.default_rng(2024).uniform(-0.5, 0.5, size=(4, 3)).astype(np.float32)
    eps2, C2 = solve_at(c, extra.astype(np.float64))
    nk, nb = s0.nk + 4, s0.nb
    C128 = np.concatenate([s0.C128, C2.reshape(4 * nb, c.M)])
    s = types.SimpleNamespace(c=c, kvec=np.concatenate([c.kvec, extra]), eps=np.concatenate([s0.eps, eps2]), C128=C128, C=C128.astype(np.complex64),
                              kidx=np.repeat(np.arange(nk), nb).astype(np.int32), ns=nk * nb, nk=nk, nb=nb, nk_grid=s0.nk)
    _FIX["solved"] = s
    return s


def solve_at(c, k_red):
    """(eps [n, M], C [n, band, M]) of the case at the reduced k-points k_red [n, 3], fp64 on the host"""
    return BC.solve_host([BC.dense_xk(c, c.Hon, c.Hoff, k) for k in k_red], [BC.dense_xk(c, c.Son, c.Soff, k) for k in k_red])


def solved_view(s, C):
    """the case namespace with the solved rows in place of bond_checks.case's random ones (what ref_kgrad_elements and run read)"""
    return types.SimpleNamespace(**{**vars(s.c), "C": C, "kidx": s.kidx, "kvec": s.kvec, "ns": s.ns})


def lattice_rvec(c):
    """R = cell_shift @ cell in fp64 (the rows of cell are the lattice vectors), rounded to fp32 as velocity.edge_vectors returns it"""
    return (np.asarray(c.shift, dtype=np.float64) @ c.cell).astype(np.float32)


def hf_velocities(s, rvec=None):
    """(v [ns, 3], T_H [ns, 3], T_S [ns, 3]) in fp64: v = Re c^+ (dH - eps dS) c from the complex128 rows, state by state"""
    key = ("hf", rvec is None)
    if key in _FIX and rvec is None:
        return _FIX[key]
    c = solved_view(s, s.C128)
    d = np.arange(s.ns, dtype=np.int32)
    rv = lattice_rvec(s.c) if rvec is None else rvec
    dH, TH = ref_kgrad_elements(c, d, d, s.c.Hoff, rv)
    dS, TS = ref_kgrad_elements(c, d, d, s.c.Soff, rv)
    out = (dH.real - s.eps.reshape(-1)[:, None] * dS.real, TH, TS)
    if rvec is None:
        _FIX[key] = out
    return out


def fd_velocities(s, h=1e-5):
    """v [ns, 3] in fp64: the central difference (eps(k + h e_alpha) - eps(k - h e_alpha)) / 2 h of bond_checks.solve_host energies along each Cartesian axis,
    dk_red = dk_cart @ cell.T / 2 pi"""
    if ("fd", h) in _FIX:
        return _FIX["fd", h]
    k = s.kvec.astype(np.float64)
    v = np.zeros((s.nk, s.nb, 3))
    for al in range(3):
        dk = (h * np.eye(3)[al]) @ s.c.cell.T / (2.0 * np.pi)
        v[:, :, al] = (solve_at(s.c, k + dk)[0] - solve_at(s.c, k - dk)[0]) / (2.0 * h)
    _FIX["fd", h] = v.reshape(s.ns, 3)
    return _FIX["fd", h]


def velocity_tolerance(s, K):
    """what band_velocities on the complex64 rows may differ from `hf_velocities` by, per element [ns, 3]: the two kernels' bounds carried through the
    combination, (K + 32) 2^-24 (T_H + |eps| T_S); the rounding of C to complex64 (each of the two rows of a product: 4 x 2^-24 of the same magnitude sum);
    one rounding of the combined fp64 value to fp32, 2^-24 |v| <= 2^-24 (T_H + |eps| T_S); and 1e-12 of it for the fp64 side"""
    _, TH, TS = hf_velocities(s)
    mag = TH + np.abs(s.eps.reshape(-1))[:, None] * TS
    return (K + 32) * U * mag + 4 * U * mag + U * mag + 1e-12 * mag


def run_velocities(s, device, degenerate_tol=None, with_S=True):
    """velocity.band_velocities on the solved crystal (complex64 rows, fp64 eigenvalues, the lattice gauge) -> v [ns, 3] fp32 as numpy"""
    from hamgnn_amd import velocity
    dev = lambda a: DC.dev(a, device)
    c = s.c
    rvec = velocity.edge_vectors(c.cell, c.shift).to(device)
    v = velocity.band_velocities(s.eps, dev(s.C), dev(s.kidx), dev(s.kvec), dev(c.Hoff), dev(c.Soff) if with_S else None, tables_of(c, device), rvec,
                                 degenerate_tol=degenerate_tol)
    assert v.dtype == torch.float32 and tuple(v.shape) == (s.ns, 3)
    return v.cpu().numpy()


def closest_pair(s):
    """(state index a of the closest pair (a, a + 1) of adjacent levels of one k-point, a tolerance that joins this pair and no other)"""
    gaps = np.diff(s.eps, axis=1)                               # [nk, nb - 1]
    order = np.argsort(gaps.reshape(-1))
    g1, g2 = gaps.reshape(-1)[order[0]], gaps.reshape(-1)[order[1]]
    kq, b = divmod(int(order[0]), s.nb - 1)
    assert g2 > g1 > 0
    return kq * s.nb + b, 0.5 * (g1 + g2)


def degenerate_block_eigenvalues(s, a):
    """[2, 3] fp64: per component the ascending eigenvalues of the block <m| d H - eps_mean d S |n> of the states a, a + 1 (complex128 rows, lattice gauge)"""
    c = solved_view(s, s.C128)
    bra, ket = np.array([a, a, a + 1, a + 1], dtype=np.int32), np.array([a, a + 1, a, a + 1], dtype=np.int32)
    rv = lattice_rvec(s.c)
    em = s.eps.reshape(-1)[a:a + 2].mean()
    B = (ref_kgrad_elements(c, bra, ket, s.c.Hoff, rv)[0] - em * ref_kgrad_elements(c, bra, ket, s.c.Soff, rv)[0]).reshape(2, 2, 3)
    assert np.abs(B - B.conj().transpose(1, 0, 2)).max() <= 1e-9 * max(1.0, np.abs(B).max())
    return np.stack([np.linalg.eigvalsh(0.5 * (B[:, :, al] + B[:, :, al].conj().T)) for al in range(3)], 1)
