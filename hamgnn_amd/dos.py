"""Density of states and its projections on a Brillouin-zone grid: the parts after the eigen-solver, and the grid.

    k_red, k_w = monkhorst_pack((8, 8, 8))                                  # Gamma-centred grid, k / -k folded
    perm, gptr, labels = group_map(head, z, "atom")                         # orbital groups of a projection in the compact orbital order
    W = state_weights(C, SC, perm_d, gptr_d, wk, padded_groups(len(labels)))    # Mulliken weights of the states of a k-chunk (C, S c rows)
    D = broaden(eps_sorted, W_sorted, E0, dE, ne, sigma, D=D, accumulate=D is not None)

`state_weights`: w = sum_{mu in g} Re(conj(c_mu) (S(k) c)_mu) by the HIP kernel `hg_mulliken_weights`; `broaden`: D[j, g] = sum_s A(E_j, eps_s) W[s, g] by
the HIP kernel `hg_dos_broaden` (csrc/spectra.hip), which generates the Gaussians in registers from the sorted eigenvalues and adds chunks into D in the
order given.  CPU tensors, and HG_DOS=torch on the GPU, take a plain torch path for the two steps (`exp` of an [energies, states] matrix in chunks + matmul;
group sums as one matmul with the 0 / 1 group matrix): the CPU route, and the baseline of tests/bench_dos.py.  `fermi_level`, `energy_grid`: host, fp64.

Next to the Gaussians, the linear tetrahedron method (no width parameter; band edges and van Hove singularities on coarse grids; a closed-form number of states):

    tet = tetrahedra((8, 8, 8), cell)                                       # six per grid cell around its shortest diagonal; corners = rows of monkhorst_pack's list
    W = state_weights(C, SC, perm_d, gptr_d, ones, Gp).reshape(nk, nb, Gp)  # wk = 1: the tetrahedra carry the k-weights
    D = tetra_dos(eps, W, tet, E0, dE, ne)                                  # eps [nk, nb] as the solver returns it; tetra_states: the number of states
    mu = fermi_level_tetra(eps, tet, nel, deg=2)

`monkhorst_pack_map`: full grid -> rows of the folded list; `corner_table`: per k-row the (tetrahedron, corner) pairs, the kernel's summation order.
`tetra_dos` / `tetra_states`: D[j, g] = sum_{k,b} A(E_j; k, b) W[k, b, g] with A the sum of Bloechl's corner weights over the corner table of k-row k, by the
HIP kernel `hg_dos_tetra` (the same GEMM as the broadening with another generator for the left operand; band chunks can be added in turn), or torch ops (CPU
tensors, HG_DOS=torch; the baseline of tests/bench_dos_tetra.py).  The formulas and the rule for flat tetrahedra stand in `tetra_dos`'s docstring.

Bond-resolved weights (COOP / COHP / ICOHP: which bonds the states are in) come from hamgnn_amd/bonds.py: `bonds.bond_weights` writes rows in the same
[ns, Gp] layout from the real-space rows and the eigenvectors, and `broaden`, `tetra_dos` and `tetra_states` take them unchanged.  The integrated,
real-space counterpart -- the density matrix on the graph's rows at the occupations of `fermi_level` -- is hamgnn_amd/density.py.

NOT built: the driver from saved Hamiltonian rows (assembly of H(k) / S(k), solver, these steps, per crystal and k-chunk).  Its one run at a realistic size
(64 Si atoms, M = 832) ended in a GPU launch failure whose cause was not found, so it was taken out with its tests: profiles/dos.md."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import ops

SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn "
           "Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk "
           "Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og").split()
SHELL_LETTERS = "spdfghik"
PROJECTIONS = (None, "atom", "species", "shell")
PAD_SIGMAS = 8.0            # erange_eV=None: the whole spectrum +- 8 sigma


# ------------------------------------------------------------------------------------------------ the k-grid
def _fold_time_reversal(k):
    """the k / -k folding of a full grid k [n, 3]: yields, per point in grid order, (r, True) -- the point is kept as row r of the folded list -- or
    (r, False) -- it is the partner (-k modulo a reciprocal lattice vector) of the kept row r.  The first of a pair in grid order is kept."""
    key = lambda v: tuple(int(t) for t in np.rint((v - np.floor(v + 1e-12)) * 2 ** 40) % 2 ** 40)      # k modulo 1 on a 2^-40 lattice
    seen, kept = {}, 0
    for i in range(k.shape[0]):
        me, partner = key(k[i]), key(-k[i])
        if partner in seen and partner != me:
            yield seen[partner], False
            continue
        seen[me] = kept
        yield kept, True
        kept += 1


def monkhorst_pack(grid, shift=(0, 0, 0), time_reversal: bool = True):
    """(k_reduced [nk, 3], weights [nk]): the Gamma-centred n1 x n2 x n3 grid k = ((i1 + s1) / n1, (i2 + s2) / n2, (i3 + s3) / n3) folded into
    (-1/2, 1/2], weights summing to 1.  With `time_reversal`, k and -k (modulo a reciprocal lattice vector) are one point of doubled weight --
    H(-k) = H(k)^* has the same eigenvalues and Mulliken weights; the point kept is the first of the pair in grid order (i3 fastest)."""
    n = [int(v) for v in grid]
    if len(n) != 3 or min(n) < 1:
        raise ValueError(f"monkhorst_pack: the grid must be three positive integers, got {grid!r}")
    s = np.asarray(shift, dtype=np.float64).reshape(3)
    idx = np.stack(np.meshgrid(*[np.arange(v) for v in n], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    k = (idx + s[None, :]) / np.asarray(n, dtype=np.float64)[None, :]
    k = k - np.ceil(k - 0.5)                                   # into (-1/2, 1/2]
    k[np.abs(k) < 1e-14] = 0.0
    w = np.full(k.shape[0], 1.0 / k.shape[0])
    if not time_reversal:
        return k, w
    fold = list(_fold_time_reversal(k))
    keep = [i for i, (_, kept) in enumerate(fold) if kept]
    weight = np.bincount([r for r, _ in fold], weights=w)      # a row's weight: the kept point's, then its partner's
    return k[keep], weight


def monkhorst_pack_map(grid, shift=(0, 0, 0), time_reversal: bool = True) -> np.ndarray:
    """int32 [n1 n2 n3]: for every point of the full grid, in the order monkhorst_pack enumerates it (i3 fastest), the row of that point or of its
    time-reversal partner in the list monkhorst_pack returns for the same arguments (the same folding rule: the first of a pair in grid order is kept)"""
    k, _ = monkhorst_pack(grid, shift, time_reversal=False)
    if not time_reversal:
        return np.arange(k.shape[0], dtype=np.int32)
    return np.asarray([r for r, _ in _fold_time_reversal(k)], dtype=np.int32)


_CORNERS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])           # the starting corners of the four main diagonals of a grid cell
_PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))   # three even, three odd


def cell_tetrahedra(grid, cell) -> np.ndarray:
    """int [6, 4, 3]: the corners, in grid steps from a cell's origin, of the six tetrahedra one grid cell is cut into around its shortest main
    diagonal in Cartesian reciprocal space (Bloechl's choice; ties: the first of (000-111, 100-011, 010-101, 001-110)).  Each tetrahedron is a
    path start -> +-step_a -> +-step_b -> +-step_c = end over one permutation of the axes; odd permutations have corners 1 and 2 exchanged, so all six have the
    same signed volume, 1 / 6 of the cell's."""
    n = np.asarray([int(v) for v in grid], dtype=np.float64)
    rec = np.linalg.inv(np.asarray(cell, dtype=np.float64)).T / n[:, None]          # rows: one grid step along each reciprocal axis
    sign = 1 - 2 * _CORNERS
    start = _CORNERS[int(np.argmin([np.linalg.norm(s @ rec) for s in sign]))]
    s = 1 - 2 * start
    out = np.empty((6, 4, 3), dtype=np.int64)
    for t, perm in enumerate(_PERMS):
        p = start.copy()
        out[t, 0] = p
        for c, ax in enumerate(perm):
            p = p.copy()
            p[ax] += s[ax]
            out[t, 1 + c] = p
        if (t >= 3) != (int(np.prod(s)) < 0):                      # orientation = parity of the permutation x the diagonal's direction
            out[t, [1, 2]] = out[t, [2, 1]]
    return out


def tetrahedra(grid, cell, shift=(0, 0, 0), time_reversal: bool = True) -> np.ndarray:
    """int32 [6 n1 n2 n3, 4]: every cell of the periodic grid cut into six tetrahedra (cell_tetrahedra), the corners as rows of monkhorst_pack's list for
    the same arguments (through monkhorst_pack_map).  All have the same volume: the weight of each is 1 / (6 n1 n2 n3).  A direction with n_i = 1, and
    the k / -k folding, give tetrahedra with repeated corners; the weight formulas (tetra_dos) hold for them."""
    n = [int(v) for v in grid]
    kmap = monkhorst_pack_map(n, shift, time_reversal)
    idx = np.stack(np.meshgrid(*[np.arange(v) for v in n], indexing="ij"), -1).reshape(-1, 1, 1, 3)
    c = (idx + cell_tetrahedra(n, cell)[None]) % np.asarray(n)[None, None, None, :]
    return kmap[(c[..., 0] * n[1] + c[..., 1]) * n[2] + c[..., 2]].reshape(-1, 4).astype(np.int32)


def corner_table(tet, nk):
    """(kt_ptr int32 [nk + 1], kt_tet int32 [4 nt], kt_corner int32 [4 nt]): per k-row the (tetrahedron, corner slot) pairs that touch it, ascending in
    the tetrahedron (then the slot): the fixed summation order of hg_dos_tetra"""
    tet = np.asarray(tet)
    if tet.ndim != 2 or tet.shape[1] != 4 or (tet.size and (tet.min() < 0 or tet.max() >= nk)):
        raise ValueError(f"corner_table: tet must be [nt, 4] with entries in [0, {nk}), got {tet.shape}")
    flat = tet.reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=nk))]).astype(np.int32)
    return ptr, (order // 4).astype(np.int32), (order % 4).astype(np.int32)


# ------------------------------------------------------------------------------------------------ orbital groups
def orbital_shells(head) -> np.ndarray:
    """[nao_max] angular momentum l of every orbital position of the head's basis (the row irreps, carried through index_change, which permutes
    inside shells only)"""
    l_row = np.concatenate([np.full(mul * (2 * l + 1), l, dtype=np.int64) for mul, l, _ in head.row])
    ic = head.index_change
    return l_row if ic is None else l_row[np.asarray(ic, dtype=np.int64)]


def group_map(head, z, projection):
    """head: a HamGNNPlusPlusOut (its basis tables); z: the crystal's atomic numbers.
    (perm int32[M or 0], gptr int32[G + 1], labels [G]) for the compact orbital order of one crystal (atom by atom, the element's orbitals ascending):
    projection None -> no group; "atom" -> one group per atom, ("Si", 3); "species" -> one per element in ascending atomic number, "O";
    "shell" -> one per (atom, l), ("Si", 3, "p").  Inside a group the orbitals ascend."""
    if projection not in PROJECTIONS:
        raise ValueError(f"projection={projection!r}: one of {PROJECTIONS}")
    zs = [int(v) for v in np.asarray(z).reshape(-1)]
    if projection is None:
        return np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int32), []
    lsh = orbital_shells(head)
    keys, members, m = [], {}, 0
    for i, Z in enumerate(zs):
        for a in sorted(head.basis_def[Z]):
            kk = (i,) if projection == "atom" else (Z,) if projection == "species" else (i, int(lsh[a]))
            if kk not in members:
                members[kk] = []
                keys.append(kk)
            members[kk].append(m)
            m += 1
    if projection == "species":
        keys.sort()
    labels = [(SYMBOLS[zs[kk[0]]], kk[0]) if projection == "atom" else SYMBOLS[kk[0]] if projection == "species"
              else (SYMBOLS[zs[kk[0]]], kk[0], SHELL_LETTERS[kk[1]]) for kk in keys]
    perm = np.concatenate([np.asarray(members[kk], dtype=np.int32) for kk in keys])
    gptr = np.concatenate([[0], np.cumsum([len(members[kk]) for kk in keys])]).astype(np.int32)
    return perm, gptr, labels


def padded_groups(G: int) -> int:
    """Gp: column 0 (the state weight) + G groups, padded to whole 16-column MFMA tiles"""
    return -(-(1 + int(G)) // 16) * 16


# ------------------------------------------------------------------------------------------------ the two steps: HIP kernels or torch
def _use_kernels(t: torch.Tensor) -> bool:
    return t.is_cuda and os.environ.get("HG_DOS", "").lower() != "torch"


def _mulliken_torch(C, SC, perm, gptr, wk, Gp):
    """ops.mulliken_weights in torch ops: the terms Re(conj(c) S c) times the 0 / 1 matrix [M, Gp] of the groups (one matmul: a fixed order)"""
    ns, M = C.shape
    G = int(gptr.shape[0]) - 1
    P = torch.zeros(M, Gp, device=C.device, dtype=torch.float32)
    if G > 0:
        col = torch.repeat_interleave(torch.arange(1, G + 1, device=C.device), (gptr[1:] - gptr[:-1]).long())
        P[perm.long(), col] = 1.0
    W = (C.real * SC.real + C.imag * SC.imag).float() @ P
    W *= wk[:, None]
    W[:, 0] = wk
    return W


def _broaden_torch(eps, W, E0, dE, ne, sigma, D=None, accumulate=False, max_elems=1 << 26):
    """ops.dos_broaden in torch ops, untruncated: exp of an [energies, states] matrix (E - eps in double, rounded once) + one matmul, in chunks of energies"""
    ns, Gp = W.shape
    out = D if accumulate else torch.empty(ne, Gp, device=W.device, dtype=torch.float32)
    E = E0 + dE * torch.arange(ne, device=W.device, dtype=torch.float64)
    step = max(1, min(ne, max_elems // max(1, ns)))
    norm = 1.0 / (sigma * math.sqrt(2.0 * math.pi))
    for j0 in range(0, ne, step):
        x = ((E[j0:j0 + step, None] - eps.double()[None, :]) / sigma).float()
        part = (torch.exp(-0.5 * x * x) * norm) @ W
        if accumulate:
            out[j0:j0 + step] += part
        else:
            out[j0:j0 + step] = part
    return out


def state_weights(C, SC, perm, gptr, wk, Gp):
    """W [ns, Gp] fp32 of the states whose eigenvector rows are C [ns, M] complex64 and whose S(k) c rows are SC: column 0 = wk, column 1 + g = wk * the
    Mulliken weight of group g (perm / gptr int32 from group_map), pad columns 0.  HIP kernel hg_mulliken_weights, or torch ops (see _use_kernels)."""
    return ops.mulliken_weights(C, SC, perm, gptr, wk, Gp) if _use_kernels(C) else _mulliken_torch(C, SC, perm, gptr, wk, Gp)


def broaden(eps, W, E0, dE, ne, sigma, D=None, accumulate=False):
    """D [ne, Gp] (+)= Gaussians of width sigma around the ASCENDING eps [ns] weighted by W [ns, Gp] on the grid E0 + j dE.  accumulate adds to the given D,
    so the states of k-chunks can be added in turn, in a fixed order.  HIP kernel hg_dos_broaden, or torch ops (see _use_kernels)."""
    fn = ops.dos_broaden if _use_kernels(W) else _broaden_torch
    return fn(eps, W, E0, dE, ne, sigma, D=D, accumulate=accumulate)


# ------------------------------------------------------------------------------------------------ the linear tetrahedron method
def _tetra_corner_weights(es, E, v, dE, g_lo, g_hi, mode):
    """the rules of tetra_dos's docstring on fp64 tensors: es [..., 4] ascending corner energies, E broadcastable to es[..., 0] -> [..., 4] weights of
    the sorted corners.  Every branch is computed everywhere on denominators made safe (1 where the branch's interval is empty) and selected after."""
    e1, e2, e3, e4 = es.unbind(-1)
    E = E + torch.zeros_like(e1)
    q, one, zero = 0.25 * v, torch.ones_like(e1), torch.zeros_like(E)
    safe = lambda x: torch.where(x > 0, x, one)
    e21, e31, e41, e32, e42, e43 = safe(e2 - e1), safe(e3 - e1), safe(e4 - e1), safe(e3 - e2), safe(e4 - e2), safe(e4 - e3)
    a, b, c, d = E - e1, E - e2, e3 - E, e4 - E
    f2, f3, f4 = a / e21, a / e31, a / e41                   # e1 < E < e2
    h1, h2, h3 = d / e41, d / e42, d / e43                   # e3 <= E < e4
    C1, C2, C3 = q * a * a / (e41 * e31), q * a * b * c / (e41 * e32 * e31), q * b * b * d / (e42 * e32 * e41)
    if mode:
        C = q * f2 * f3 * f4
        low = (C * (4.0 - (f2 + f3 + f4)), C * f2, C * f3, C * f4)
        C = q * h1 * h2 * h3
        high = (q - C * h1, q - C * h2, q - C * h3, q - C * (4.0 - (h1 + h2 + h3)))
        mid = (C1 + (C1 + C2) * c / e31 + (C1 + C2 + C3) * d / e41, C1 + C2 + C3 + (C2 + C3) * c / e32 + C3 * d / e42,
               (C1 + C2) * a / e31 + (C2 + C3) * b / e32, (C1 + C2 + C3) * a / e41 + C3 * b / e42)
        above = q + zero
    else:
        P = v * f2 * f3 / e41
        low = (P * (3.0 - (f2 + f3 + f4)), P * f2, P * f3, P * f4)
        P = v * h1 * h2 / e43
        high = (P * h1, P * h2, P * h3, P * (3.0 - (h1 + h2 + h3)))
        D1, D2, D3 = 2.0 * q * a / (e41 * e31), q * (b * c + a * c - a * b) / (e41 * e32 * e31), q * (2.0 * b * d - b * b) / (e42 * e32 * e41)
        mid = (D1 + ((D1 + D2) * c - (C1 + C2)) / e31 + ((D1 + D2 + D3) * d - (C1 + C2 + C3)) / e41,
               D1 + D2 + D3 + ((D2 + D3) * c - (C2 + C3)) / e32 + (D3 * d - C3) / e42,
               ((D1 + D2) * a + (C1 + C2)) / e31 + ((D2 + D3) * b + (C2 + C3)) / e32,
               ((D1 + D2 + D3) * a + (C1 + C2 + C3)) / e41 + (D3 * b + C3) / e42)
        above = zero
    m = 0.25 * (((e1 + e2) + e3) + e4)
    flat = (q * (E >= m).to(e1.dtype)) if mode else torch.where((m >= g_lo) & (m <= g_hi), q * torch.clamp(1.0 - (E - m).abs() / dE, min=0.0) / dE, zero)
    is_flat = (e4 - e1) < dE
    out = []
    for i in range(4):
        w = torch.where(E < e2, low[i], torch.where(E >= e3, high[i], mid[i]))
        w = torch.where(E <= e1, zero, torch.where(E >= e4, above, w))
        out.append(torch.where(is_flat, flat + zero, w))
    return torch.stack(out, -1)


def _tetra_torch(eps, W, tet, E0, dE, ne, mode, D=None, accumulate=False, max_elems=1 << 22):
    """ops.dos_tetra in torch ops: the corner weights of every (energy, tetrahedron, band) in fp64, added into A [energies, nk nb] at the corners'
    k-rows (index_add_), rounded to fp32 once, one matmul with W; in chunks of energies.  tet: int64 tensor [nt, 4] on eps's device."""
    nk, nb, Gp = W.shape
    nt = int(tet.shape[0])
    out = D if accumulate else torch.empty(ne, Gp, device=W.device, dtype=torch.float32)
    if nt == 0 or nk * nb == 0:
        return out if accumulate else out.zero_()
    es, order = torch.sort(eps.double()[tet], dim=1, stable=True)                                  # [nt, 4, nb]
    rows = (tet[:, :, None].expand(-1, -1, nb).gather(1, order) * nb + torch.arange(nb, device=W.device)).permute(0, 2, 1).reshape(-1)
    es = es.permute(0, 2, 1)                                                                       # [nt, nb, 4]
    E = E0 + dE * torch.arange(ne, device=W.device, dtype=torch.float64)
    step = max(1, min(ne, max_elems // max(1, nt * nb)))
    W2 = W.reshape(nk * nb, Gp)
    for j0 in range(0, ne, step):
        Ej = E[j0:j0 + step]
        w = _tetra_corner_weights(es[None], Ej[:, None, None], 1.0 / nt, dE, E0, E0 + (ne - 1) * dE, mode)      # [step, nt, nb, 4]
        A = torch.zeros(Ej.shape[0], nk * nb, device=W.device, dtype=torch.float64).index_add_(1, rows, w.reshape(Ej.shape[0], -1))
        part = A.float() @ W2
        if accumulate:
            out[j0:j0 + step] += part
        else:
            out[j0:j0 + step] = part
    return out


_TABLES = {}


def _tetra_tables(tet, nk, device):
    """(tet int32 [nt, 4], (kt_ptr, kt_tet, kt_corner), tet int64) on the device, cached by the content of tet (checked against nk once)"""
    tet = np.ascontiguousarray(tet.cpu().numpy() if isinstance(tet, torch.Tensor) else tet, dtype=np.int32)
    key = (tet.shape, hash(tet.tobytes()), int(nk), str(device))
    if key not in _TABLES:
        if len(_TABLES) >= 8:
            _TABLES.clear()
        kt = corner_table(tet, nk)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        _TABLES[key] = (dev(tet), tuple(dev(a) for a in kt), dev(tet.astype(np.int64)))
    return _TABLES[key]


def _tetra(eps, W, tet, E0, dE, ne, mode, D, accumulate):
    if eps.dim() != 2 or W.dim() != 3 or tuple(W.shape[:2]) != tuple(eps.shape):
        raise ValueError(f"tetra_dos: eps must be [nk, nb] and W [nk, nb, Gp], got {tuple(eps.shape)}, {tuple(W.shape)}")
    if not dE > 0:
        raise ValueError(f"tetra_dos: the grid step must be positive, got {dE!r}")
    if accumulate and D is None:
        raise ValueError("tetra_dos: accumulate needs the D to add to")
    tet32, kt, tet64 = _tetra_tables(tet, int(eps.shape[0]), W.device)
    if not _use_kernels(W):
        return _tetra_torch(eps, W, tet64, float(E0), float(dE), int(ne), mode, D=D, accumulate=accumulate)
    if eps.numel() == 0:
        band_lo = band_hi = torch.zeros(int(eps.shape[1]), device=W.device, dtype=torch.float32)
    else:
        band_lo, band_hi = eps.amin(0), eps.amax(0)
    return ops.dos_tetra(eps, W, tet32, kt, band_lo, band_hi, E0, dE, ne, mode=mode, D=D, accumulate=accumulate)


def tetra_dos(eps, W, tet, E0, dE, ne, D=None, accumulate=False):
    """D [ne, Gp] (+)= the DOS / PDOS by the linear tetrahedron method (Bloechl, Jepsen, Andersen 1994) on the grid E0 + j dE.  eps [nk, nb] fp32, ascending
    in b at every k (the solver's order); W [nk, nb, Gp] fp32: the rows of state_weights(..., wk = ones, ...) of state (k, b), unsorted; tet int32 [nt, 4]
    from tetrahedra() for the k-list eps and W are on (numpy or tensor; its corner table is built once and cached).  No width parameter; the result is per
    k-point average (integral over the Brillouin zone = 1 per band).  accumulate adds to the given D, so band chunks can be fed in turn, in a fixed order;
    all k-points of a band chunk must be present at once.  HIP kernel hg_dos_tetra, or torch ops (see _use_kernels).

    The weights.  Inside a tetrahedron of weight v = 1 / nt the band energy and the projection weight are linear.  Corner energies sorted
    e1 <= e2 <= e3 <= e4 (ties: the lower corner slot first), e_ij = e_i - e_j, q = v / 4, a = E - e1, b = E - e2, c = e3 - E, d = e4 - E.
    DOS of the tetrahedron g_T: 0 outside [e1, e4]; 3 v a^2 / (e21 e31 e41); v / (e31 e41) [3 e21 + 6 b - 3 (e31 + e42) b^2 / (e32 e42)];
    3 v d^2 / (e41 e42 e43) in the three intervals.  Corner weight c_i(E) = g_T(E) x the barycentric coordinate i of the centroid of the cross-section at
    E (a triangle in the outer intervals, a quadrilateral in the middle one: the area-weighted centroid of its two triangles), sum_i c_i = g_T; the
    number-of-states weights w_i (tetra_states) are their integrals, Bloechl's integration weights:
      E <= e1: 0.  E >= e4: c_i = 0, w_i = q.
      e1 < E < e2:  f_j = a / e_j1, P = v f2 f3 / e41: c_1 = P (3 - f2 - f3 - f4), c_j = P f_j;  C = q f2 f3 f4: w_1 = C (4 - f2 - f3 - f4), w_j = C f_j.
      e2 <= E < e3: C1 = q a^2 / (e41 e31), C2 = q a b c / (e41 e32 e31), C3 = q b^2 d / (e42 e32 e41);
                    w_1 = C1 + (C1 + C2) c / e31 + (C1 + C2 + C3) d / e41,  w_2 = C1 + C2 + C3 + (C2 + C3) c / e32 + C3 d / e42,
                    w_3 = (C1 + C2) a / e31 + (C2 + C3) b / e32,            w_4 = (C1 + C2 + C3) a / e41 + C3 b / e42;  c_i = d w_i / dE term by term.
      e3 <= E < e4: h_j = d / e_4j, P = v h1 h2 / e43: c_4 = P (3 - h1 - h2 - h3), c_j = P h_j;  C = q h1 h2 h3: w_4 = q - C (4 - h1 - h2 - h3), w_j = q - C h_j.
    A branch is evaluated only where its interval is not empty, so no 0 / 0 is formed.
    The flat rule.  A tetrahedron with e4 - e1 < dE (all four equal included: every tetrahedron of a 1 x 1 x 1 grid) is a delta function at the mean m of
    its corner energies.  DOS: its weight is shared linearly between the two grid energies that bracket m (cloud-in-cell), q max(0, 1 - |E_j - m| / dE) / dE
    per corner; a flat tetrahedron whose mean lies outside [E0, E0 + (ne - 1) dE] contributes nothing.  Number of states: a step at m, q per corner where
    E_j >= m.  This is what makes the sum rule hold for flat bands.  Everything is evaluated in double from the fp32 eigenvalues and rounded to fp32 once."""
    return _tetra(eps, W, tet, E0, dE, ne, 0, D, accumulate)


def tetra_states(eps, W, tet, E0, dE, ne, D=None, accumulate=False):
    """N [ne, Gp] (+)= the number of states below E0 + j dE and its projections by the linear tetrahedron method: tetra_dos with the integration weights
    w_i in place of c_i (see there, the flat rule included).  At an energy above every eigenvalue N[j] = sum_{k, b} W[k, b] / nk exactly (to rounding)."""
    return _tetra(eps, W, tet, E0, dE, ne, 1, D, accumulate)


# ------------------------------------------------------------------------------------------------ host helpers
def _plateau_level(count, lo0, hi0, nel):
    """the level in [lo0, hi0] at which the non-decreasing count(mu) = nel, by bisection in fp64.  Where the count is flat every level of the plateau
    holds nel to the tolerance 1e-12 max(1, nel): the mean of the plateau's two ends is returned."""
    tol = 1e-12 * max(1.0, nel)
    if not count(lo0) - tol <= nel <= count(hi0) + tol:
        raise ValueError(f"{nel} electrons do not fit {count(hi0):.3f} states")

    def edge(target, below):                                   # the first level whose count reaches (below) / exceeds (not below) the target
        lo, hi = lo0, hi0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if (count(mid) < target) if below else (count(mid) <= target):
                lo = mid
            else:
                hi = mid
            if hi - lo <= 1e-13 * max(1.0, abs(mid)):
                break
        return 0.5 * (lo + hi)
    return 0.5 * (edge(nel - tol, True) + edge(nel + tol, False))


def fermi_level(eps, w, nel, sigma, deg):
    """the level mu at which deg * sum_s w_s erfc((eps_s - mu) / (sigma sqrt 2)) / 2 = nel; bisection in fp64 on the host.  Where the count is flat
    (a gap much wider than sigma) every level of the plateau holds nel to rounding: the middle of the plateau is returned."""
    eps_t, w_t = torch.from_numpy(np.asarray(eps, dtype=np.float64)), torch.from_numpy(np.asarray(w, dtype=np.float64))
    count = lambda mu: deg * float((w_t * 0.5 * torch.erfc((eps_t - mu) / (sigma * math.sqrt(2.0)))).sum())
    return _plateau_level(count, float(eps_t.min()) - 10.0 * sigma, float(eps_t.max()) + 10.0 * sigma, nel)


def fermi_level_tetra(eps, tet, nel, deg):
    """the level mu at which deg * (the tetrahedron method's number of states at mu) = nel, for eps [nk, nb] on the k-list of tet: bisection in fp64 on
    the host on the closed form n_T(E) = v a^3 / (e21 e31 e41);  v / (e31 e41) [e21^2 + 3 e21 b + 3 b^2 - (e31 + e42) b^3 / (e32 e42)];
    v (1 - d^3 / (e41 e42 e43)) in the three intervals (the sums of tetra_dos's w_i; a tetrahedron with four equal corners is a step).  Where the count is
    flat (a gap) every level of the plateau holds nel: the middle of the plateau is returned, as fermi_level does."""
    eps, tet = np.asarray(eps, dtype=np.float64), np.asarray(tet, dtype=np.int64)
    es = np.sort(eps[tet], axis=1)                                         # [nt, 4, nb]
    e1, e2, e3, e4 = es[:, 0], es[:, 1], es[:, 2], es[:, 3]
    safe = lambda x: np.where(x > 0, x, 1.0)
    e21, e31, e41, e32, e42, e43 = safe(e2 - e1), safe(e3 - e1), safe(e4 - e1), safe(e3 - e2), safe(e4 - e2), safe(e4 - e3)

    def count(mu):
        a, b, d = mu - e1, mu - e2, e4 - mu
        n = np.where(mu < e2, a ** 3 / (e21 * e31 * e41),
                     np.where(mu >= e3, 1.0 - d ** 3 / (e41 * e42 * e43),
                              ((e2 - e1) ** 2 + 3.0 * (e2 - e1) * b + 3.0 * b * b - (e31 + e42) * b ** 3 / (e32 * e42)) / (e31 * e41)))
        return deg * float(np.where(mu >= e4, 1.0, np.where(mu <= e1, 0.0, n)).sum()) / tet.shape[0]

    lo0, hi0 = float(eps.min()), float(eps.max())
    mu, tol = _plateau_level(count, lo0, hi0, nel), 1e-12 * max(1.0, nel)      # (its tolerance on the count)
    # the count leaves a plateau like a cube, so the bisection finds its ends only to the cube root of tol: a plateau ends at eigenvalues, take those
    below, above = eps[eps <= mu], eps[eps >= mu]
    a, b = float(below.max()) if below.size else lo0, float(above.min()) if above.size else hi0
    return 0.5 * (a + b) if count(b) - count(a) <= 4.0 * tol else mu


def energy_grid(erange_eV, ne, sigma, emin=0.0, emax=0.0):
    """(E0, dE) of ne energies over erange_eV, or over the whole spectrum [emin, emax] +- 8 sigma when it is None.  A step above sigma is refused: with
    dE <= sigma the sum over the grid integrates a Gaussian to 3e-9, which sum rules rely on."""
    ne = int(ne)
    if ne < 2:
        raise ValueError("energy_grid: at least two energies")
    lo, hi = (emin - PAD_SIGMAS * sigma, emax + PAD_SIGMAS * sigma) if erange_eV is None else (float(erange_eV[0]), float(erange_eV[1]))
    if not hi > lo:
        raise ValueError(f"energy_grid: empty energy range {erange_eV!r}")
    dE = (hi - lo) / (ne - 1)
    if dE > sigma:
        raise ValueError(f"energy_grid: the grid step {dE:.4g} eV is above sigma_eV = {sigma:.4g}: the sum over the grid no longer integrates a "
                         f"Gaussian (use ne >= {int(math.ceil((hi - lo) / sigma)) + 1} or a larger sigma_eV)")
    return lo, dE
