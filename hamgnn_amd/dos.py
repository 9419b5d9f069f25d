"""Density of states and its projections on a Brillouin-zone grid: the parts after the eigen-solver, and the grid.

    k_red, k_w = monkhorst_pack((8, 8, 8))                                  # Gamma-centred grid, k / -k folded
    perm, gptr, labels = group_map(head, z, "atom")                         # orbital groups of a projection in the compact orbital order
    W = state_weights(C, SC, perm_d, gptr_d, wk, padded_groups(len(labels)))    # Mulliken weights of the states of a k-chunk (C, S c rows)
    D = broaden(eps_sorted, W_sorted, E0, dE, ne, sigma, D=D, accumulate=D is not None)

`state_weights`: w = sum_{mu in g} Re(conj(c_mu) (S(k) c)_mu) by the HIP kernel `hg_mulliken_weights`; `broaden`: D[j, g] = sum_s A(E_j, eps_s) W[s, g] by
the HIP kernel `hg_dos_broaden` (csrc/spectra.hip), which generates the Gaussians in registers from the sorted eigenvalues and adds chunks into D in the
order given.  CPU tensors, and HG_DOS=torch on the GPU, take a plain torch path for the two steps (`exp` of an [energies, states] matrix in chunks + matmul;
group sums as one matmul with the 0 / 1 group matrix): the CPU route, and the baseline of tests/bench_dos.py.  `fermi_level`, `energy_grid`: host, fp64.

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
    key = lambda v: tuple(int(t) for t in np.rint((v - np.floor(v + 1e-12)) * 2 ** 40) % 2 ** 40)      # k modulo 1 on a 2^-40 lattice
    seen, keep, weight = {}, [], []
    for i in range(k.shape[0]):
        me, partner = key(k[i]), key(-k[i])
        if partner in seen and partner != me:
            weight[seen[partner]] += w[i]
            continue
        seen[me] = len(keep)
        keep.append(i)
        weight.append(w[i])
    return k[keep], np.asarray(weight)


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


# ------------------------------------------------------------------------------------------------ host helpers
def fermi_level(eps, w, nel, sigma, deg):
    """the level mu at which deg * sum_s w_s erfc((eps_s - mu) / (sigma sqrt 2)) / 2 = nel; bisection in fp64 on the host.  Where the count is flat
    (a gap much wider than sigma) every level of the plateau holds nel to rounding: the middle of the plateau is returned."""
    eps_t, w_t = torch.from_numpy(np.asarray(eps, dtype=np.float64)), torch.from_numpy(np.asarray(w, dtype=np.float64))
    count = lambda mu: deg * float((w_t * 0.5 * torch.erfc((eps_t - mu) / (sigma * math.sqrt(2.0)))).sum())
    lo0, hi0 = float(eps_t.min()) - 10.0 * sigma, float(eps_t.max()) + 10.0 * sigma
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
