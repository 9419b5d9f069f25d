"""The one-particle density matrix on a k-grid, in real space and only where the crystal graph has rows: P_on [N, nao^2] and P_off [E, nao^2] in the layout of
the rows the head emits.  The integrated counterpart of dos.py (states by energy) and bonds.py (states by bond), and a post-solver part like them: it takes
the solver's eigenvectors.  What it is for: the restart / initial guess a DFT code reads; Mulliken charges and overlap / Hamilton populations per bond
without an energy grid; and, by Hellmann-Feynman, the gradient of sum_s f_s eps_s with respect to the Hamiltonian rows.

    tables = bonds.bond_tables(head, z, edge_index, cell_shift, device)     # the tables of bonds.py, reused
    mu  = dos.fermi_level(eps, w, nel, sigma, deg=2)                        # eps [nk, nb] fp64 on the host, w = k-weights per state
    occ = occupations(eps, mu, sigma, deg=2)                                # sum(w * occ) = nel
    f   = (w * occ).reshape(-1)  -> fp32 on the device                      # one real weight per state; f * eps for the energy-weighted density matrix
    P_on, P_off = density_rows(C, kidx, kvec, f, tables)                    # C [ns, M] complex64, kidx int32 [ns] -> rows of kvec fp32 [nk, 3]
    density_rows(C2, kidx2, kvec, f2, tables, out=(P_on, P_off), accumulate=True)      # eigenvector chunks in turn, as the solver hands them out
    q_atom, q_orb = populations(P_on, P_off, Son, Soff, tables)             # overlap rows: Mulliken gross populations
    icohp = bond_populations(P_on, P_off, Hon, Hoff, bonds.bond_groups(...))# Hamiltonian rows: ICOHP at these occupations; overlap rows: overlap populations

The quantity, with mu(i, a) = ooff[i] + orank[i][a] the compact orbital index of hg_hk_assemble and the edge convention of kspace.assemble_k
(H(k)[(i a), (j b)] += exp(2 pi i k . shift_e) X_off[e][a, b], i = erow[e], j = ecol[e]):
    P_off[e][a, b] = sum_s f_s Re(exp(2 pi i k_s . shift_e) conj(C[s, mu(i, a)]) C[s, mu(j, b)])
    P_on [i][a, b] = sum_s f_s Re(conj(C[s, mu(i, a)]) C[s, mu(i, b)])
and exactly 0 where either atom lacks the orbital.  The real part is the right one for real rows on a time-reversal-folded grid
(dos.monkhorst_pack(time_reversal=True)): the state at -k is the complex conjugate, so a weight that counts both members of a pair gives twice the real
part and the imaginary parts cancel.  By construction sum_ab X_off[e][a, b] P_off[e][a, b] = sum_s f_s t_e(s), t_e the bond term of bonds.py, and
(P_on, P_off) = kspace.assemble_k_adjoint(G) of G_k[p, q] = sum_{s at k} f_s C[s, p] conj(C[s, q]): the dense P(k) is never formed (M^2 complex
elements and 8 M^2 ns flops per k-point, whatever the sparsity), the work grows with the number of rows.

`density_rows` runs the HIP kernel hg_density_rows (csrc/spectra.hip: an SDDMM on fp32 MFMA, one workgroup per edge / atom, no atomics, bit-reproducible)
on CUDA tensors; CPU tensors, and HG_DOS=torch on the GPU (the switch of dos._use_kernels), take a plain torch path (chunked gathers + einsum), the
baseline of tests/bench_density.py.

Out of scope: spin-orbit rows, several weight vectors in one launch (call twice), tetrahedron occupation weights, batches of several crystals (one call
per crystal), and any driver that runs the eigen-solver.  Edge-sharded graphs: a rank's rows P_off of its own edges are complete, but its on-site rows
P_on are complete only on the rank that holds all states -- the rows of different ranks' STATE chunks add, the rows of different ranks' EDGES do not
overlap.  Collinear spin is the spin-free call once per channel."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import dos, ops
from .bonds import group_tensors
from .kspace import edge_phases, padded_rows


def occupations(eps, mu, sigma, deg=2):
    """deg / 2 erfc((eps - mu) / (sigma sqrt 2)) in fp64: the occupation of a state under Gaussian smearing, exactly the count dos.fermi_level bisects on, so
    sum_s w_s occupations(eps, mu, sigma, deg)[s] = nel at its mu.  eps: a tensor (the result is a float64 tensor on its device) or array-like (numpy)."""
    if isinstance(eps, torch.Tensor):
        return deg * 0.5 * torch.erfc((eps.to(torch.float64) - mu) / (sigma * math.sqrt(2.0)))
    e = torch.from_numpy(np.ascontiguousarray(np.asarray(eps, dtype=np.float64)))
    return (deg * 0.5 * torch.erfc((e - mu) / (sigma * math.sqrt(2.0)))).numpy()


# ------------------------------------------------------------------------------------------------ the rows: HIP kernel or torch
def _density_rows_torch(C, kidx, kvec, f, erow, ecol, shift, orank, ooff, out=None, accumulate=False, max_elems=1 << 24):
    """ops.density_rows in torch ops, in the precision of C (complex64 or complex128): the rows of C gathered per atom into the nao-padded layout (0 where the
    atom lacks the orbital), the row operand scaled by f, then per chunk of edges the column operand times the phase (k . shift in double, rounded once) and
    two real einsums over the states"""
    ns = int(C.shape[0])
    N, nao = orank.shape
    E = int(erow.shape[0])
    rdt = C.real.dtype
    CA, _ = padded_rows(C, orank, ooff)                                                               # [ns, N, nao]
    fx, fy = CA.real * f.to(rdt)[:, None, None], CA.imag * f.to(rdt)[:, None, None]
    P_on = (torch.einsum("sia,sib->iab", fx, CA.real) + torch.einsum("sia,sib->iab", fy, CA.imag)).reshape(N, nao * nao)
    P_off = torch.empty(E, nao * nao, device=C.device, dtype=rdt)
    step = max(1, max_elems // max(1, ns * nao))
    kd = kvec.double()[kidx.long()]                                                                   # [ns, 3]
    for q0 in range(0, E, step):
        i, j = erow[q0:q0 + step].long(), ecol[q0:q0 + step].long()
        B = edge_phases(kd, shift[q0:q0 + step], rdt)[:, :, None] * CA[:, j]                          # [ns, members, nao]
        P_off[q0:q0 + step] = (torch.einsum("sea,seb->eab", fx[:, i], B.real) + torch.einsum("sea,seb->eab", fy[:, i], B.imag)).reshape(-1, nao * nao)
    if out is None:
        return P_on, P_off
    if accumulate:
        out[0].add_(P_on)
        out[1].add_(P_off)
    else:
        out[0].copy_(P_on)
        out[1].copy_(P_off)
    return out[0], out[1]


def density_rows(C, kidx, kvec, f, tables, out=None, accumulate=False):
    """(P_on [N, nao^2], P_off [E, nao^2]) fp32: the density-matrix rows of the states whose eigenvector rows are C [ns, M] complex64 (S-normalised by the
    caller; kidx int32 [ns] -> rows of kvec fp32 [nk, 3]) with one real weight f fp32 [ns] per state -- k-weight x occupation, times eps for the
    energy-weighted matrix; it may be negative.  P = sum_s f_s Re(phase conj(c_ia) c_jb): the real part, which is the whole of it for real rows on a
    time-reversal-folded grid (dos.monkhorst_pack(time_reversal=True)) whose weights count both k and -k.  tables: bonds.bond_tables(...) on C's device.
    out = (P_on, P_off) to write into; accumulate=True adds to it (eigenvector chunks in turn; elements at missing orbitals stay as they are), otherwise
    every element is written, zeros at missing orbitals included.  On an edge-sharded graph a rank's P_off rows of its own edges are complete, its P_on rows
    cover its own states only.  Every argument is checked on the host before anything runs (ValueError naming it).  HIP kernel hg_density_rows, or torch ops
    (see dos._use_kernels)."""
    t = tables
    if isinstance(C, torch.Tensor) and C.dim() == 2 and int(C.shape[1]) != t.M:
        raise ValueError(f"density_rows: C has {int(C.shape[1])} orbital columns, the tables {t.M}")
    args = (C, kidx, kvec, f, t.erow, t.ecol, t.shift, t.orank, t.ooff)
    if isinstance(C, torch.Tensor) and dos._use_kernels(C):
        return ops.density_rows(*args, out=out, accumulate=accumulate)
    ops.density_rows_check(*args, out, accumulate)
    return _density_rows_torch(*args, out=out, accumulate=accumulate)


# ------------------------------------------------------------------------------------------------ populations
def _fixed_order_sum(index, src, n):
    """out[i] = sum of the rows src[q] with index[q] == i in a fixed order: ops.scatter_rows (stable sort + segmented sum) on the GPU, index_add_ on the CPU"""
    if src.is_cuda:
        return ops.scatter_rows(index, src, n, persistent=False)
    return src.new_zeros((n,) + tuple(src.shape[1:])).index_add_(0, index.long(), src)


def populations(P_on, P_off, X_on, X_off, tables):
    """(per_atom [N], per_orbital [N, nao]): gross populations on the row atom, per_orbital[i, a] = sum_b P_on[i][a, b] X_on[i][a, b] + sum_{e: erow[e] = i}
    sum_b P_off[e][a, b] X_off[e][a, b], per_atom its sum over a.  With overlap rows: the Mulliken populations (their total is sum_s f_s for S-normalised
    states); with Hamiltonian rows the atoms' shares of sum_s f_s eps_s.  Fixed-order sums: two calls are bit-identical."""
    nao = tables.nao
    N, E = int(P_on.shape[0]), int(P_off.shape[0])
    if tuple(P_on.shape) != (N, nao * nao) or tuple(X_on.shape) != (N, nao * nao) or tuple(P_off.shape) != (E, nao * nao) or tuple(X_off.shape) != (E, nao * nao) \
            or tuple(tables.erow.shape) != (E,):
        raise ValueError(f"populations: P_on / X_on must be [N, {nao * nao}], P_off / X_off [E, {nao * nao}] with the tables' {int(tables.erow.shape[0])} edges, got "
                         f"{tuple(P_on.shape)}, {tuple(X_on.shape)}, {tuple(P_off.shape)}, {tuple(X_off.shape)}")
    on = (P_on * X_on).reshape(N, nao, nao).sum(2)
    off = (P_off * X_off).reshape(E, nao, nao).sum(2)
    per_orbital = on + _fixed_order_sum(tables.erow, off, N)
    return per_orbital.sum(1), per_orbital


def bond_populations(P_on, P_off, X_on, X_off, groups):
    """[G]: sum over the members of every group of bonds.bond_groups (CSR lists eptr, eidx of edges and aptr, aidx of on-site blocks; numpy or tensors on the
    rows' device) of sum_ab P[a, b] X[a, b].  Overlap rows: the overlap population of the bond; Hamiltonian rows: ICOHP at the occupations that formed P.
    Over groups that hold every edge and every atom exactly once the total is sum_s f_s (overlap rows, S-normalised states) / sum_s f_s eps_s (Hamiltonian
    rows).  Fixed-order sums."""
    dev = P_on.device
    eptr, eidx, aptr, aidx = group_tensors(groups, dev)
    G = int(eptr.shape[0]) - 1
    if G < 0 or int(aptr.shape[0]) != G + 1:
        raise ValueError(f"bond_populations: eptr and aptr must both be [G + 1], got {tuple(eptr.shape)}, {tuple(aptr.shape)}")
    for name, idx, n in (("eidx", eidx, int(P_off.shape[0])), ("aidx", aidx, int(P_on.shape[0]))):
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError(f"bond_populations: {name} has entries outside [0, {n})")
    m_e, m_a = (P_off * X_off).sum(1), (P_on * X_on).sum(1)
    gid = lambda p: torch.repeat_interleave(torch.arange(G, device=dev), (p[1:] - p[:-1]).long())
    vals = torch.cat([m_e[eidx.long()], m_a[aidx.long()]])
    return _fixed_order_sum(torch.cat([gid(eptr), gid(aptr)]), vals[:, None], G)[:, 0]
