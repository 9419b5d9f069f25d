"""Bond-resolved state weights on a k-grid: COOP (crystal orbital overlap population), COHP (crystal orbital Hamilton population) and the integrated ICOHP
from the real-space rows the head emits -- which bonds the states are in, and whether they are bonding or antibonding there.  A post-solver part like dos.py:
it takes the solver's eigenvectors and hands dos.py's kernels their weight rows.

    groups = bond_groups(edge_index, cell_shift, z, by="pair")              # host: which edges / atoms make up a bond (CSR lists + labels)
    tables = bond_tables(head, z, edge_index, cell_shift, device)           # device: kspace.CrystalTables (row / column atom and shift per edge, orank, ooff, M)
    Gp = dos.padded_groups(len(groups[4]))
    W_S = bond_weights(C, kidx, kvec, Son, Soff, tables, groups, wk, Gp)    # overlap rows: COOP weights
    W_H = bond_weights(C, kidx, kvec, Hon, Hoff, tables, groups, wk, Gp)    # Hamiltonian rows: COHP weights
    coop  = dos.tetra_dos(eps, W_S.reshape(nk, nb, Gp), tet, E0, dE, ne)    # (wk = ones: the tetrahedra carry the k-weights)
    cohp  = dos.tetra_dos(eps, W_H.reshape(nk, nb, Gp), tet, E0, dE, ne)
    icohp = dos.tetra_states(eps, W_H.reshape(nk, nb, Gp), tet, E0, dE, ne)
    (or dos.broaden on the sorted states, wk = the k-weights)

The quantity, for state s (row s of C [ns, M] complex64, at k-point kvec[kidx[s]]) and the compact orbital index mu(i, a) = ooff[i] + orank[i][a] of
hg_hk_assemble:  t_e(s) = Re(exp(2 pi i k_s . shift_e) sum_{a, b} conj(C[s, mu(i, a)]) X_off[e][a, b] C[s, mu(j, b)]) for the directed edge e from its row atom
i = edge_index[0][e] to its column atom j = edge_index[1][e] (the convention of kspace.assemble_k: H(k)[i a, j b] += phase X_off[e][a, b]), and o_i(s) the same
with the on-site block X_on[i] and no phase;  W[s, 0] = wk[s], W[s, 1 + g] = wk[s] (sum of t_e over the edges of group g + sum of o_i over its atoms), pad
columns 0.  If every edge and every atom is in exactly one group, sum_g W[s, 1 + g] = wk[s] Re(c_s^+ X(k_s) c_s): wk[s] for overlap rows and S-normalised
states, wk[s] eps_s for Hamiltonian rows.  Units are those of the rows.  Sign convention: a bonding state lowers the energy, so NEGATIVE COHP means
bonding and positive antibonding (plots usually show -COHP); COOP is positive for bonding.

kvec and the shifts only enter through k . shift: reduced k-points with integer cell shifts (what bond_groups reads), or the Cartesian pair of
kspace.assemble_k (data.k_vecs, data.nbr_shift).  `bond_weights` runs the HIP kernel hg_bond_weights (csrc/spectra.hip) on CUDA tensors; CPU tensors, and
HG_DOS=torch on the GPU (the switch of dos._use_kernels), take a plain torch path (chunked gathers + einsum), the baseline of tests/bench_bonds.py.

Out of scope: spin-orbit rows ((2 nao)^2: four spin blocks per bond), batches of several crystals (one call per crystal), edge-sharded graphs (a rank's
weights are partial sums over its own edges), and any driver that runs the eigen-solver.  Collinear spin is the spin-free call once per channel."""
from __future__ import annotations

import numpy as np
import torch

from . import dos, ops
from .basis import orbital_rank_table
from .kspace import CrystalTables, edge_phases, padded_rows

BY = ("edge", "pair", "species_pair")


# ------------------------------------------------------------------------------------------------ bond groups (host)
def _np(a, dtype):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def bond_groups(edge_index, nbr_shift, z, by="pair", onsite=True, pos=None, cell=None, rmax=None):
    """(eptr int32 [G + 1], eidx int32, aptr int32 [G + 1], aidx int32, labels [G]): the bond groups of one crystal as two CSR lists, edges and atoms
    (on-site blocks), whose member order is the summation order.  edge_index [2, E] (row atom, column atom), nbr_shift [E, 3] integer cell shifts, z [N].
      by="edge":  a directed edge (i, j, shift) and its inverse (j, i, -shift) form one group -- self-image edges (i, i, +-shift) pair up the same way, an edge
                  without an inverse stands alone; groups in the order of their first edge.  Label (sym_i, i, sym_j, j, shift) of the group's first edge.
      by="pair":  all edges between the atoms i <= j, over all images and both directions; ascending (i, j).  Label (sym_i, i, sym_j, j).
      by="species_pair": all edges between two elements; ascending unordered (Z_i, Z_j).  Label (sym_a, sym_b).
    onsite=True appends one group per atom, label (sym, i) (per element for "species_pair", label (sym,)) that holds the on-site blocks: then every atom is in
    exactly one group, and so is every edge unless rmax drops it.  rmax: edges longer than rmax (|pos[j] + shift @ cell - pos[i]|, in the length unit of
    pos and cell) are in no group; needs pos [N, 3] and cell [3, 3].  With pos and cell every edge-group label ends with the length of its shortest edge."""
    if by not in BY:
        raise ValueError(f"bond_groups: by={by!r}: one of {BY}")
    ei, sh, zs = _np(edge_index, np.int64), _np(nbr_shift, np.float64), _np(z, np.int64).reshape(-1)
    if ei.ndim != 2 or ei.shape[0] != 2 or sh.shape != (ei.shape[1], 3):
        raise ValueError(f"bond_groups: edge_index must be [2, E] and nbr_shift [E, 3], got {ei.shape}, {sh.shape}")
    if sh.size and np.abs(sh - np.rint(sh)).max() > 0:
        raise ValueError("bond_groups: nbr_shift must hold integer cell shifts (the graph's cell_shift, not its Cartesian nbr_shift)")
    N, E = len(zs), ei.shape[1]
    if E and (ei.min() < 0 or ei.max() >= N):
        raise ValueError(f"bond_groups: edge_index has entries outside [0, {N})")
    if (pos is None) != (cell is None):
        raise ValueError("bond_groups: pos and cell go together")
    if rmax is not None and pos is None:
        raise ValueError("bond_groups: rmax needs pos and cell (the edge lengths)")
    length = None
    if pos is not None:
        p, c = _np(pos, np.float64).reshape(N, 3), _np(cell, np.float64).reshape(3, 3)
        length = np.linalg.norm(p[ei[1]] + sh @ c - p[ei[0]], axis=1)
    shi = np.rint(sh).astype(np.int64)
    sym = lambda Z: dos.SYMBOLS[int(Z)]
    members, keys = {}, []
    for e in range(E):
        if rmax is not None and length[e] > rmax:
            continue
        i, j, s = int(ei[0, e]), int(ei[1, e]), tuple(int(v) for v in shi[e])
        if by == "edge":
            key = min((i, j, s), (j, i, tuple(-v for v in s)))
        elif by == "pair":
            key = (min(i, j), max(i, j))
        else:
            key = (min(int(zs[i]), int(zs[j])), max(int(zs[i]), int(zs[j])))
        if key not in members:
            members[key] = []
            keys.append(key)
        members[key].append(e)
    if by != "edge":
        keys.sort()
    labels = []
    for key in keys:
        if by == "edge":
            e = members[key][0]
            lab = (sym(zs[ei[0, e]]), int(ei[0, e]), sym(zs[ei[1, e]]), int(ei[1, e]), tuple(int(v) for v in shi[e]))
        elif by == "pair":
            lab = (sym(zs[key[0]]), key[0], sym(zs[key[1]]), key[1])
        else:
            lab = (sym(key[0]), sym(key[1]))
        labels.append(lab if length is None else lab + (float(length[members[key]].min()),))
    elists = [members[key] for key in keys]
    alists = [[] for _ in keys]
    if onsite:
        if by == "species_pair":
            for Z in sorted(set(int(v) for v in zs)):
                alists.append([i for i in range(N) if int(zs[i]) == Z])
                labels.append((sym(Z),))
        else:
            for i in range(N):
                alists.append([i])
                labels.append((sym(zs[i]), i))
        elists += [[] for _ in range(len(alists) - len(elists))]
    csr = lambda lists: (np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32),
                         np.asarray([x for v in lists for x in v], dtype=np.int32))
    eptr, eidx = csr(elists)
    aptr, aidx = csr(alists)
    return eptr, eidx, aptr, aidx, labels


# ------------------------------------------------------------------------------------------------ device tables
def bond_tables(head, z, edge_index, nbr_shift, device):
    """The kspace.CrystalTables of one crystal on `device`, as hg_bond_weights and hg_density_rows read them: erow / ecol = edge_index[0] / [1], orank from the
    head's basis (basis.orbital_rank_table, the table HamGNNPlusPlusOut.compile uploads; the head need not be compiled), ooff, M, and `nbr_shift` as given --
    integer cell shifts for reduced k-points, or the Cartesian pair of the assembly."""
    zs = _np(z, np.int64).reshape(-1)
    missing = sorted({int(Z) for Z in zs if int(Z) not in head.basis_def})
    if missing:
        raise ValueError(f"bond_tables: the head's basis has no element {missing}")
    ei = _np(edge_index, np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2 or (ei.size and (ei.min() < 0 or ei.max() >= len(zs))):
        raise ValueError(f"bond_tables: edge_index must be [2, E] with entries in [0, {len(zs)}), got {ei.shape}")
    sh = _np(nbr_shift, np.float32).reshape(-1, 3)
    if sh.shape[0] != ei.shape[1]:
        raise ValueError(f"bond_tables: nbr_shift must be [{ei.shape[1]}, 3], got {sh.shape}")
    return CrystalTables.from_edges(ei, sh, zs, orbital_rank_table(head.basis_def, int(head.nao_max)), device)


# ------------------------------------------------------------------------------------------------ the weights: HIP kernel or torch
def _bond_weights_torch(C, kidx, kvec, X_on, X_off, erow, ecol, shift, orank, ooff, eptr, eidx, aptr, aidx, wk, Gp, max_elems=1 << 24):
    """ops.bond_weights in torch ops: the rows of C gathered per atom into the nao-padded layout (0 where the atom lacks the orbital), then per chunk of
    group members one einsum c_i^+ X c_j, the phase (k . shift in double, rounded once), and index_add_ into the members' group columns"""
    ns = int(C.shape[0])
    N, nao = orank.shape
    G = int(eptr.shape[0]) - 1
    dev = C.device
    CA, have = padded_rows(C, orank, ooff)                                                            # [ns, N, nao]
    W = torch.zeros(ns, Gp, device=dev, dtype=torch.float32)
    step = max(1, max_elems // max(1, ns * nao))
    hv = have.to(torch.float32)

    def add(members, gid, rows, ri, cj, phase):
        for q0 in range(0, int(members.shape[0]), step):
            m = members[q0:q0 + step].long()
            i, j = ri[m].long(), cj[m].long()
            X = rows[m].reshape(-1, nao, nao) * hv[i][:, :, None] * hv[j][:, None, :]
            T = torch.einsum("eab,seb->sea", X.to(C.dtype), CA[:, j])
            p = (CA[:, i].conj() * T).sum(-1)                                                       # [ns, members]
            if phase:
                p = edge_phases(kvec[kidx.long()], shift[m], torch.float32) * p                   # [ns, members]
            W.index_add_(1, 1 + gid[q0:q0 + step], p.real.contiguous())

    gid = lambda ptr_: torch.repeat_interleave(torch.arange(G, device=dev), (ptr_[1:] - ptr_[:-1]).long())
    if G > 0:
        add(eidx, gid(eptr), X_off, erow, ecol, True)
        atoms = torch.arange(N, device=dev, dtype=torch.int32)
        add(aidx, gid(aptr), X_on, atoms, atoms, False)
    W *= wk[:, None]
    W[:, 0] = wk
    return W


def group_tensors(groups, device):
    """(eptr, eidx, aptr, aidx) of bond_groups(...) as int32 tensors on `device`; entries that are tensors already are taken as they are"""
    return tuple(g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g, dtype=np.int32)).to(device) for g in groups[:4])


def bond_weights(C, kidx, kvec, X_on, X_off, tables, groups, wk, Gp):
    """W [ns, Gp] fp32 of the states whose eigenvector rows are C [ns, M] complex64 (kidx int32 [ns] -> rows of kvec fp32 [nk, 3]): column 0 = wk, column
    1 + g = wk * the weight of bond group g, pad columns 0, from the rows X_on [N, nao^2], X_off [E, nao^2] fp32 (overlap: COOP, Hamiltonian: COHP).
    tables: bond_tables(...) on C's device; groups: bond_groups(...) (numpy, or int32 tensors on C's device; the labels are not read); Gp from
    dos.padded_groups(G).  HIP kernel hg_bond_weights, or torch ops (see dos._use_kernels)."""
    eptr, eidx, aptr, aidx = group_tensors(groups, C.device)
    t = tables
    if int(C.shape[1]) != t.M:
        raise ValueError(f"bond_weights: C has {int(C.shape[1])} orbital columns, the tables {t.M}")
    args = (C, kidx, kvec, X_on, X_off, t.erow, t.ecol, t.shift, t.orank, t.ooff, eptr, eidx, aptr, aidx, wk, int(Gp))
    if dos._use_kernels(C):
        return ops.bond_weights(*args)
    if int(Gp) < int(eptr.shape[0]):
        raise ValueError(f"bond_weights: Gp = {Gp} holds no room for the state weight and {int(eptr.shape[0]) - 1} groups")
    return _bond_weights_torch(*args)
