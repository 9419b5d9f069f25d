"""Band (group) velocities on a k-grid, v_n(k) = d eps_n / d k, by Hellmann-Feynman from the real-space rows the head emits -- no further solve, no
difference quotient, no M x M matrix.  A post-solver part like dos.py, bonds.py and density.py: it takes the solver's eigenvalues and eigenvectors and hands
dos.py's kernels their weight rows (Fermi velocities, the transport distribution sum v_a v_b delta(E - eps), velocity-adaptive smearing, band following).

    tables = bonds.bond_tables(head, z, edge_index, cell_shift, device)     # the tables of bonds.py, reused (integer cell shifts, reduced k-points)
    rvec = edge_vectors(cell, cell_shift).to(device)                        # [E, 3] fp32: the Cartesian lattice vector of every edge (lattice gauge)
    v = band_velocities(eps, C, kidx, kvec, Hoff, Soff, tables, rvec)       # [ns, 3] fp32, unit of the rows x unit of rvec (eV Angstrom, ...)
    v = band_velocities(..., degenerate_tol=1e-4)                           # degenerate runs: the eigenvalues of their velocity blocks
    W = transport_weights(v, wk)                                            # [ns, Gp]: wk | wk v_a v_b (xx, yy, zz, yz, xz, xy) | 0
    tdf = dos.broaden(eps, W, E0, dE, ne, sigma)                            # columns 1 .. 6: the transport distribution function; column 0: the DOS
    (or dos.tetra_dos / dos.tetra_states on W.reshape(nk, nb, Gp) with wk = ones)
    d = kgrad_elements(C, bra, ket, kidx, kvec, Hoff, tables, rvec)         # [np, 3] complex64: chosen elements <bra| dH/dk |ket> (interband, degenerate blocks)

The quantity.  With R_e the vector of edge e (rvec[e]), (i, j) = (erow[e], ecol[e]) its row and column atom, mu(i, a) = ooff[i] + orank[i][a] the compact
orbital index of hg_hk_assemble and the convention of kspace.assemble_k, X(k)[(i a), (j b)] += exp(2 pi i k . shift_e) X_off[e][a, b]:
    d_alpha X(k)[(i a), (j b)] = sum_e i R_e,alpha exp(2 pi i k . shift_e) X_off[e][a, b]                  (the on-site blocks do not depend on k)
    kgrad_elements: out[p, alpha] = sum_e i R_e,alpha exp(2 pi i k_p . shift_e) sum_{a, b} conj(C[bra_p, mu(i, a)]) X_off[e][a, b] C[ket_p, mu(j, b)]
    band_velocities: v[n, alpha] = Re c_n^+ (d_alpha H(k) - eps_n d_alpha S(k)) c_n                        (S-normalised rows, c^+ S c = 1)
for reduced k-points and integer cell shifts, R_e = cell_shift_e @ cell (the rows of cell are the lattice vectors) is the derivative with respect to the
CARTESIAN k, k_red = k_cart @ cell.T / (2 pi): v comes out in (unit of the rows) x (unit of cell).  The cost is ns E nao^2 per row set, against three M x M
assemblies and 3 M^3 per k-point for C^+ dH C, of which only the diagonal would be used.

Gauge.  rvec is the caller's: `edge_vectors` without positions gives the lattice gauge, in which kspace.assemble_k builds H(k) and the solver's C is
expressed; with positions it adds pos[j] - pos[i] (the atomic gauge, whose H(k) differs by the diagonal unitary exp(i k . pos)).  Band velocities are the
same in both, and so are the eigenvalues of a degenerate block (with the matching -eps d S term); single off-diagonal elements are NOT: in the atomic
gauge they hold the extra intra-cell term i (pos_j - pos_i) and are the ones to use for momentum (optical) matrix elements.

`kgrad_elements` runs the HIP kernel hg_kgrad_elements (csrc/spectra.hip: the per-edge MFMA contraction of hg_bond_weights, the edges split into chunks
across workgroups and added in a fixed order, no atomics, bit-reproducible, a pair's bits independent of the launch's other pairs) on CUDA tensors; CPU
tensors, and HG_DOS=torch on the GPU (the switch of dos._use_kernels), take a plain torch path (chunked gathers + einsum), the baseline of
tests/bench_velocity.py.

Out of scope: spin-orbit rows ((2 nao)^2: four spin blocks per edge), edge-sharded graphs (a rank's elements are partial sums over its own edges),
batches of several crystals (one call per crystal), second derivatives / effective masses, one fused pass over the H and the S rows (two calls), and any
driver that runs the eigen-solver.  Collinear spin is the spin-free call once per channel."""
from __future__ import annotations

import numpy as np
import torch

from . import dos, ops
from .bonds import _np
from .kspace import edge_phases, padded_rows

PAIRS = ("xx", "yy", "zz", "yz", "xz", "xy")                  # the column order of transport_weights
_PAIR_IDX = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


# ------------------------------------------------------------------------------------------------ edge vectors (host)
def edge_vectors(cell, cell_shift, pos=None, edge_index=None):
    """rvec [E, 3] fp32 (formed in double, rounded once; on cell_shift's device if that is a tensor): cell_shift @ cell, the Cartesian lattice vector of
    every edge -- the lattice gauge, in which kspace.assemble_k builds H(k).  cell [3, 3] (or [1, 3, 3]) with the lattice vectors as rows, cell_shift [E, 3]
    integer cell shifts.  With pos [N, 3] and edge_index [2, E] (row atom, column atom) it adds pos[j] - pos[i]: the atomic gauge, rvec = the bond vector.
    Band velocities and the eigenvalues of degenerate blocks do not depend on the gauge; single off-diagonal elements do (see the module docstring)."""
    c = _np(cell, np.float64).reshape(3, 3)
    sh = _np(cell_shift, np.float64)
    if sh.ndim != 2 or sh.shape[1] != 3:
        raise ValueError(f"edge_vectors: cell_shift must be [E, 3], got {sh.shape}")
    if sh.size and np.abs(sh - np.rint(sh)).max() > 0:
        raise ValueError("edge_vectors: cell_shift must hold integer cell shifts (the graph's cell_shift, not its Cartesian nbr_shift)")
    if (pos is None) != (edge_index is None):
        raise ValueError("edge_vectors: pos and edge_index go together")
    r = sh @ c
    if pos is not None:
        p, ei = _np(pos, np.float64), _np(edge_index, np.int64)
        if p.ndim != 2 or p.shape[1] != 3 or ei.shape != (2, sh.shape[0]) or (ei.size and (ei.min() < 0 or ei.max() >= p.shape[0])):
            raise ValueError(f"edge_vectors: pos must be [N, 3] and edge_index [2, {sh.shape[0]}] with entries in [0, N), got {p.shape}, {ei.shape}")
        r = r + p[ei[1]] - p[ei[0]]
    out = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32))
    return out.to(cell_shift.device) if isinstance(cell_shift, torch.Tensor) else out


# ------------------------------------------------------------------------------------------------ the elements: HIP kernel or torch
def _kgrad_elements_torch(C, bra, ket, kidx, kvec, X_off, erow, ecol, shift, rvec, orank, ooff, max_elems=1 << 24):
    """ops.kgrad_elements in torch ops, in the precision of C (complex64 or complex128): the rows of C gathered per atom into the nao-padded layout (0 where
    the atom lacks the orbital), then per chunk of edges one einsum X c_ket, the dot with conj(c_bra), the phase (k . shift in double, rounded once) and
    one matmul with i rvec"""
    N, nao = orank.shape
    E, npair = int(erow.shape[0]), int(ket.shape[0])
    rdt = C.real.dtype
    CA, have = padded_rows(C, orank, ooff)                                                            # [ns, N, nao]
    hv = have.to(rdt)
    b, k = bra.long()[:, None], ket.long()[:, None]
    kd = kvec.double()[kidx.long()[ket.long()]]                                                       # [np, 3]
    out = torch.zeros(npair, 3, device=C.device, dtype=C.dtype)
    step = max(1, max_elems // max(1, npair * nao))
    for q0 in range(0, E if npair else 0, step):
        i, j = erow[q0:q0 + step].long(), ecol[q0:q0 + step].long()
        X = X_off[q0:q0 + step].to(rdt).reshape(-1, nao, nao) * hv[i][:, :, None] * hv[j][:, None, :]
        T = torch.einsum("eab,peb->pea", X.to(C.dtype), CA[k, j[None, :]])
        p = (CA[b, i[None, :]].conj() * T).sum(-1)                                                    # [np, edges]
        z = edge_phases(kd, shift[q0:q0 + step], rdt) * p
        out += torch.complex(-z.imag, z.real) @ rvec[q0:q0 + step].to(C.dtype)                        # i z R
    return out


def kgrad_elements(C, bra, ket, kidx, kvec, X_off, tables, rvec):
    """out [np, 3] complex64: out[p, alpha] = <bra_p| d X(k) / d k_alpha |ket_p> = sum_e i rvec[e, alpha] exp(2 pi i k_p . shift_e) c_bra^+ X_off[e] c_ket for
    the pairs of rows bra, ket int32 [np] of C [ns, M] complex64 (kidx int32 [ns] -> rows of kvec fp32 [nk, 3]; both states of a pair at one k-point) from
    the rows X_off [E, nao^2] fp32 and the edge vectors rvec [E, 3] fp32 (edge_vectors: the gauge is the caller's).  Diagonal pairs (s, s) give the band
    velocities once H and S rows are combined (band_velocities), a few extra pairs the blocks of degenerate subspaces, chosen off-diagonal pairs interband
    elements.  tables: bonds.bond_tables(...) on C's device.  Every argument is checked on the host before anything runs (ValueError naming it).  A pair's
    result does not depend on the other pairs of the call.  HIP kernel hg_kgrad_elements, or torch ops (see dos._use_kernels)."""
    t = tables
    if isinstance(C, torch.Tensor) and C.dim() == 2 and int(C.shape[1]) != t.M:
        raise ValueError(f"kgrad_elements: C has {int(C.shape[1])} orbital columns, the tables {t.M}")
    args = (C, bra, ket, kidx, kvec, X_off, t.erow, t.ecol, t.shift, rvec, t.orank, t.ooff)
    if isinstance(C, torch.Tensor) and dos._use_kernels(C):
        return ops.kgrad_elements(*args)
    ops.kgrad_elements_check(*args)
    return _kgrad_elements_torch(*args)


# ------------------------------------------------------------------------------------------------ band velocities
def degenerate_runs(eps, kidx, tol):
    """[(first, last + 1)] of the runs of at least two consecutive states of one k-point whose neighbours lie within tol of each other; eps [ns] and kidx
    [ns] host arrays, the states of a k-point contiguous and ascending (ValueError otherwise)"""
    eps, kidx = np.asarray(eps, dtype=np.float64).reshape(-1), np.asarray(kidx, dtype=np.int64).reshape(-1)
    same = kidx[1:] == kidx[:-1]
    if len(np.unique(kidx)) != 1 + int((~same).sum()) or bool((np.diff(eps)[same] < 0).any()):
        raise ValueError("band_velocities: degenerate_tol needs the states of every k-point contiguous and ascending in eps (as band_energies_export returns them)")
    joined = same & (np.diff(eps) <= tol)
    runs, s = [], 0
    while s < len(joined):
        if joined[s]:
            e = s
            while e < len(joined) and joined[e]:
                e += 1
            runs.append((s, e + 1))
            s = e
        s += 1
    return runs


def band_velocities(eps, C, kidx, kvec, H_off, S_off, tables, rvec, degenerate_tol=None):
    """v [ns, 3] fp32 on C's device: v[n, alpha] = Re c_n^+ (d_alpha H(k) - eps_n d_alpha S(k)) c_n for the states whose S-normalised eigenvector rows are
    C [ns, M] complex64 and whose eigenvalues are eps (ns values: a tensor or array of any shape, [nk, nb] as the solver returns it included), from the
    Hamiltonian and overlap rows H_off, S_off [E, nao^2] fp32; S_off = None: an orthonormal basis, one call instead of two.  Two calls of kgrad_elements,
    combined as Re dH - eps Re dS in double and rounded once.  Units: those of the rows times those of rvec.
    degenerate_tol (in the unit of eps; needs the states of a k-point contiguous and ascending): inside a degenerate subspace the diagonal elements depend
    on the solver's arbitrary choice of vectors.  Runs of states of one k-point whose neighbours lie within degenerate_tol get their full Hermitian block
    <m| d_alpha H - eps_mean d_alpha S |n> (eps_mean the mean of the run) through extra pairs, and per component alpha the run's entries are the
    eigenvalues of that block, ascending -- the velocities of the bands that cross there, though not matched across components.  None: the plain diagonal."""
    if not isinstance(C, torch.Tensor) or C.dim() != 2:
        raise ValueError(f"band_velocities: C must be complex64 [ns, M], got {type(C).__name__} {tuple(getattr(C, 'shape', ()))}")
    ns, dev = int(C.shape[0]), C.device
    e_h = _np(eps, np.float64).reshape(-1)
    if e_h.shape[0] != ns:
        raise ValueError(f"band_velocities: eps must hold the {ns} eigenvalues of the rows of C, got {e_h.shape[0]}")
    runs = [] if degenerate_tol is None else degenerate_runs(e_h, _np(kidx, np.int64), float(degenerate_tol))
    diag = torch.arange(ns, dtype=torch.int32)
    extra = [(m, n) for a, b in runs for m in range(a, b) for n in range(m + 1, b)]                  # the upper triangles; the blocks are Hermitian
    up = torch.tensor(extra, dtype=torch.int32).reshape(-1, 2)
    bra, ket = torch.cat([diag, up[:, 0]]).to(dev), torch.cat([diag, up[:, 1]]).to(dev)
    dH = kgrad_elements(C, bra, ket, kidx, kvec, H_off, tables, rvec)
    dS = None if S_off is None else kgrad_elements(C, bra, ket, kidx, kvec, S_off, tables, rvec)
    e_d = torch.from_numpy(e_h).to(dev)
    v = dH[:ns].real.double()
    if dS is not None:
        v = v - e_d[:, None] * dS[:ns].real.double()
    if runs:
        dHh = dH.cpu().to(torch.complex128).numpy()
        dSh = None if dS is None else dS.cpu().to(torch.complex128).numpy()
        vh, q = v.cpu().numpy(), ns
        for a, b in runs:
            m, em = b - a, float(e_h[a:b].mean())
            iu = np.triu_indices(m, 1)
            nu = len(iu[0])
            el = lambda d: 0.0 if d is None else (np.concatenate([d[a:b], d[q:q + nu]]))
            vals = el(dHh) - em * el(dSh)                                                             # [m + nu, 3]: diagonal, then the upper triangle
            for al in range(3):
                B = np.zeros((m, m), dtype=np.complex128)
                B[iu] = vals[m:, al]
                B = B + B.conj().T + np.diag(vals[:m, al].real)
                vh[a:b, al] = np.linalg.eigvalsh(B)
            q += nu
        v = torch.from_numpy(vh).to(dev)
    return v.to(torch.float32)


# ------------------------------------------------------------------------------------------------ weight rows for dos.py
def transport_weights(v, wk, Gp=None):
    """W [ns, Gp] fp32 in the layout dos.broaden, dos.tetra_dos and dos.tetra_states take: column 0 = wk, columns 1 .. 6 = wk v_a v_b in the order PAIRS = xx,
    yy, zz, yz, xz, xy (formed in double, rounded once), pad columns 0; Gp defaults to dos.padded_groups(6).  v [ns, 3] (band_velocities), wk [ns] the
    k-weights per state (ones for the tetrahedron routines).  Broadened or integrated over the states, columns 1 .. 6 are the transport distribution
    function sum_s wk v_a v_b delta(E - eps_s) in (unit of v)^2 / (unit of eps)."""
    Gp = dos.padded_groups(6) if Gp is None else int(Gp)
    if v.dim() != 2 or int(v.shape[1]) != 3 or tuple(wk.shape) != (int(v.shape[0]),):
        raise ValueError(f"transport_weights: v must be [ns, 3] and wk [ns], got {tuple(v.shape)}, {tuple(wk.shape)}")
    if Gp < 7:
        raise ValueError(f"transport_weights: Gp = {Gp} holds no room for the state weight and the 6 components")
    W = torch.zeros(int(v.shape[0]), Gp, device=v.device, dtype=torch.float32)
    vd, wd = v.double(), wk.double()
    W[:, 0] = wk
    for c, (a, b) in enumerate(_PAIR_IDX):
        W[:, 1 + c] = (wd * vd[:, a] * vd[:, b]).float()
    return W
