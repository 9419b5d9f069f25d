"""The k-space step after the read-out: `HamGNNPlusPlusOut(calculate_band_energy=True)` of the reference
(hamgnn/models/hamgnn_output.py:1675-1996 calculate_band_energies; k-point generation :3802-3854; hamgnn/physics/kpoints.py:26-165).

Per crystal: k-points (random, or a path through given nodes in reduced coordinates) -> H(k), S(k) in the compact orbital basis by the
HIP kernel `hg_hk_assemble` (phase-factor sums over the edges of every atom pair, fixed order) -> generalized eigenproblem
H(k) psi = E S(k) psi through the Cholesky factor of S(k) exactly as the reference does it, on hipSOLVER via `torch.linalg`
(cholesky / inv / eigh on complex64: library calls, not kernels of this repository) -> band energies, wavefunctions, band gap,
optional band window.  The spin-free branch with the reference overlaps `Son / Soff` (also what the reference runs with ham_only=False: its
overlap-network variant :1368-1673 factorises the REFERENCE overlap too and is only reached with export_reciprocal_values) and the spinor
branch `band_energies_soc` (:1998-2286)."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from functools import cached_property
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import ops
from .topo import gget


# ------------------------------------------------------------------------------------------------ k-points (host geometry)
def k_path_points(kpts, nk: int, lat: np.ndarray):
    """The k-path of the reference (kpoints_generator(dim_k=3, lat).k_path(kpts, nk), hamgnn/physics/kpoints.py:26-165) as one piecewise
    linear interpolation: the path is a polyline through the reduced-coordinate nodes `kpts`, parametrised by its arc length in the
    reciprocal metric of `lat`; every node is pinned to the sample index nearest to its share of the total length, and between two pinned
    indices the samples are equally spaced.  That is `np.interp` of the three coordinates over the sample index with the pinned indices as
    abscissae.  Returns (k_vec [nk, 3] reduced, inv(lat).T)."""
    nodes = np.asarray(kpts, dtype=np.float64)
    if nodes.ndim != 2 or nodes.shape[1] != 3:
        raise ValueError("k_path: the nodes must be an [n, 3] list of reduced coordinates")
    if nk < nodes.shape[0]:
        raise ValueError("k_path: fewer sample points than nodes")
    cellm = np.asarray(lat, dtype=np.float64)
    metric = np.linalg.inv(cellm @ cellm.T)                                    # |dk|^2 = dk^T (A A^T)^-1 dk for reduced dk
    steps = np.diff(nodes, axis=0)
    arc = np.concatenate([[0.0], np.cumsum(np.sqrt(np.einsum("ni,ij,nj->n", steps, metric, steps)))])
    pins = np.rint(arc / arc[-1] * (nk - 1)).astype(np.int64)                  # sample index of every node (ends: 0 and nk - 1 exactly)
    pins[0], pins[-1] = 0, nk - 1
    if np.any(np.diff(pins) <= 0):
        raise ValueError("k_path: two nodes fall onto the same sample point (coincident nodes or too few points)")
    idx = np.arange(nk, dtype=np.float64)
    k_vec = np.stack([np.interp(idx, pins.astype(np.float64), nodes[:, d]) for d in range(3)], axis=1)
    return k_vec, np.linalg.inv(cellm).T


AU2ANG = 0.5291772083       # hamgnn/utils/constants.py:2


def auto_k_path_nodes(lat_bohr: np.ndarray, pos_bohr: np.ndarray, z) -> list:
    return auto_k_path(lat_bohr, pos_bohr, z)[1]


def auto_k_path(lat_bohr: np.ndarray, pos_bohr: np.ndarray, z):
    """-> (labels, nodes).  k_path='auto' of the reference (hamgnn_output.py:3812-3833): the high-symmetry path of the crystal from pymatgen's KPathSeek -- a Structure in
    Angstrom with the species' symbols, the labels of all path segments in a row with consecutive repeats dropped, their reduced coordinates as nodes.
    pymatgen is a third-party dependency of the reference (imported at :19-21) that this image does not have: without it the call raises."""
    try:
        from pymatgen.core.periodic_table import Element
        from pymatgen.core.structure import Structure
        from pymatgen.symmetry.kpath import KPathSeek
    except ImportError as e:
        raise NotImplementedError("k_path='auto' needs pymatgen (Structure / Element / KPathSeek), as in the reference (hamgnn_output.py:19-21, 3812-3837); "
                                  "give a list of reduced k-points or None (random) instead") from e
    structure = Structure(lattice=np.asarray(lat_bohr) * AU2ANG, species=[Element.from_Z(int(k)).symbol for k in z], coords=np.asarray(pos_bohr) * AU2ANG,
                          coords_are_cartesian=True)
    seek = KPathSeek(structure=structure)
    labels = [lab for group in seek.kpath["path"] for lab in group]
    unique = [labels[0]]
    for x in labels[1:]:
        if x != unique[-1]:
            unique.append(x)
    return unique, [seek.kpath["kpoints"][k] for k in unique]


def make_k_vectors(k_path, num_k: int, cell: torch.Tensor, rng=np.random, data=None) -> torch.Tensor:
    """data.k_vecs of the reference (:3802-3854): [n_crystals, num_k, 3] Cartesian-reciprocal k-vectors (no 2 pi: it sits in the phase).
    k_path: list of nodes in reduced coordinates; None -> uniformly random reduced k in [-1, 1)^3 (numpy's global RNG, as the reference); 'auto' -> the
    crystal's high-symmetry path (auto_k_path_nodes; needs `data` for positions / species and pymatgen; as in the reference a path that cannot be sampled
    falls back to random points)."""
    out = []
    cells = cell.detach().cpu().double().numpy().reshape(-1, 3, 3)
    auto = isinstance(k_path, str) and k_path.lower() == "auto"
    if auto:
        if data is None:
            raise ValueError("k_path='auto' needs the graph (positions and species of every crystal)")
        counts = gget(data, "node_counts")
        counts = [int(c) for c in counts.tolist()] if counts is not None else [int(data.z.shape[0])]
        pos_all, z_all = data.pos.detach().cpu().double().numpy(), data.z.detach().cpu().numpy()
        starts = np.concatenate([[0], np.cumsum(counts)])
    for ci, lat in enumerate(cells):
        if isinstance(k_path, (list, tuple)):
            k_vec, lat_per_inv = k_path_points(k_path, num_k, lat)
        elif auto:
            nodes = auto_k_path_nodes(lat, pos_all[starts[ci]:starts[ci + 1]], z_all[starts[ci]:starts[ci + 1]])
            try:
                k_vec, lat_per_inv = k_path_points(nodes, num_k, lat)
            except Exception:                                  # noqa: BLE001  (the reference's bare except, :3709-3713 / :3838-3841: random k-points)
                lat_per_inv = np.linalg.inv(lat).T
                k_vec = 2.0 * rng.rand(num_k, 3) - 1.0
        elif k_path is None:
            lat_per_inv = np.linalg.inv(lat).T
            k_vec = 2.0 * rng.rand(num_k, 3) - 1.0
        else:
            raise NotImplementedError(f"k_path={k_path!r}: a list of reduced k-points, 'auto' or None (random)")
        out.append(torch.from_numpy(k_vec.dot(lat_per_inv[np.newaxis, :, :]).reshape(-1, 3)).float())
    return torch.stack(out, 0)


# ------------------------------------------------------------------------------------------------ per-crystal index plumbing
def _crystal_slices(data):
    node_counts = gget(data, "node_counts")
    src = data.edge_index[0]
    if node_counts is None:
        return [(0, int(data.z.shape[0]), 0, int(src.shape[0]))]
    ncs = [int(v) for v in node_counts.tolist()]
    batch = gget(data, "batch")
    ecs = torch.bincount(batch[src], minlength=len(ncs)).tolist() if batch is not None else [int(src.shape[0])]
    out, n0, e0 = [], 0, 0
    for n, e in zip(ncs, ecs):
        out.append((n0, n, e0, int(e)))
        n0, e0 = n0 + n, e0 + int(e)
    return out


@dataclass(frozen=True, eq=False)
class CrystalTables:
    """The integer tables of one crystal that every consumer of the compact orbital basis reads (hg_hk_assemble and its adjoint, hg_bond_weights,
    hg_density_rows, the torch paths): built once per crystal and handed on.  n0, n, e0, e: the crystal's rows and edges inside the batch; orank int32
    [n, nao]: rank of an orbital inside its element's valid set or -1; ooff int32 [n]: first compact index of every atom; M: number of compact
    orbitals; erow / ecol int32 [e]: crystal-local row / column atom of every edge (edge_index[0] / [1]); shift fp32 [e, 3]: the shift the tables
    were GIVEN -- the Cartesian nbr_shift of the graph for the assembly (from_graph, with Cartesian k-vectors), integer cell shifts for the reduced-k
    convention of bonds.py (from_edges); only k . shift is ever formed.  The edges grouped by atom pair (pair_ptr, pair_edges, pair_ij) are only read
    by the assembly and its adjoint: computed at first use, then kept."""
    n0: int
    n: int
    e0: int
    e: int
    nao: int
    M: int
    orank: torch.Tensor
    ooff: torch.Tensor
    erow: torch.Tensor
    ecol: torch.Tensor
    shift: torch.Tensor

    @classmethod
    def from_graph(cls, data, n0, n, e0, e, orank_all):
        """rows n0:n0+n and edges e0:e0+e of a (batched) graph; orank_all [N, nao]: the head's rank table gathered by data.z; shift = data.nbr_shift
        rounded to fp32, what the kernels read -- so the torch adjoint of a graph with an fp64 nbr_shift now sees the forward's shifts, not the fp64 ones"""
        orank = orank_all[n0:n0 + n].to(torch.int32).contiguous()
        norb = (orank >= 0).sum(1)
        ooff = (torch.cumsum(norb, 0) - norb).to(torch.int32).contiguous()
        erow, ecol = ((data.edge_index[r][e0:e0 + e] - n0).to(torch.int32).contiguous() for r in (0, 1))
        return cls(n0, n, e0, e, int(orank.shape[1]), int(norb.sum()), orank, ooff, erow, ecol, data.nbr_shift[e0:e0 + e].float().contiguous())

    @classmethod
    def from_edges(cls, edge_index, shift, z, orank_by_z, device):
        """one whole crystal on `device` from host or device arrays: edge_index [2, E], shift [E, 3], z [N], orank_by_z [119, nao] (basis.orbital_rank_table)"""
        t = lambda a, dt: torch.as_tensor(a).to(device=device, dtype=dt)
        z = t(z, torch.int64).reshape(-1)
        graph = SimpleNamespace(edge_index=t(edge_index, torch.int64), nbr_shift=t(shift, torch.float32).reshape(-1, 3))
        return cls.from_graph(graph, 0, int(z.shape[0]), 0, int(graph.nbr_shift.shape[0]), t(orank_by_z, torch.int32)[z])

    @cached_property
    def _pairs(self):
        """edges grouped by atom pair, in the order of a stable sort of row * n + column"""
        key = self.erow.long() * self.n + self.ecol.long()
        order = torch.sort(key, stable=True).indices
        uniq, counts = torch.unique_consecutive(key[order], return_counts=True)
        ptr = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=key.device)
        ptr[1:] = torch.cumsum(counts, 0)
        return ptr, order.contiguous(), torch.stack([uniq // self.n, uniq % self.n], 1).contiguous()

    pair_ptr = property(lambda self: self._pairs[0], doc="int64 [npairs + 1]: the edges of pair p are pair_edges[pair_ptr[p]:pair_ptr[p + 1]]")
    pair_edges = property(lambda self: self._pairs[1], doc="int64 [e]: crystal-local edge ids, grouped by pair")
    pair_ij = property(lambda self: self._pairs[2], doc="int64 [npairs, 2]: (row atom, column atom) of every pair that has an edge")

    def __getitem__(self, name):
        """tab["erow"]: reading a field by its name, as from the dict bonds.bond_tables used to return (reading only: the object is no mapping)"""
        return getattr(self, name)

    @cached_property
    def compact_index(self):
        """int64 [n, nao]: compact orbital index of (atom, orbital) inside the crystal, or -1"""
        return torch.where(self.orank >= 0, self.ooff[:, None] + self.orank, torch.full_like(self.orank, -1)).long()


def padded_rows(C, orank, ooff):
    """(CA [ns, N, nao], have [N, nao]): the rows of C [ns, M] gathered per atom into the nao-padded layout, CA[s, i, a] = C[s, ooff[i] + orank[i][a]] and 0
    where the atom lacks the orbital (have = orank >= 0): the torch paths of bonds.py, density.py and velocity.py start here"""
    ns, M = C.shape
    have = orank >= 0
    comp = torch.where(have, ooff[:, None] + orank, torch.full_like(orank, M)).long()                # [N, nao]; M: the appended zero column
    return torch.cat([C, C.new_zeros(ns, 1)], 1)[:, comp], have


def edge_phases(k, shift, rdt):
    """complex [n, m] of real dtype rdt: exp(2 pi i k . shift) of the k rows [n, 3] and the shifts [m, 3]; the angle in double, rounded once (as hg_edge_phase)"""
    ang = 2.0 * np.pi * (k.double() @ shift.double().T)
    return torch.complex(torch.cos(ang).to(rdt), torch.sin(ang).to(rdt))


def assemble_k(on, off, tab, kvec):
    """[nk, M, M] complex64 of one crystal (the rows and edges of `tab`) from planar [.., nao^2] blocks of the batch"""
    return ops.hk_assemble(on[tab.n0:tab.n0 + tab.n].contiguous(), off[tab.e0:tab.e0 + tab.e].contiguous(), tab.shift, kvec.contiguous().float(),
                           tab.pair_ptr, tab.pair_edges, tab.pair_ij, tab.n, tab.nao, tab.orank, tab.ooff, tab.M)


def assemble_k_adjoint(G, tab, kvec):
    """Adjoint of assemble_k (hg_hk_assemble) for one crystal: G [nk, M, M] complex = the gradient of a real loss with respect to H(k) in
    torch's convention (d/dRe + i d/dIm) -> (g_on [n, nao^2], g_off [e, nao^2]) real.  With H(k)[(i a), (j b)] = on_i[a, b] delta_ij +
    sum_{e: i -> j} exp(2 pi i k . shift_e) off_e[a, b]:  g_off_e[a, b] = sum_k Re(conj(phase_k(e)) G_k[(i a), (j b)]).
    On the GPU: the HIP kernel hg_hk_assemble_adjoint on the pair tables of assemble_k (fixed order, no temporaries).  CPU tensors, and
    HG_HK_ADJOINT=torch on the GPU, take the torch path below."""
    if G.is_cuda and os.environ.get("HG_HK_ADJOINT", "").lower() != "torch":
        return ops.hk_assemble_adjoint(G.to(torch.complex64), tab.shift, kvec.contiguous().float(), tab.pair_ptr, tab.pair_edges, tab.pair_ij,
                                       tab.n, tab.e, tab.nao, tab.orank, tab.ooff, tab.M)
    return _assemble_k_adjoint_torch(G, tab, kvec)


def _assemble_k_adjoint_torch(G, tab, kvec):
    """assemble_k_adjoint as gathers and one complex multiply-reduce per chunk of k (torch tensor ops; device-agnostic, any precision,
    checked on CPU against autograd; [8, e, nao, nao] complex temporaries per chunk)"""
    comp, n, e, nao = tab.compact_index, tab.n, tab.e, tab.nao  # [n, nao]
    nk = G.shape[0]
    rdt = G.real.dtype
    ok_on = ((comp[:, :, None] >= 0) & (comp[:, None, :] >= 0)).to(rdt)
    Gon = G[:, comp.clamp(min=0)[:, :, None], comp.clamp(min=0)[:, None, :]]                # [nk, n, nao, nao]
    g_on = (Gon.real.sum(0) * ok_on).reshape(n, nao * nao)
    R, Cc = comp[tab.erow.long()], comp[tab.ecol.long()]
    ok = ((R[:, :, None] >= 0) & (Cc[:, None, :] >= 0)).to(rdt)
    cph = edge_phases(kvec, tab.shift, torch.float64).conj().to(G.dtype)                         # [nk, e] conj(phase), formed in double (see the kernel)
    g_off = torch.zeros(e, nao, nao, device=G.device, dtype=rdt)
    for k0 in range(0, nk, 8):
        Ge = G[k0:k0 + 8][:, R.clamp(min=0)[:, :, None], Cc.clamp(min=0)[:, None, :]]          # [<=8, e, nao, nao]
        g_off += (cph[k0:k0 + 8][:, :, None, None] * Ge).real.sum(0)
    return g_on, (g_off * ok).reshape(e, nao * nao)


def _eig_solve(Hk, Sk):
    """generalized eigenproblem through the Cholesky factor of S(k), as the reference (:1911-1928) -> (evals [k, M], evecs [k, band, M], Ht)"""
    L = torch.linalg.cholesky(Sk)
    Linv = torch.linalg.inv(L)
    LHinv = torch.linalg.inv(L.conj().transpose(-1, -2))
    Ht = torch.bmm(torch.bmm(Linv, Hk), LHinv)
    evals, evecs = torch.linalg.eigh(Ht)
    evecs = torch.einsum("ijk,ika->iaj", LHinv, evecs)
    return evals, evecs, Ht


def _window_bounds(head, val_c, z_c):
    """(half, lo, hi): the band below which half the valence electrons sit, and the band window [lo:hi] of band_num_control (None, None: all bands)"""
    half = math.ceil(float(val_c.sum()) / 2)
    bnc = head.band_num_control
    if bnc is None:
        return half, None, None
    if isinstance(bnc, dict):
        return half, 0, int(sum(int(bnc.get(int(zz), bnc.get(str(int(zz)), 0))) for zz in z_c.tolist()))
    win = max(1, int(bnc * half)) if isinstance(bnc, float) else min(int(bnc), half)
    return half, half - win, half + win


def _gap_and_window(head, evals, evecs, val_c, z_c):
    """the band gap (min / max over ALL k of the two bands around half filling, before the window is cut) and the band window -> (evals, evecs, gap)"""
    half, lo, hi = _window_bounds(head, val_c, z_c)
    gap = (evals[:, half].min() - evals[:, half - 1].max()).reshape(1)
    if lo is not None:
        evals, evecs = evals[:, lo:hi], evecs[:, lo:hi, :]
    return evals, evecs, gap


def _eig_chain(head, Hk, Sk, val_c, z_c):
    """_eig_solve on all k-points of a crystal + gap + band window -> (evals, evecs, Ht, gap)"""
    evals, evecs, Ht = _eig_solve(Hk, Sk)
    evals, evecs, gap = _gap_and_window(head, evals, evecs, val_c, z_c)
    return evals, evecs, Ht, gap


# ------------------------------------------------------------------------------------------------ edge-sharded crystal (parallel.shard_graph)
# Every rank holds all atoms and its own edges.  H(k) and S(k) are sums over edges: each rank assembles its partial matrices for ALL k (the replicated
# on-site rows enter on rank 0 only), one all-reduce makes them whole, and the k-points are dealt to the ranks in contiguous blocks for the Cholesky /
# eigh chain -- the dominant cost of the step.  Eigenvalues (and, in the forward, eigenvectors) are all-gathered, so everything derived from all k (band
# window, gap) is computed identically on every rank.  The backward gathers the per-block gradient G of H(k) and runs the assembly's adjoint over the
# rank's own edges with all k: the on-site gradient comes out identical on every rank, the off-site gradient is the rank's own.
def _shard_of(data):
    """(rank, world) of an edge-sharded graph, else None"""
    from . import parallel
    if not parallel.is_sharded(data):
        return None
    import torch.distributed as dist
    if not dist.is_initialized():
        raise RuntimeError("graph is sharded but torch.distributed is not initialised")
    return tuple(int(v) for v in data.get("_hg_shard"))


def _own_onsite(on, shard):
    """the replicated on-site rows enter the summed assembly once: on rank 0"""
    return on if shard is None or shard[0] == 0 else torch.zeros_like(on)


def _k_block(shard, nk):
    """[k0, k1): the contiguous block of k-points this rank solves (empty when nk < world for some ranks)"""
    rank, world = shard
    return rank * nk // world, (rank + 1) * nk // world


def _sum_over_ranks(mat):
    """sum of the ranks' partial [nk, M, M] complex matrices (as real pairs: gloo takes no complex tensors)"""
    import torch.distributed as dist
    buf = torch.view_as_real(mat.contiguous()).contiguous()
    dist.all_reduce(buf, op=dist.ReduceOp.SUM)
    return torch.view_as_complex(buf)


def _gather_k(block, shard, nk):
    """the ranks' k-blocks [k1 - k0, ...] (real or complex) -> [nk, ...] in k order on every rank; blocks are padded to the largest one"""
    import torch.distributed as dist
    world = shard[1]
    sizes = [(r + 1) * nk // world - r * nk // world for r in range(world)]
    cplx = block.is_complex()
    b = torch.view_as_real(block.contiguous()) if cplx else block
    buf = b.new_zeros((max(sizes),) + tuple(b.shape[1:]))
    buf[:b.shape[0]] = b
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf)
    out = torch.cat([p[:sz] for p, sz in zip(parts, sizes)], 0).contiguous()
    return torch.view_as_complex(out) if cplx else out


def broadcast_k_vectors(k_vecs, data):
    """random (or path) k-vectors of a sharded graph: rank 0's, on every rank"""
    if _shard_of(data) is None:
        return k_vecs
    import torch.distributed as dist
    k_vecs = k_vecs.contiguous()
    dist.broadcast(k_vecs, src=0)
    return k_vecs


def _solve_k_block(shard, nk, solve, empty):
    """the tensors `solve(k0, k1)` returns for this rank's block of k-points ([k1 - k0, ...] each; the tuple `empty` of [0, ...] zeros where the rank
    has no k-point), gathered to [nk, ...] in k order on every rank.  Every rank joins the gathers."""
    k0, k1 = _k_block(shard, nk)
    return tuple(_gather_k(t, shard, nk) for t in (solve(k0, k1) if k1 > k0 else empty))


def _eig_chain_sharded(head, Hk, Sk, val_c, z_c, shard):
    """_eig_chain on the summed H(k), S(k) of a sharded crystal: this rank solves its k-block, the blocks are gathered"""
    nk, M = int(Hk.shape[0]), int(Hk.shape[1])
    evals, evecs, Ht = _solve_k_block(shard, nk, lambda k0, k1: _eig_solve(Hk[k0:k1], Sk[k0:k1]),
                                      (Hk.real.new_zeros(0, M), Hk.new_zeros(0, M, M), Hk.new_zeros(0, M, M)))
    evals, evecs, gap = _gap_and_window(head, evals, evecs, val_c, z_c)
    return evals, evecs, Ht, gap


def _crystals(name, head, rows, data, k_vecs):
    """The opening every public function of the k-space step shares -> (shard, Son, Soff, crystals): `shard` = (rank, world) of an edge-sharded graph or
    None, the reference overlap rows in fp32 (the rank's own: _own_onsite), and an iterator over the crystals of the batch (the one crystal of a sharded
    graph) that yields (tab, kvec, val_c, z_c): the crystal's CrystalTables -- built here, once -- its k-vectors [nk, 3], and the valence electrons and
    species of its atoms.  `rows`: any of the caller's row tensors (its device is where the tables go); `name`: the caller, for the error."""
    dev = rows.device
    k_vecs = gget(data, "k_vecs") if k_vecs is None else k_vecs
    if k_vecs is None:
        raise ValueError(f"{name}: no k-vectors (data.k_vecs)")
    k_vecs = k_vecs.to(dev)
    z = data.z
    orank_all = head._orank.to(dev)[z]                         # [N, nao] rank of an orbital in its element's valid set or -1
    val = head._num_valence.to(dev)[z].to(torch.float64)
    shard = _shard_of(data)
    slices = _crystal_slices(data)
    if shard is not None and len(slices) != 1:
        raise ValueError("the k-space step on an edge-sharded graph: a sharded graph holds exactly one crystal")
    crystals = ((CrystalTables.from_graph(data, n0, n, e0, e, orank_all), k_vecs[c], val[n0:n0 + n], z[n0:n0 + n]) for c, (n0, n, e0, e) in enumerate(slices))
    return shard, _own_onsite(data.Son.contiguous().float(), shard), data.Soff.contiguous().float(), crystals


def band_energies(head, onsite_hamiltonian, offsite_hamiltonian, data, k_vecs: Optional[torch.Tensor] = None):
    """calculate_band_energies(onsite, offsite, data) of the reference (:1675-1996, export_reciprocal_values=False): returns
    (band_energy [sum_c bands_c, num_k], wavefunction (flattened), band_gap [n_crystals], H_sym (flattened))."""
    shard, Son, Soff, crystals = _crystals("band_energies", head, onsite_hamiltonian, data, k_vecs)
    energies, waves, gaps, hsyms = [], [], [], []
    for tab, kvec, val_c, z_c in crystals:
        Hk = assemble_k(_own_onsite(onsite_hamiltonian, shard), offsite_hamiltonian, tab, kvec)
        Sk = assemble_k(Son, Soff, tab, kvec)
        if shard is None:
            evals, evecs, Ht, gap = _eig_chain(head, Hk, Sk, val_c, z_c)
        else:
            evals, evecs, Ht, gap = _eig_chain_sharded(head, _sum_over_ranks(Hk), _sum_over_ranks(Sk), val_c, z_c, shard)
        gaps.append(gap)
        energies.append(evals.transpose(-1, -2))
        waves.append(evecs.reshape(-1))
        hsyms.append(Ht.reshape(-1))
    return torch.cat(energies, 0), torch.cat(waves, 0), torch.cat(gaps, 0), torch.cat(hsyms, 0)


def band_energies_export(head, onsite_hamiltonian, offsite_hamiltonian, data, overlap=None, k_vecs: Optional[torch.Tensor] = None):
    """The `export_reciprocal_values=True` form of the k-space step: calculate_band_energies(..., True) (hamgnn_output.py:1675-1996; `overlap`
    None) and calculate_band_energies_with_overlap(..., True) (:1368-1673; `overlap` = the PREDICTED (onsite, offsite) overlap rows of the
    overlap networks).  Returns (band_energy [sum_c bands_c, num_k], wavefunction [C, num_k, bands, M] normalised to <psi|S(k)|psi> = 1,
    HK [C, num_k, M, M], SK [C, num_k, M, M] (the reference overlap, or the predicted one), dSK [C, num_k, M, M, 3] from data.dSon / dSoff,
    band_gap [C]).  As in the reference the eigenproblem is always solved with the REFERENCE overlap (:1603), and the per-crystal results are
    stacked, i.e. every crystal of the batch must have the same number of orbitals."""
    if _shard_of(data) is not None:
        raise NotImplementedError("export_reciprocal_values on an edge-sharded graph is not built: H(k), S(k) and dS(k) would be those of the rank's "
                                  "own edges only; run the export on the whole crystal")
    nao = head.nao_max
    _, Son, Soff, crystals = _crystals("band_energies_export", head, onsite_hamiltonian, data, k_vecs)
    dSon, dSoff = data.dSon.float().reshape(Son.shape[0], nao * nao, 3), data.dSoff.float().reshape(Soff.shape[0], nao * nao, 3)
    energies, waves, gaps, HKs, SKs, dSKs = [], [], [], [], [], []
    for tab, kvec, val_c, z_c in crystals:
        Hk = assemble_k(onsite_hamiltonian, offsite_hamiltonian, tab, kvec)
        Sk = assemble_k(Son, Soff, tab, kvec)
        Sp = Sk if overlap is None else assemble_k(overlap[0].contiguous().float(), overlap[1].contiguous().float(), tab, kvec)
        dSk = torch.stack([assemble_k(dSon[..., d].contiguous(), dSoff[..., d].contiguous(), tab, kvec) for d in range(3)], -1)
        evals, evecs, _, gap = _eig_chain(head, Hk, Sk, val_c, z_c)
        norm = torch.einsum("nai,nij,naj->na", evecs.conj(), Sk, evecs).real
        evecs = evecs * (1.0 / torch.sqrt(norm)).unsqueeze(-1)
        energies.append(evals.transpose(-1, -2))
        waves.append(evecs)
        gaps.append(gap)
        HKs.append(Hk)
        SKs.append(Sp)
        dSKs.append(dSk)
    if len({tuple(w.shape) for w in waves}) != 1:
        raise ValueError("export_reciprocal_values stacks the crystals' H(k) / S(k) / wavefunctions (hamgnn_output.py:1984-1990): every crystal of the "
                         "batch must have the same number of orbitals and bands")
    return torch.cat(energies, 0), torch.stack(waves, 0), torch.stack(HKs, 0), torch.stack(SKs, 0), torch.stack(dSKs, 0), torch.cat(gaps, 0)


def _soc_overlap(Sk, Hk, M):
    """kron(1_2, S(k)) (:2165-2167) in the shape of the spinor H(k)"""
    Ssoc = torch.zeros_like(Hk)
    Ssoc[:, :M, :M] = Sk
    Ssoc[:, M:, M:] = Sk
    return Ssoc


def _soc_solve(Hk, Ssoc, vectors=True):
    """the spinor eigenproblem through the Cholesky factor of kron(1_2, S(k)) (:2236-2252) -> (evals [k, 2 M], evecs [k, 2 M, band] or None)"""
    L = torch.linalg.cholesky(Ssoc)
    Linv = torch.linalg.inv(L)
    LHinv = torch.linalg.inv(L.conj().transpose(-1, -2))
    if not vectors:
        return torch.linalg.eigvalsh(torch.bmm(torch.bmm(Linv, Hk), LHinv)), None
    evals, evecs = torch.linalg.eigh(torch.bmm(torch.bmm(Linv, Hk), LHinv))
    return evals, torch.bmm(LHinv, evecs)


def _soc_window_bounds(head, val_c, z_c):
    """the band window [lo:hi] of band_num_control on a spin-orbit head (:2254-2263), or (None, None): all bands"""
    bnc = head.band_num_control
    if bnc is None:
        return None, None
    if isinstance(bnc, dict):
        return 0, int(sum(int(bnc.get(int(zz), bnc.get(str(int(zz)), 0))) for zz in z_c.tolist()))
    nval = int(val_c.sum())
    return nval - int(bnc), nval + int(bnc)


def band_energies_soc(head, real_onsite, imag_onsite, real_offsite, imag_offsite, data, k_vecs: Optional[torch.Tensor] = None):
    """calculate_band_energies_with_spin_orbit_coupling of the reference (hamgnn_output.py:1998-2286): spinor Hamiltonian rows
    [., (2 nao)^2] (real and imaginary part, on-site and off-site) -> (band_energy [sum_c bands_c, num_k], wavefunction (flattened)).
    Per crystal the four spin blocks (uu, ud, du, dd) of H(k) are phase-factor sums like the spin-free case -- each block = assembly of its
    real part + i x assembly of its imaginary part (the assembly is linear), eight launches of hg_hk_assemble -- stacked to [2 M, 2 M];
    S(k) is the spin-free overlap on both spin diagonals (kron(1_2, S(k)), :2165-2167); generalised eigenproblem through the Cholesky
    factor of S(k) (:2236-2252, hipSOLVER through torch.linalg); band window :2254-2263 (dict: leading bands; int: +- that many bands
    around the number of valence electrons).  Edge-sharded crystal: the stacked H(k) and S(k) are summed over the ranks once each, every rank
    solves its block of k-points, eigenvalues and eigenvectors are gathered (see _eig_chain_sharded)."""
    shard, Son, Soff, crystals = _crystals("band_energies_soc", head, real_onsite, data, k_vecs)
    energies, waves = [], []
    for tab, kvec, val_c, z_c in crystals:
        M = tab.M
        Sk = assemble_k(Son, Soff, tab, kvec)
        Hk = _soc_hk(_own_onsite(real_onsite, shard), _own_onsite(imag_onsite, shard), real_offsite, imag_offsite, tab, kvec)      # [nk, 2 M, 2 M]
        if shard is None:
            evals, evecs = _soc_solve(Hk, _soc_overlap(Sk, Hk, M))
        else:
            Hk, Sk = _sum_over_ranks(Hk), _sum_over_ranks(Sk)
            evals, evecs = _solve_k_block(shard, int(Hk.shape[0]), lambda k0, k1: _soc_solve(Hk[k0:k1], _soc_overlap(Sk[k0:k1], Hk[k0:k1], M)),
                                          (Hk.real.new_zeros(0, 2 * M), Hk.new_zeros(0, 2 * M, 2 * M)))
        lo, hi = _soc_window_bounds(head, val_c, z_c)
        if lo is not None:
            evals, evecs = evals[:, lo:hi], evecs[:, lo:hi, :]
        energies.append(evals.transpose(-1, -2))
        waves.append(evecs.reshape(-1))
    return torch.cat(energies, 0), torch.cat(waves, 0)


def _sharded_chain_gradient(solve, Hk, shard, cot_window, lo, hi, gap=None):
    """G [nk, M, M] = gradient of sum(window(evals) * cot_window) (+ gap term) with respect to the summed H(k) of a sharded crystal: the cotangent is
    laid out on the eigenvalues of ALL bands and k [nk, bands]; this rank differentiates `solve` (H(k) block -> evals) on its k-block with its slice
    of the cotangent, and the blocks of G are gathered.  gap: (half, cotangent scalar) -- the gap is min_k evals[:, half] - max_k evals[:, half - 1], so
    its cotangent is one-hot at the arg-min / arg-max of the GATHERED eigenvalues and joins the band cotangent: one chain per k-point."""
    nk, nb_all = int(Hk.shape[0]), int(Hk.shape[1])
    C = torch.zeros(nk, nb_all, device=Hk.device, dtype=Hk.real.dtype)
    if cot_window is not None:
        C[:, lo:hi] = cot_window.to(C.dtype).transpose(0, 1)
    k0, k1 = _k_block(shard, nk)
    with torch.enable_grad():
        Hb = Hk[k0:k1].detach().requires_grad_()
        evals = solve(Hb, k0, k1) if k1 > k0 else None         # solved once; both gathers below read it (no k-point: they take their zeros)
        if gap is not None:
            half, gc = gap
            (full,) = _solve_k_block(shard, nk, lambda *_: (evals.detach(),), (C.new_zeros(0, nb_all),))
            C[torch.argmin(full[:, half]), half] += gc.to(C.dtype)
            C[torch.argmax(full[:, half - 1]), half - 1] -= gc.to(C.dtype)
        return _solve_k_block(shard, nk, lambda *_: torch.autograd.grad((evals * C[k0:k1]).sum(), Hb), (Hk.new_zeros(0, nb_all, nb_all),))[0]


def band_energy_backward(head, onsite_hamiltonian, offsite_hamiltonian, data, cotangent, k_vecs: Optional[torch.Tensor] = None, gap_cotangent=None):
    """gradient of sum(band_energy * cotangent) + sum(band_gap * gap_cotangent) with respect to the real-space blocks (the band_energy /
    band_gap losses of the reference's second training stage, Model.py:150-196): H(k) from the assembly kernel, the Cholesky / eigh chain
    differentiated by torch.autograd (library solvers, as in the forward) ONCE per crystal for both terms, then the assembly's adjoint
    (hg_hk_assemble_adjoint).  cotangent [sum_c bands_c, num_k] or None, gap_cotangent [n_crystals] or None.  The gap is a min / max over k
    of the two bands around half filling, taken before the band window is cut (_eig_chain).  Returns (g_on, g_off).
    Edge-sharded crystal: H(k), S(k) summed over the ranks, the chain differentiated on this rank's k-block, G gathered, the adjoint over the
    rank's own edges with all k -- g_on is the whole crystal's on every rank, g_off belongs to the rank's edges (_sharded_chain_gradient)."""
    if cotangent is None and gap_cotangent is None:
        raise ValueError("band_energy_backward: neither a band-energy nor a band-gap cotangent")
    shard, Son, Soff, crystals = _crystals("band_energy_backward", head, onsite_hamiltonian, data, k_vecs)
    g_on = torch.zeros_like(onsite_hamiltonian)
    g_off = torch.zeros_like(offsite_hamiltonian)
    row = 0
    for c, (tab, kvec, val_c, z_c) in enumerate(crystals):
        Hk = assemble_k(_own_onsite(onsite_hamiltonian, shard), offsite_hamiltonian, tab, kvec)
        Sk = assemble_k(Son, Soff, tab, kvec)
        if shard is None:
            with torch.enable_grad():
                Hk = Hk.detach().requires_grad_()
                evals, _, _, gap = _eig_chain(head, Hk, Sk, val_c, z_c)
                evals = evals.transpose(-1, -2)                    # [bands, nk]
                nb = evals.shape[0]
                scalar = 0.0
                if cotangent is not None:
                    scalar = scalar + (evals * cotangent[row:row + nb].to(evals.dtype)).sum()
                if gap_cotangent is not None:
                    scalar = scalar + (gap * gap_cotangent[c].to(gap.dtype)).sum()
                (G,) = torch.autograd.grad(scalar, Hk)
        else:
            Hk, Sk = _sum_over_ranks(Hk), _sum_over_ranks(Sk)
            half, lo, hi = _window_bounds(head, val_c, z_c)
            nb = len(range(tab.M)[slice(lo, hi)])
            G = _sharded_chain_gradient(lambda Hb, k0, k1: _eig_solve(Hb, Sk[k0:k1])[0], Hk, shard,
                                        None if cotangent is None else cotangent[row:row + nb], lo, hi,
                                        gap=None if gap_cotangent is None else (half, gap_cotangent[c]))
        row += nb
        g_on[tab.n0:tab.n0 + tab.n], g_off[tab.e0:tab.e0 + tab.e] = assemble_k_adjoint(G, tab, kvec)
    return g_on, g_off


def _soc_hk(real_onsite, imag_onsite, real_offsite, imag_offsite, tab, kvec):
    """spinor H(k) [nk, 2 M, 2 M] of one crystal: four spin blocks, each the assembly of its real part + i x the assembly of its imaginary part"""
    nao = tab.nao
    blk = lambda t, a, b: t.reshape(-1, 2, nao, 2, nao)[:, a, :, b, :].reshape(-1, nao * nao).contiguous().float()
    rows = []
    for a in (0, 1):
        cols = []
        for b in (0, 1):
            Hr = assemble_k(blk(real_onsite, a, b), blk(real_offsite, a, b), tab, kvec)
            Hi = assemble_k(blk(imag_onsite, a, b), blk(imag_offsite, a, b), tab, kvec)
            cols.append(Hr + 1j * Hi)
        rows.append(torch.cat(cols, -1))
    return torch.cat(rows, -2)


def band_energy_backward_soc(head, real_onsite, imag_onsite, real_offsite, imag_offsite, data, cotangent, k_vecs: Optional[torch.Tensor] = None):
    """gradient of sum(band_energy * cotangent) of band_energies_soc with respect to the four spinor row sets (a band-energy loss on a
    spin-orbit head; Model.py:150-196 with prediction: band_energy, bands from hamgnn_output.py:1998-2286).  As band_energy_backward: the
    Cholesky / eigh chain on the stacked [2 M, 2 M] H(k) is differentiated by torch.autograd (library solvers), then every spin block of
    the gradient G goes through the assembly's adjoint -- G_ab for the real rows, -i G_ab for the imaginary rows (H_ab = A(real) + i A(imag)
    with the real-linear assembly A).  Returns (g_real_on, g_imag_on, g_real_off, g_imag_off) in the rows' [., 2, nao, 2, nao] layout.
    Edge-sharded crystal: as band_energy_backward (the on-site gradients are the whole crystal's on every rank)."""
    nao = head.nao_max
    shard, Son, Soff, crystals = _crystals("band_energy_backward_soc", head, real_onsite, data, k_vecs)
    g = [torch.zeros(t.shape[0], 2, nao, 2, nao, device=real_onsite.device, dtype=torch.float32) for t in (real_onsite, imag_onsite, real_offsite, imag_offsite)]
    row = 0
    for tab, kvec, val_c, z_c in crystals:
        M, (n0, n, e0, e) = tab.M, (tab.n0, tab.n, tab.e0, tab.e)
        Sk = assemble_k(Son, Soff, tab, kvec)
        Hk = _soc_hk(_own_onsite(real_onsite, shard), _own_onsite(imag_onsite, shard), real_offsite, imag_offsite, tab, kvec)
        lo, hi = _soc_window_bounds(head, val_c, z_c)
        if shard is None:
            Ssoc = _soc_overlap(Sk, Hk, M)
            with torch.enable_grad():
                Hk = Hk.detach().requires_grad_()
                evals, _ = _soc_solve(Hk, Ssoc, vectors=False)
                if lo is not None:
                    evals = evals[:, lo:hi]
                evals = evals.transpose(-1, -2)                    # [bands, nk]
                nb = evals.shape[0]
                (G,) = torch.autograd.grad((evals * cotangent[row:row + nb].to(evals.dtype)).sum(), Hk)
        else:
            Hk, Sk = _sum_over_ranks(Hk), _sum_over_ranks(Sk)
            nb = len(range(2 * M)[slice(lo, hi)])
            G = _sharded_chain_gradient(lambda Hb, k0, k1: _soc_solve(Hb, _soc_overlap(Sk[k0:k1], Hb, M), vectors=False)[0], Hk, shard,
                                        cotangent[row:row + nb], lo, hi)
        row += nb
        for a in (0, 1):
            for b in (0, 1):
                Gab = G[:, a * M:(a + 1) * M, b * M:(b + 1) * M]
                r_on, r_off = assemble_k_adjoint(Gab, tab, kvec)
                i_on, i_off = assemble_k_adjoint(-1j * Gab, tab, kvec)
                g[0][n0:n0 + n, a, :, b, :] = r_on.reshape(n, nao, nao)
                g[1][n0:n0 + n, a, :, b, :] = i_on.reshape(n, nao, nao)
                g[2][e0:e0 + e, a, :, b, :] = r_off.reshape(e, nao, nao)
                g[3][e0:e0 + e, a, :, b, :] = i_off.reshape(e, nao, nao)
    return tuple(t.reshape(t.shape[0], -1) for t in g)
