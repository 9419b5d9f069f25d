"""HamGNN_pre.build_internal_graph: the wider periodic graph both backbones pass messages on (BaseModel.generate_graph,
hamgnn/models/base_model.py:237-288; used in hamgnn/models/hamgnn_conv.py:252-283).  Two atoms are neighbours when their distance is below
radius_scale * (r_i + r_j) (the radii table of basis.atomic_radii, 10.0 for an element the table lacks: base_model.py:63, 84); the layers run
on that graph and the representation goes back on the edges the data came with, through `matching_edges`.

The reference rebuilds the graph on the host (ASE) in every forward.  Here it is built on the device -- csrc/neighbour.hip: hg_neighbour_bin
(cell list in fractional coordinates), hg_neighbour_pairs (count pass, prefix sum, fill pass: one packed int64 key per edge), a sort of the keys
(their ascending order IS the canonical edge order (i, j, S0, S1, S2), so nothing depends on scheduling), hg_neighbour_decode -- and kept on the
data object until `pos`, `cell`, `z`, `batch`, `edge_index` or `cell_shift` are replaced or changed in place (the mechanism of topo.py).  A build
reads two small tensors back: the edge count (with the error flags of the kernels) and "every data edge matched".

Batches: atom indices of crystal b are offset by the atoms of ALL crystals before it.  (The reference adds `node_counts[idx - 1]`, the size of the
previous crystal alone, instead of the running sum -- right for batches of up to two crystals only.)"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .basis import atomic_radii
from .data.graph import Graph
from .topo import _sig, gget

CACHE_ATTR = "_hg_internal_graph"
DEFAULT_RADIUS = 10.0                                          # base_model.py:63
SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe "
           "Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr "
           "Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og").split()
KEY_ATOM_BITS, KEY_SHIFT_OFF, KEY_SHIFT_MAX = 24, 16, 15       # the packed edge key of csrc/neighbour.hip: i << 39 | j << 15 | three 5-bit shifts
_FLAG_TEXT = {1: "a singular or non-finite cell (or no positive radius)", 2: "more than 15 periodic images along a lattice direction: the radii are far larger than the cell",
              4: "a neighbour table was too small (inputs changed while the graph was built?)", 8: "a non-finite position or a batch index outside the cells given"}
_TABLES = {}


def check_radius_config(radius_scale):
    """hamgnn_conv.py:90-95: a missing radius_scale means 1.0, a given one must be greater than 1.0"""
    if radius_scale is None:
        return 1.0
    if not float(radius_scale) > 1.0:
        raise ValueError("HamGNN_pre.radius_scale: the radius scaling factor must be greater than 1.0 (build_internal_graph)")
    return float(radius_scale)


def radius_table(radius_type="openmx", radius_scale=1.0, device="cpu") -> torch.Tensor:
    """fp64 [number of elements]: radius_scale * radius of the element (base_model.py:65-84), DEFAULT_RADIUS where the table has no entry"""
    key = (str(radius_type), float(radius_scale), str(device))
    if key not in _TABLES:
        tab = atomic_radii(radius_type)
        host = np.array([tab.get(s, DEFAULT_RADIUS) for s in SYMBOLS], dtype=np.float64) * float(radius_scale)
        _TABLES[key] = torch.from_numpy(host).to(device)
    return _TABLES[key]


def _raise_flags(fl):
    if fl:
        raise ValueError("build_internal_graph: " + "; ".join(t for b, t in _FLAG_TEXT.items() if fl & b))


def pack_keys(edge_index, cell_shift) -> torch.Tensor:
    """the packed keys of (i, j, S) rows; -1 where a shift lies outside the key's range (such an edge is in no internal list)"""
    s = cell_shift.long() + KEY_SHIFT_OFF
    ok = ((s >= KEY_SHIFT_OFF - KEY_SHIFT_MAX) & (s <= KEY_SHIFT_OFF + KEY_SHIFT_MAX)).all(1)
    key = (edge_index[0].long() << 39) | (edge_index[1].long() << 15) | (s[:, 0] << 10) | (s[:, 1] << 5) | s[:, 2]
    return torch.where(ok, key, torch.full_like(key, -1))


def neighbour_list(pos, cell, batch, node_counts, radius):
    """All directed periodic pairs (i, j, S) with |pos_j + S cell - pos_i| < radius_i + radius_j, sorted by (i, j, S0, S1, S2).
    -> (keys [E] sorted packed keys, edge_index [2, E] int64, cell_shift [E, 3] int64, nbr_shift [E, 3] fp32, flags: the kernels' error word, still on the device)"""
    N, dev = int(pos.shape[0]), pos.device
    cell = cell.reshape(-1, 3, 3).contiguous()
    B = int(cell.shape[0])
    if N >= (1 << KEY_ATOM_BITS):
        raise NotImplementedError(f"build_internal_graph: at most 2^{KEY_ATOM_BITS} atoms per batch")
    if batch is None and B != 1:
        raise ValueError("build_internal_graph: a batch of several cells needs data.batch")
    atom_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    if node_counts is not None:
        atom_ptr[1:] = torch.cumsum(node_counts.to(dev).long(), 0)          # CUMULATIVE offsets (module docstring)
    elif batch is not None:
        atom_ptr[1:] = torch.cumsum(torch.bincount(batch, minlength=B)[:B], 0)
    else:
        atom_ptr[1] = N
    batch = None if batch is None else batch.long().contiguous()
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    rcut = (2.0 * radius.max()).reshape(1)                                   # the largest r_i + r_j
    cl = ops.neighbour_bin(pos, cell, batch, atom_ptr, rcut, flags)
    order = torch.sort(cl.bin_id, stable=True)                              # atoms in bin order; inside a bin by index
    cl.bin_atoms = order.indices.contiguous()
    cl.bin_start = torch.searchsorted(order.values, torch.arange(cl.bins_cap + 1, device=dev)).contiguous()
    counts = ops.neighbour_pairs(pos, radius, batch, cl, flags)
    seg_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    seg_ptr[1:] = torch.cumsum(counts, 0)
    total, fl = torch.stack([seg_ptr[-1], flags[0].long()]).tolist()        # read-back 1 of 2: E' and the error word
    _raise_flags(fl)
    if total == 0:
        raise ValueError("build_internal_graph: the internal graph has no edges")
    keys = ops.neighbour_pairs(pos, radius, batch, cl, flags, seg_ptr=seg_ptr, capacity=total)
    keys = torch.sort(keys).values.contiguous()
    ei, cs, ns = ops.neighbour_decode(keys, cell, batch, N)
    return keys, ei, cs, ns, flags


def match_edges(keys, edge_index, cell_shift) -> torch.Tensor:
    """index of every (i, j, S) row in the sorted key list, -1 where it is absent"""
    want = pack_keys(edge_index, cell_shift)
    idx = torch.searchsorted(keys, want).clamp_(max=int(keys.shape[0]) - 1)
    return torch.where(keys[idx] == want, idx, torch.full_like(idx, -1))


def _make_key(data, radius_type, radius_scale):
    return tuple(_sig(gget(data, k)) for k in ("pos", "cell", "z", "batch", "edge_index", "cell_shift")) + (str(radius_type), float(radius_scale))


def build_internal_graph(data, radius_type="openmx", radius_scale=1.0) -> Graph:
    """the derived graph: z / pos / cell / batch / node_counts of `data`, the internal edge_index / cell_shift (dtypes of the data's) / nbr_shift, and
    matching_edges [E_data]: the internal edge of every data edge, in data-edge order"""
    cell, cshift = gget(data, "cell"), gget(data, "cell_shift")
    if cell is None or cshift is None:
        raise ValueError("build_internal_graph needs data.cell and data.cell_shift (the periodic images of the data's edges)")
    pos, z, batch = gget(data, "pos"), gget(data, "z"), gget(data, "batch")
    pos = pos.contiguous()
    cell = cell.reshape(-1, 3, 3).to(pos.dtype).contiguous()
    tab = radius_table(radius_type, radius_scale, pos.device)
    node_counts = gget(data, "node_counts")
    # (z outside [0, num_types) is refused by the topology check of the forward; the clamp only keeps this look-up inside the table until then)
    keys, ei, cs, ns, flags = neighbour_list(pos, cell, batch, node_counts, tab[z.long().clamp(0, tab.shape[0] - 1)].contiguous())
    e_data = gget(data, "edge_index")
    match = match_edges(keys, e_data, cshift)
    missing, fl = torch.stack([(match < 0).sum(), flags[0].long()]).tolist()   # read-back 2 of 2: "all matched" and the fill pass' error word
    _raise_flags(fl)
    if missing:
        raise ValueError(f"build_internal_graph: {missing} of the data's {int(match.shape[0])} edges are not in the internal graph. "
                         "Please increase radius_scale factor!")
    g = Graph(z=z, pos=pos, cell=cell, edge_index=ei.to(e_data.dtype), cell_shift=cs.to(cshift.dtype), nbr_shift=ns, matching_edges=match)
    if batch is not None:
        g["batch"] = batch
    if node_counts is not None:
        g["node_counts"] = node_counts
    return g


def get_internal_graph(data, radius_type="openmx", radius_scale=1.0) -> Graph:
    """the cached internal graph of `data` (identity + in-place version of pos / cell / z / batch / edge_index / cell_shift, and the radii): an unchanged object
    builds once, `data.pos.add_(...)` rebuilds; Graph.to and parallel.shard_graph do not carry the cache to the graphs they derive"""
    key = _make_key(data, radius_type, radius_scale)
    c = data.get(CACHE_ATTR) if isinstance(data, dict) else getattr(data, "__dict__", {}).get(CACHE_ATTR)
    if c is not None and c[0] == key:
        return c[1]
    g = build_internal_graph(data, radius_type, radius_scale)
    try:
        if isinstance(data, dict):
            dict.__setitem__(data, CACHE_ATTR, (key, g))
        else:
            object.__setattr__(data, CACHE_ATTR, (key, g))
    except Exception:                                          # objects without a __dict__: rebuilt per call
        pass
    return g


def restrict_geometry(geo, rows):
    """the Geometry of the edges `rows` of `geo`: rbf / wig / length / edge_index indexed, nothing recomputed"""
    out = object.__new__(type(geo))
    out.E, out.lmax, out.wig_off, out.nW = int(rows.shape[0]), geo.lmax, geo.wig_off, geo.nW
    out.rbf, out.wig, out.length = geo.rbf[rows].contiguous(), geo.wig[rows].contiguous(), geo.length[rows].contiguous()
    out.edge_index = geo.edge_index[:, rows].contiguous()
    out.src, out.dst = out.edge_index[0].contiguous(), out.edge_index[1].contiguous()
    if hasattr(geo, "D"):                                      # (the CPU suite's stand-in keeps the fp64 Wigner matrices)
        out.D = geo.D[rows.cpu().numpy()]
    return out
