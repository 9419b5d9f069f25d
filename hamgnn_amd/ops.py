"""Thin torch-tensor wrappers over the C ABI (include/hamgnn_hip.h).  PyTorch is plumbing here: device memory, streams.
Every function launches hand-written HIP kernels from libhamgnn_hip.so; nothing falls back to torch arithmetic."""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import plan as P
from ._lib import call, strided


def _on_tensor_device(fn):
    """Run the launch with the device of the first tensor argument current (its current stream is then the launch stream): a caller
    that drives a second GPU without torch.cuda.set_device would otherwise enqueue on the wrong device's stream."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        for a in args:
            t = a if torch.is_tensor(a) else (a[0] if isinstance(a, (list, tuple)) and a and torch.is_tensor(a[0]) else None)
            if t is not None:
                if t.is_cuda and t.device.index != torch.cuda.current_device():
                    with torch.cuda.device(t.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapped


def _dev(arr: np.ndarray, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(device)


def require_fp32(module, data=None):
    """The HIP path computes in fp32 (tables, kernels, outputs).  The reference's `precision: 64` flow -- torch.set_default_dtype(float64) + model.to(float64)
    + float64 graph tensors (hamgnn/main.py:469-474, hamgnn/models/hamgnn_conv.py:248-250) -- must not silently come back as fp32-accurate rows: refuse it."""
    why = None
    if torch.get_default_dtype() == torch.float64:
        why = "torch.get_default_dtype() is float64"
    elif module is not None and next((p.dtype for p in module.parameters()), None) == torch.float64:      # (model.to(float64) converts every parameter: the first one tells; O(1) per forward)
        why = "the model's parameters are float64"
    elif data is not None:
        pos = data["pos"] if isinstance(data, dict) else getattr(data, "pos", None)
        if torch.is_tensor(pos) and pos.dtype == torch.float64:
            why = "data.pos is float64"
    if why:
        raise NotImplementedError(f"precision: 64 is not built ({why}): the MI355X path computes in fp32 and does not down-cast silently "
                                  "(reference: hamgnn/main.py:469-474)")


def _require_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("hamgnn_amd: the MI355X hot path needs CUDA(ROCm) tensors; there is no CPU fallback")


PROFILE_EVENTS = None        # bench.py sets this to a list: (start, end, rows, tag) HIP event pairs around the launches of linear_planar, tp_fused and row_program
_NOT_PROFILED = contextlib.nullcontext()


@contextlib.contextmanager
def _event_pair(rows, tag):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()                                       # torch's current stream == the launch stream (_lib.call)
    yield
    ev1.record()
    PROFILE_EVENTS.append((ev0, ev1, rows, tag))


def _profiled(rows, tag):
    """context of one launch: a HIP event pair around it on PROFILE_EVENTS while bench.py collects them"""
    return _NOT_PROFILED if PROFILE_EVENTS is None else _event_pair(rows, tag)


def _residuals(res):
    """(res0, res0_stride, res1, res1_stride) of up to two residual row tensors: pointer and row stride each (column windows of wider rows pass as they
    are), NULL and 0 where there is none"""
    args = []
    for r in (*res, None, None)[:2]:
        args += [strided(r), r.stride(0) if r is not None else 0]
    return args


def _row_slots(ts):
    """(tensors, host array of their row strides) of up to four row tensors by slot, None and 0 for a slot not in use: `src` / `src_stride` and `src_idx` of the
    edge kernels (the typed call turns the tensors into the array of pointers and checks each as a strided() argument)"""
    ts = (*ts, None, None, None, None)[:max(4, len(ts))]
    return ts, (C.c_int64 * 4)(*[t.stride(0) if t is not None else 0 for t in ts])


_NO_WIG_OFF = (C.c_int * 8)()


def _wigner(geo):
    """(wig, nW, wig_off) of a geometry, or NULL, 0 and zero offsets for launches that do not rotate"""
    return (geo.wig, geo.nW, geo.wig_off) if geo is not None else (None, 0, _NO_WIG_OFF)


def _hcache(geo) -> dict:
    """the per-forward cache of hidden radial rows on a geometry object"""
    return geo.__dict__.setdefault("_hcache", {})


S_SPLIT_OFF = os.environ.get("HG_S_SPLIT", "1") == "0"      # A/B switch: the fp32 form of the radial scale (16 fp32 MFMAs per row tile instead of 6 half-precision ones)
W3_SPLIT_PENDING: list = []     # (DeviceProgram, device scalar max |W3|) of refreshed programs whose half-precision range check is still to be read (check_w3_split)
REPLAY_SPLIT = False         # set by graph_capture.CapturedForward while it warms up and captures: launches of the smallest crystals take the finer 2d split
REPLAY_SPLIT_TILES = int(os.environ.get("HG_REPLAY_SPLIT_TILES", "1024"))    # the 2d split while tiles x segments x phase shares stay below this (two rounds of the chip's 512 slots)


_BUILD_CONFIG_OK = False


def check_build_config():
    """the planner's wave / ring counts against the compiled ones of the loaded library (once per process; raises on a mismatch instead of launching a
    schedule the kernel would misread -- the counts are environment-tunable for the A/B scripts under tools/)"""
    global _BUILD_CONFIG_OK
    if _BUILD_CONFIG_OK:
        return
    want = {0: ("HG_IS_WAVES", P.IS_WAVES), 1: ("HG_LITE_WAVES", P.IS_WAVES_LITE), 2: ("HG_LITE_SRING", P.LITE_SRING)}
    for what, (name, val) in want.items():
        got = call("hg_build_config", what)
        if got != int(val):
            raise RuntimeError(f"{name}={val} does not match the loaded library (compiled with {got}): rebuild the variant or unset the variable")
    _BUILD_CONFIG_OK = True


def w3_split_refill(w: torch.Tensor, se, so, dh, dl, scale: float, lo_scale: float) -> torch.Tensor:
    """the split-half-precision twins of the fp32 W3 blocks of the packed weight blob `w`, rewritten IN PLACE by one launch (csrc/radial.hip:hg_w3_split_refill; index
    tensors: DeviceProgram.refresh_w3_split); returns the device scalar max |w 2^s| for the lazy range check (check_w3_split)"""
    mx = torch.empty(1, device=w.device, dtype=torch.float32)
    call("hg_w3_split_refill", w, se, so, dh, dl, se.numel(), scale, lo_scale, mx)
    return mx[0]


def check_w3_split():
    """one host read for all programs refreshed since the last launch: a W3 weight beyond the half-precision range switches that program's launches to the fp32
    form of the radial scale (and back, once the weights have come back)"""
    if not W3_SPLIT_PENDING:
        return
    pend = list(W3_SPLIT_PENDING)
    W3_SPLIT_PENDING.clear()
    mx = torch.stack([m for _, m in pend]).cpu()
    for (dp, _), m in zip(pend, mx.tolist()):
        dp._w3_split_off = not (m <= P.W3_SPLIT_MAX)


class DeviceProgram:
    """A plan.Program uploaded to the GPU."""

    def __init__(self, prog: P.Program, device, schedule: str = "seg"):
        """schedule: "seg" = segment-stationary kernel only (hg_tp_fused); "is" / "auto" = also build the input-stationary
        schedule (hg_tp_is); "auto" silently keeps "seg" when it does not fit; "is_parts" = input-stationary with the output segments
        spread over as many workgroups per 16-edge tile as their LDS tiles need (plan.lds_partition)."""
        self.prog = prog
        self.weights = _dev(prog.weights, device)
        self.segs = _dev(prog.seg_table, device)
        self.items = _dev(prog.item_table, device)
        self.nseg = int(prog.seg_table.shape[0])
        self.hidden = int(prog.hidden_pad)
        self.out_dim = int(prog.out_layout.dim)
        self.lds_bytes = int(prog.tile_floats) * 4
        self.flags = 1 if (prog.item_table.shape[0] and (prog.item_table[:, 0] == P.IT_POST).any()) else 0
        # input-stationary schedule of the same items (csrc/tp_is.hip) when the tiles of all output segments fit the LDS
        self.sched = None
        self._device = device
        self._is_tables = {}                                   # parts -> (IsSchedule, device tables)
        self._is_weights = {}                                  # parts -> weight blob with the schedule's own streams appended (lite_mode runs)
        self._w3_idx = None                                    # refresh_w3_split's index tensors (structural: built on first use)
        self._w3_split_off = False                             # check_w3_split: a refreshed W3 weight left the half-precision range
        if prog.vsegs and schedule not in ("is", "is_parts"):
            raise ValueError("a program with merged items runs on the input-stationary kernel only")
        self.fixed_parts = None                                # "lds": the tiles of all output segments need several workgroups per 16 edges
        if schedule in ("is", "auto", "is_parts"):             # "is_parts": input-stationary, over several workgroups per tile if need be
            try:
                self.sched = self.is_tables(1)[0]
            except NotImplementedError:
                if schedule == "is":
                    raise
                if schedule == "is_parts":
                    self.sched = self.is_tables("lds")[0]
                    self.fixed_parts = "lds"

    def weights_changed(self):
        """after the packed weight blob was rewritten in place (nn.MessagePackBlock.refresh): rebuild what is derived from it"""
        self.refresh_w3_split()
        self._is_weights.clear()                               # (lite programs are recompiled, not refreshed; kept consistent anyway)
        self._is_tables = {k: v for k, v in self._is_tables.items() if v[0].extra_weights is None}

    def refresh_w3_split(self):
        """the split-half-precision twins of the W3 fragment blocks (plan/program.py:w3_split_fill) recomputed ON THE DEVICE from the fp32 blocks of the blob --
        the device-side repack (hamgnn_amd/repack.py) is affine in the parameters, hi = f16(x) / lo = f16(x - hi) is not.  Whether every weight is inside the
        half-precision range is checked lazily, by ONE host read before the next launch (check_w3_split): outside it the launches keep the fp32 form."""
        regs = self.prog.w3_regions
        if not regs:
            return
        if self._w3_idx is None:
            se, so, dh, dl = [], [], [], []
            for off, rtm in regs:
                n = 4 * rtm * 256
                src, dst = P.w3_split_index(rtm)
                se.append(off + src[:, 0]); so.append(off + src[:, 1]); dh.append(off + n + dst[0]); dl.append(off + n + dst[1])
            self._w3_idx = tuple(_dev(np.concatenate(a).astype(np.int64), self._device) for a in (se, so, dh, dl))
        se, so, dh, dl = self._w3_idx
        sc_, lo_ = float(2.0 ** int(self.prog.w3_exp)), float(2.0 ** P.SPLIT_LO_EXP)
        W3_SPLIT_PENDING.append((self, w3_split_refill(self.weights, se, so, dh, dl, sc_, lo_)))

    def part_table_host(self, sc) -> np.ndarray:
        """the schedule's part table as the launch passes it in host memory: [12] (W3 split twins present) cleared when a refreshed weight left the half-precision range"""
        if (self._w3_split_off or S_SPLIT_OFF) and int(sc.part_table[0][12]):
            pt = sc.part_table.copy()
            pt[:, 12] = 0
            return pt
        return sc.part_table

    def is_tables(self, parts):
        """(schedule, device tables) of the input-stationary kernel split into `parts` sub-schedules (built on first use)"""
        if parts not in self._is_tables:
            sc = P.is_schedule(self.prog, parts)
            self._is_tables[parts] = (sc, tuple(_dev(t, self._device) for t in (sc.seg_table, sc.block_table, sc.phase_table, sc.group_table,
                                                                                  sc.item_table, sc.part_table, sc.rowtab)))
            if sc.extra_weights is not None:                   # lite_mode runs: their step streams ride behind the program's weights
                self._is_weights[parts] = torch.cat([self.weights, _dev(sc.extra_weights, self._device, torch.float32)])
        return self._is_tables[parts]

    def is_weights(self, parts) -> torch.Tensor:
        """the weight blob a launch with `parts` sub-schedules reads"""
        return self._is_weights.get(parts, self.weights)

    def is_parts_for(self, rows: int) -> int:
        """How many workgroups share one 16-edge tile.  The chip holds 512 workgroups of this kernel (2 per CU); a launch with fewer
        tiles than that is a latency problem -- every workgroup walks the whole program serially -- so the output segments are spread
        over 8 (or one per segment) workgroups per tile while the extra staging work still fits the idle CUs."""
        if self.fixed_parts is not None:
            return self.fixed_parts
        forced = os.environ.get("HG_IS_PARTS")
        if forced:
            return max(1, int(forced))
        tiles = (rows + 15) // 16
        nseg = int(self.prog.seg_table.shape[0])
        # under hipGraph capture only (graph_capture.CapturedForward; HG_REPLAY_SPLIT = "2d<K>" forces it, "0" forbids it): one workgroup per (output segment,
        # K-th of its phases), tiles ADDED into zero-filled rows -- the one schedule without a fixed summation order, hence never the eager default
        mode = os.environ.get("HG_REPLAY_SPLIT", "2d4" if REPLAY_SPLIT else "0")
        if mode.startswith("2d") and tiles * nseg * int(mode[2:] or 3) <= REPLAY_SPLIT_TILES and not int(self.sched.part_table[0][11]):
            return ("2d", nseg, int(mode[2:] or 3))
        if tiles * nseg <= 512:
            return nseg
        if tiles <= 300 and nseg >= 8:
            return 8
        return 1


class DeviceLinear:
    """plan.LinearTables uploaded to the GPU (hg_linear_planar)"""

    def __init__(self, tabs: P.LinearTables, device, refreshable: bool = False):
        """refreshable: the tables keep their zero blocks, so that the weight blob is an affine map of the flat weight with a fixed structure and can be
        rewritten in place after an optimiser step (nn.E3Linear._refresh)"""
        self.tabs = tabs
        self.refreshable = bool(refreshable)
        self.nitems = int(tabs.items.shape[0])
        self.items, self.units, self.paths = _dev(tabs.items, device), _dev(tabs.units, device), _dev(tabs.paths, device)
        self.weights = _dev(tabs.weights, device)
        self.in_dim, self.out_dim = int(tabs.in_dim), int(tabs.out_dim)


@_on_tensor_device
def linear_planar(dl: DeviceLinear, x: torch.Tensor, res: Sequence[Optional[torch.Tensor]] = (), tag: str = "linear") -> torch.Tensor:
    """o3.Linear on planar rows, one streaming pass (csrc/linear.hip); res: up to two residual row tensors (output layout) added on the way"""
    rows = int(x.shape[0])
    assert x.shape[1] == dl.in_dim
    res = [r for r in res if r is not None]
    assert len(res) <= 2 and all(r.shape == (rows, dl.out_dim) for r in res)
    out = torch.empty(rows, dl.out_dim, device=x.device, dtype=torch.float32)         # every column is written, padding included
    with _profiled(rows, tag):
        call("hg_linear_planar", x, x.stride(0), dl.items, dl.nitems, dl.units, dl.paths, dl.weights, *_residuals(res), rows, out, dl.out_dim)
    return out


LW_ROWS = 1024                     # rows of a chunk of csrc/linear_wgrad.hip
_LW_TABLES: dict = {}


def linear_wgrad_tables(irreps_in, irreps_out, device):
    """(units int32 [nunits, 8] on the device, gather index int64 [numel] into the summed partial blocks, scale float32 [numel]) of the weight
    gradient of o3.Linear(irreps_in -> irreps_out): a unit = 16 input channels x <= 64 output channels of one path; the flat e3nn weight
    (paths (i_in, i_out), each [mul_in, mul_out] row-major, 1 / sqrt(fan_in)) is a gather of the unit blocks.  Cached per signature."""
    key = (str(irreps_in), str(irreps_out), str(device))
    if key not in _LW_TABLES:
        from .so3 import Irreps
        ii, io = Irreps(irreps_in), Irreps(irreps_out)
        li, lo = P.PlanarLayout(ii), P.PlanarLayout(io)
        paths = [(i, k) for i, (_, l1, p1) in enumerate(ii) for k, (_, l2, p2) in enumerate(io) if (l1, p1) == (l2, p2)]
        fan = {}
        for i, k in paths:
            fan[k] = fan.get(k, 0) + ii[i][0]
        units, gather, scale = [], [], []
        for i, k in paths:
            mi, l, _ = ii[i]
            mk = io[k][0]
            ublock = {}
            for u0 in range(0, mi, 16):
                for v0 in range(0, mk, 64):
                    ublock[(u0, v0)] = len(units)
                    units.append([li.off[i], li.mulp[i], lo.off[k], lo.mulp[k], 2 * l + 1, u0, v0, min(64, mk - v0)])
            for u in range(mi):
                for v in range(mk):
                    gather.append(ublock[(u - u % 16, v - v % 64)] * 1024 + (u % 16) * 64 + v % 64)
                    scale.append(1.0 / math.sqrt(fan[k]))
        _LW_TABLES[key] = (_dev(np.asarray(units if units else [[0] * 8], np.int32), device), len(units),
                           torch.tensor(gather, dtype=torch.int64, device=device), torch.tensor(scale, dtype=torch.float32, device=device))
    return _LW_TABLES[key]


def linear_wgrad(irreps_in, irreps_out, x: torch.Tensor, gy: torch.Tensor) -> torch.Tensor:
    """d sum(y * gy) / d weight of an o3.Linear in e3nn's flat layout, all paths in ONE launch of csrc/linear_wgrad.hip + a fixed-order sum over
    the row chunks (x, gy: planar rows of the Linear's input and of the gradient of its output)"""
    _require_gpu(x)                # (ahead of the return that launches nothing)
    units, nunits, gather, scale = linear_wgrad_tables(irreps_in, irreps_out, x.device)
    if nunits == 0:
        return x.new_zeros(0)
    rows = int(x.shape[0])
    assert gy.shape[0] == rows
    nchunk = (rows + LW_ROWS - 1) // LW_ROWS
    part = torch.empty(nchunk, nunits * 1024, device=x.device, dtype=torch.float32)
    call("hg_linear_wgrad", x, x.stride(0), gy, gy.stride(0), rows, units, nunits, part)
    return part.sum(0)[gather] * scale


class BlockGemm:
    """unit table of csrc/block_gemm.hip on the device: units = [(a_off, a_ld, a_trans, b_off, b_ld, b_trans, c_off, c_ld, M, N, K, scale)]"""

    def __init__(self, units, device):
        arr = np.zeros((max(1, len(units)), 12), np.int32)
        for n, u in enumerate(units):
            arr[n, :11] = [int(v) for v in u[:11]]
            arr[n, 11] = np.float32(u[11]).view(np.int32)
        self.nunits = len(units)
        self.max_tiles = max([-(-int(u[8]) // 64) * -(-int(u[9]) // 64) for u in units], default=1)
        self.units_np, self.units = arr, _dev(arr, device)


def use_block_gemm(t: torch.Tensor) -> bool:
    """hg_block_gemm is a HIP entry point: device tensors only (the CPU suite swaps block_gemm for its numpy twin and takes it too)"""
    return (t.is_cuda or block_gemm.__module__ != __name__) and os.environ.get("HG_BLOCK_GEMM", "1") != "0"


def block_gemm(bg: BlockGemm, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """c[c_off + m * c_ld + n] = scale * sum_k op(a)[m, k] op(b)[k, n] for every unit of `bg` (a, b: flat fp32; c: flat fp32 or fp64, written in place)"""
    assert c.dtype in (torch.float32, torch.float64)           # (`void* c`: the one pointer whose type the header leaves to a flag)
    call("hg_block_gemm", a, b, c, c.dtype == torch.float64, bg.units, bg.nunits, bg.max_tiles)
    return c


def wig_offsets(lmax):
    offs, tot = P.wigner_offsets(lmax)
    arr = (C.c_int * 8)(*([int(o) for o in offs] + [0] * (8 - len(offs))))
    return arr, tot


class Geometry:
    """rbf, packed per-edge Wigner matrices and the receiver CSR of one graph batch (computed once per forward)."""

    def __init__(self, pos, edge_index, nbr_shift, cutoff, num_radial, lmax, jtab_dev, rbf_func: str = "bessel"):
        _require_gpu(pos)
        if pos.device.index != torch.cuda.current_device():
            raise RuntimeError(f"hamgnn_amd: make {pos.device} the current device (torch.cuda.set_device) before the forward")
        E = edge_index.shape[1]
        dev = pos.device
        self.E, self.lmax = E, lmax
        self.wig_off, self.nW = wig_offsets(lmax)
        self.rbf = torch.empty(E, num_radial, device=dev, dtype=torch.float32)
        self.wig = torch.empty(E, self.nW, device=dev, dtype=torch.float32)
        self.length = torch.empty(E, device=dev, dtype=torch.float32)
        ang = torch.empty(E, 4, device=dev, dtype=torch.float32)
        pos = pos.contiguous().float()
        self.edge_index = edge_index.contiguous()
        nbr_shift = nbr_shift.contiguous().float()
        call("hg_edge_geometry", pos, self.edge_index, nbr_shift, E, cutoff, num_radial, lmax, jtab_dev, self.rbf, self.wig, self.length, ang)
        if rbf_func == "gaussian":                             # GaussianSmearing(0, cutoff, num_radial) x cosine cutoff, from the lengths
            offs = _gaussian_offsets(float(cutoff), int(num_radial), dev)
            delta = float((offs[2][1] - offs[2][0]).item())    # the reference's width: spacing of its fp32 linspace (host copy, no sync)
            call("hg_radial_basis", self.length, E, 1, cutoff, offs[1], delta, num_radial, self.rbf)
        elif rbf_func != "bessel":
            raise ValueError(f"Unsupported radial basis function on the MI355X path: {rbf_func}")
        self.src = self.edge_index[0].contiguous()
        self.dst = self.edge_index[1].contiguous()


_GAUSS_OFFS = {}


def _gaussian_offsets(cutoff, num_radial, dev):
    key = (cutoff, num_radial, str(dev))
    if key not in _GAUSS_OFFS:
        host = torch.linspace(0.0, cutoff, num_radial, dtype=torch.float32)
        _GAUSS_OFFS[key] = (key, host.to(dev), host)
    return _GAUSS_OFFS[key]


@_on_tensor_device
def radial_hidden(rbf: torch.Tensor, layers: Sequence[torch.Tensor], act_cst: float) -> torch.Tensor:
    """hidden activations of a FullyConnectedNet (every hidden layer: x @ W / sqrt(fan_in) folded into W, normalised SiLU); the kernel holds up to three
    layers per launch, deeper radial MLPs (`radial_MLP` with more than three entries; r6) chain launches -- every layer of the list is a hidden one"""
    if len(layers) > 3:
        return radial_hidden(radial_hidden(rbf, layers[:3], act_cst), layers[3:], act_cst)
    E = rbf.shape[0]
    dims = [int(layers[0].shape[0])] + [int(w.shape[1]) for w in layers]
    W = torch.cat([w.reshape(-1) for w in layers]).contiguous()
    out = torch.empty(E, dims[-1], device=rbf.device, dtype=torch.float32)
    call("hg_radial_hidden", rbf, E, W, (C.c_int * len(dims))(*dims), len(layers), act_cst, out)
    return out


def radial_hidden_cached(geo: "Geometry", layers: Sequence[torch.Tensor], act_cst: float) -> torch.Tensor:
    """radial_hidden(geo.rbf, layers) through the per-forward cache on the geometry object (filled for all weight generators of a
    backbone at once by prefill_radial_hidden; computed singly otherwise)"""
    cache = _hcache(geo)
    key = id(layers[0])
    if key not in cache:
        cache[key] = radial_hidden(geo.rbf, layers, act_cst)
    return cache[key]


def prefill_radial_hidden(geo: "Geometry", generators: Sequence[Sequence[torch.Tensor]], act_cst: float) -> bool:
    """all weight generators of a forward in ONE launch (hg_radial_hidden_multi); False if their shapes do not allow it"""
    H = radial_hidden_multi(geo.rbf, generators, act_cst)
    if H is None:
        return False
    cache = _hcache(geo)
    for m, g in enumerate(generators):
        cache[id(g[0])] = H[m]
    return True


class KanGenerator:
    """the hidden part of one B-spline KAN weight generator (HamGNN_pre.use_kan) packed for csrc/kan.hip and uploaded: knot tables + W' of every layer but the
    last (plan.kan_pack_hidden).  `width` = columns of the rows Phi it produces = rows of the W3' the edge programs were built with (plan.kan_last_layer)."""

    def __init__(self, layers, device):
        blob, self.dims, self.grid_size, self.packed = P.kan_pack_hidden(layers)
        self.blob = _dev(blob, device, torch.float32)
        self.h_pad = (self.dims[-1] + 15) // 16 * 16
        self.width = (self.grid_size + 4) * self.h_pad
        self.shape_key = (tuple(self.dims), self.grid_size)


@_on_tensor_device
def kan_hidden_multi(rbf: torch.Tensor, generators: Sequence[KanGenerator]) -> torch.Tensor:
    """Phi [n, E, width] of SEVERAL KAN weight generators of one shape that read the same basis rows, one launch (hg_kan_hidden)"""
    g0 = generators[0]
    assert all(g.shape_key == g0.shape_key for g in generators), "use_kan: generators of one launch share their layer widths and grid size"
    assert rbf.shape[1] == g0.dims[0]
    E = rbf.shape[0]
    blob = g0.blob if len(generators) == 1 else torch.cat([g.blob for g in generators])
    out = torch.empty(len(generators), E, g0.width, device=rbf.device, dtype=torch.float32)        # the kernel writes every column, padding included
    call("hg_kan_hidden", rbf, E, blob, g0.blob.numel(), len(generators), (C.c_int * len(g0.dims))(*g0.dims), len(g0.dims) - 1, g0.grid_size, bool(g0.packed), out)
    return out


def kan_hidden(rbf: torch.Tensor, gen: KanGenerator) -> torch.Tensor:
    """Phi [E, width] of one KAN weight generator: what the edge kernels take in place of a FullyConnectedNet's hidden rows"""
    return kan_hidden_multi(rbf, [gen])[0]


def kan_hidden_cached(geo: "Geometry", gen: KanGenerator) -> torch.Tensor:
    """kan_hidden(geo.rbf, gen) through the per-forward cache on the geometry object (radial_hidden_cached's; filled by prefill_kan_hidden)"""
    cache = _hcache(geo)
    key = id(gen)
    if key not in cache:
        cache[key] = kan_hidden(geo.rbf, gen)
    return cache[key]


def prefill_kan_hidden(geo: "Geometry", generators: Sequence[KanGenerator]) -> bool:
    """all KAN weight generators of a forward that share a shape in ONE launch each (a backbone: all of them -- 9 for two layers)"""
    groups: dict = {}
    for g in generators:
        groups.setdefault(g.shape_key, []).append(g)
    cache = _hcache(geo)
    for gens in groups.values():
        Phi = kan_hidden_multi(geo.rbf, gens)
        for m, g in enumerate(gens):
            cache[id(g)] = Phi[m]
    return True


def mfma_probe(device, iters: int = 4000, reps: int = 3) -> float:
    """fp32 MFMA TFLOP/s the device sustains right now on random operands (hg_mfma_probe: two waves per SIMD on every CU, nothing but
    v_mfma_f32_16x16x4_f32 in the loop) -- the attainable ceiling bench.py quotes beside the nominal peak."""
    dev = torch.device(device)
    with torch.cuda.device(dev):
        src = torch.randn(65536, device=dev)
        nblocks = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
        out = torch.empty(nblocks * 256, device=dev)
        run = lambda: call("hg_mfma_probe", src, out, nblocks, iters)
        run()
        torch.cuda.synchronize(dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(reps):
            run()
        ev1.record()
        torch.cuda.synchronize(dev)
        ms = ev0.elapsed_time(ev1) / reps
    return nblocks * 4 * iters * 8 * 2048 / (ms * 1e-3) / 1e12


@_on_tensor_device
def radial_hidden_multi(rbf: torch.Tensor, generators: Sequence[Sequence[torch.Tensor]], act_cst: float) -> Optional[torch.Tensor]:
    """hidden activations of SEVERAL radial weight generators that read the same basis rows, one launch: [n, E, 64]; None when a
    generator is not of the shipped 64 -> 64 -> 64 shape (callers then use radial_hidden per generator)."""
    if not generators or any(len(g) != 2 or tuple(g[0].shape) != (64, 64) or tuple(g[1].shape) != (64, 64) for g in generators):
        return None
    if rbf.shape[1] != 64:
        return None
    E = rbf.shape[0]
    W = torch.cat([w.reshape(-1) for g in generators for w in g]).contiguous()
    out = torch.empty(len(generators), E, 64, device=rbf.device, dtype=torch.float32)
    call("hg_radial_hidden_multi", rbf, E, W, len(generators), act_cst, out)
    return out


@_on_tensor_device
def rotate_gather(x: torch.Tensor, idx: Optional[torch.Tensor], geo: Geometry, chan_tab: torch.Tensor, transpose=False,
                  x2: Optional[torch.Tensor] = None, idx2: Optional[torch.Tensor] = None):
    """one or two gathered sources rotated with the same per-edge frames; returns out (or (out, out2))."""
    E = geo.E
    Dp = int(x.shape[1])
    out = torch.empty(E, Dp, device=x.device, dtype=torch.float32)              # the kernel writes every slot incl. zero padding
    out2 = torch.empty(E, Dp, device=x.device, dtype=torch.float32) if x2 is not None else None
    if x2 is not None:
        assert x2.stride(0) == x.stride(0)
    call("hg_rotate_gather", x, x2, x.stride(0), idx, idx2, geo.wig, geo.nW, geo.wig_off, chan_tab, chan_tab.shape[0], E, bool(transpose), out, out2, Dp)
    return out if x2 is None else (out, out2)


@_on_tensor_device
def tp_fused(dp: DeviceProgram, srcs: List[torch.Tensor], rows: int, h2n=None, h2e=None, geo: Optional[Geometry] = None,
             tag: str = "linear", gather: Optional[List[Optional[torch.Tensor]]] = None, rot_mask: int = 0,
             res: Sequence[Optional[torch.Tensor]] = (), reduce=None) -> torch.Tensor:
    """gather / rot_mask (input-stationary schedule only): srcs[i] holds global-frame node rows, gathered by gather[i] and rotated
    into the edge frame inside the kernel (bit i of rot_mask) instead of a separate hg_rotate_gather pass.
    res: up to two residual row tensors in the output's planar layout, added in the epilogue (segment-stationary programs).
    reduce = (eperm, run_id, R) of topo.Topology.receiver_major(): the launch walks the rows in the order eperm and writes the R run sums
    instead of one row per edge (the fused node scatter; input-stationary single-part launches only)."""
    assert (gather is None and rot_mask == 0) or dp.sched is not None
    res = [r for r in res if r is not None]
    assert len(res) <= 2 and (not res or dp.sched is None) and all(r.shape == (rows, dp.out_dim) for r in res)
    parts = dp.is_parts_for(rows) if dp.sched is not None else 1       # decided ONCE per launch (it reads the environment): the allocation, the tables and the weights agree
    assert reduce is None or (dp.sched is not None and parts == 1)
    alloc = torch.zeros if isinstance(parts, tuple) else torch.empty  # (the 2d split ADDS its tiles into zero-filled rows: plan.is_schedule ("2d", P, K))
    out = alloc(rows if reduce is None else reduce[2], dp.out_dim, device=srcs[0].device, dtype=torch.float32)      # the kernel writes every slot incl. zero channel padding
    head = (*_row_slots(srcs), len(srcs), h2n, h2e, dp.hidden, *_wigner(geo))          # (both entry points begin alike)
    with _profiled(rows, tag):
        if dp.sched is not None:
            check_build_config()
            check_w3_split()
            sc, tables = dp.is_tables(parts)
            eperm, run_id = reduce[:2] if reduce is not None else (None, None)
            call("hg_tp_is", *head, dp.is_weights(parts), *tables[:6], np.ascontiguousarray(dp.part_table_host(sc)), sc.part_table.shape[0], tables[6],
                 sc.lds_floats * 4, _row_slots(gather or ())[0], rot_mask, eperm, run_id, out, dp.out_dim, rows)
        else:
            call("hg_tp_fused", *head, dp.weights, dp.segs, dp.nseg, dp.items, out, dp.out_dim, rows, dp.lds_bytes, dp.flags, *_residuals(res))
    return out


_SCATTER_CACHE: "collections.OrderedDict" = collections.OrderedDict()     # LRU over (sort order, counts) of index tensors, bounded in entries AND bytes
_SCATTER_CACHE_MAX_ENTRIES = 64
_SCATTER_CACHE_MAX_BYTES = 256 << 20


def scatter_rows(index: torch.Tensor, src: torch.Tensor, n: int, persistent: bool = True) -> torch.Tensor:
    """out[i] = sum of the rows src[q] with index[q] == i, in a FIXED order (stable sort by index, then a segmented sum): the
    deterministic form of torch.zeros(n, ...).index_add_(0, index, src), whose float atomics make a training step differ from run to run.
    torch tensor ops (sort / segment_reduce), any device; edge-level glue of the backward passes, not a hot kernel.
    persistent = False: `index` is a throw-away view (not a constant of the model or the graph): its sort order is not cached.  The cache holds strong
    references to what it keeps, so it is a small LRU with a byte cap -- the edge-level indices of graphs already discarded do not pin device memory
    (13 MB per 822 k-edge index, 257 entries before)."""
    if src.shape[0] == 0:
        return src.new_zeros((n,) + tuple(src.shape[1:]))
    key = (index.data_ptr(), index._version, int(index.shape[0]), int(n), index.device)
    hit = _SCATTER_CACHE.get(key) if persistent else None
    if hit is None or hit[0] is not index:                     # the index tensors of the backward glue (tp_idx, l_idx, z, the contraction tables) are
        order = torch.sort(index.long(), stable=True).indices  # constants of a model: sorted once (keyed on the tensor object and its version)
        counts = torch.bincount(index.long(), minlength=n)
        if counts.shape[0] != n:                               # an index >= n: index_add_ raised here, segment_reduce(unsafe=True) would return extra rows
            raise IndexError(f"scatter_rows: index {int(index.max())} out of range for {n} rows")
        hit = (index, order, counts)
        if persistent:
            _SCATTER_CACHE[key] = hit
            size = lambda h: sum(t.numel() * t.element_size() for t in h)
            while len(_SCATTER_CACHE) > _SCATTER_CACHE_MAX_ENTRIES or (len(_SCATTER_CACHE) > 1 and sum(size(h) for h in _SCATTER_CACHE.values()) > _SCATTER_CACHE_MAX_BYTES):
                _SCATTER_CACHE.popitem(last=False)
    elif persistent:
        _SCATTER_CACHE.move_to_end(key)
    _, order, counts = hit
    return torch.segment_reduce(src[order].contiguous(), "sum", lengths=counts, axis=0, unsafe=True)


def scatter_cols(index: torch.Tensor, src: torch.Tensor, n: int) -> torch.Tensor:
    """out[:, i] = sum of src[:, q] with index[q] == i (src [rows, Q, ...] -> [rows, n, ...]) in a fixed order: scatter_rows along dim 1,
    the deterministic form of torch.zeros(rows, n, ...).index_add_(1, index, src)."""
    return scatter_rows(index, src.transpose(0, 1).contiguous(), n).transpose(0, 1)


class DeviceRowProgram:
    """plan.RowProgram uploaded to the GPU (csrc/rowprog.hip)"""

    def __init__(self, rp: "P.RowProgram", device):
        self.rp = rp
        self.stages = _dev(rp.stages, device)
        self.units = _dev(rp.units if rp.units.size else np.zeros((1, P.RP_UNIT_I32), np.int32), device)
        self.weights = _dev(rp.weights, device, torch.float32)
        self.act_tab = _dev(rp.act_tab if rp.act_tab.size else np.zeros((1, 2), np.int32), device)
        self.out_tab = _dev(rp.out_tab if rp.out_tab.size else np.zeros((1, 2), np.int32), device)
        self.consts = (C.c_float * 5)(*[float(c) for c in P.ACT_CONSTS])


@_on_tensor_device
def row_program(drp: DeviceRowProgram, x: torch.Tensor, res: Sequence[torch.Tensor] = (), row_idx: Optional[torch.Tensor] = None, tag: str = "row_program") -> torch.Tensor:
    """run a plan.RowProgram on planar rows x [rows, din] (rows gathered by row_idx when given) -> [rows, dout] (+ the rows in `res`)"""
    rp = drp.rp
    x = x if x.stride(1) == 1 else x.contiguous()
    rows = int(row_idx.shape[0]) if row_idx is not None else int(x.shape[0])
    assert x.shape[1] >= rp.din and len(res) <= 2
    y = torch.empty(rows, rp.dout, device=x.device, dtype=torch.float32)
    r = [t if t.stride(1) == 1 else t.contiguous() for t in res]
    with _profiled(rows, tag):
        call("hg_row_program", x, x.stride(0), row_idx, rp.din, y, y.stride(0), rp.dout, *_residuals(r), drp.stages, rp.stages.shape[0], drp.units,
             drp.weights, drp.act_tab, drp.out_tab, rp.act_tab.shape[0], rp.out_tab.shape[0], drp.consts, rp.in_buf, rp.out_buf, rp.rs[0], rp.rs[1], rp.strip, rows)
    return y


class DeviceWgFused:
    """plan.WgFused uploaded to the GPU (fused weight-gradient kernel, csrc/tp_wgrad.hip)"""

    def __init__(self, wf: "P.WgFused", device):
        self.wf = wf
        self.units = _dev(wf.units, device)
        self.weights = _dev(wf.weights, device, torch.float32)
        self.chtab = _dev(wf.chtab, device)
        self.tp_pos = [None if t is None else torch.from_numpy(t).to(device) for t in wf.tp_pos]
        self.tp_scale = [None if t is None else torch.from_numpy(np.asarray(t, dtype=np.float32)).to(device) for t in wf.tp_scale]
        self.l_pos = [torch.from_numpy(t).to(device) for t in wf.l_pos]

    def nsplit_for(self, rows: int) -> int:
        """edge splits of a launch: enough workgroups to fill the chip several times over, at least a few iterations each"""
        tiles = (rows + 15) // 16
        return int(max(1, min(64, -(-8192 // int(self.units.shape[0])), tiles // 8)))      # measured (profiles/r03_wgrad.md): 8 -> 64 splits 11.5 -> 9.3 ms at 44 k edges


def tp_wgrad(dwf: DeviceWgFused, srcs: Sequence[Optional[torch.Tensor]], g: torch.Tensor, h_node: torch.Tensor, h_edge: Optional[torch.Tensor],
             nsplit: Optional[int] = None):
    """one launch of the fused weight-gradient kernel over all rows of `g`: (acc [nsplit, acc_floats], [gs per branch [rows, n_channels]]).
    srcs: edge-frame planar source rows by slot (None for slots the block does not use)."""
    _require_gpu(g)                # (g.device is made current below)
    wf = dwf.wf
    rows = int(g.shape[0])
    S = int(nsplit or dwf.nsplit_for(rows))
    acc = torch.zeros(S, wf.acc_floats, device=g.device, dtype=torch.float32)
    alloc = torch.empty if wf.gs_complete else torch.zeros      # (every channel of every row is written by exactly one wave when the row tiles cover all channels)
    gs = [alloc(rows, n, device=g.device, dtype=torch.float32) for n in wf.nch]
    keep = [(t if t.stride(1) == 1 else t.contiguous()) if t is not None else None for t in srcs]      # (column windows of wider rows pass as they are: pointer + row stride)
    for t in keep:
        assert t is None or (t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0), "hg_tp_wgrad stages float4 pieces of fp32 rows"
    g = g.contiguous()
    h_node = h_node.contiguous()
    h_edge = h_edge.contiguous() if h_edge is not None else None
    assert h_node.shape[1] >= wf.hidden and (h_edge is None or h_edge.stride(0) == h_node.stride(0))
    gs1 = gs[1] if len(gs) > 1 else None
    with torch.cuda.device(g.device):
        call("hg_tp_wgrad", *_row_slots(keep), len(srcs), g, g.stride(0), h_node, h_edge, h_node.stride(0), wf.hidden, gs[0], gs[0].stride(0),
             gs1, gs1.stride(0) if gs1 is not None else 0, acc, wf.acc_floats, S, dwf.units, dwf.units.shape[0], dwf.weights, dwf.chtab, wf.lds_bytes, rows)
    return acc, gs


@_on_tensor_device
def segment_sum(msg: torch.Tensor, rowptr: torch.Tensor, perm: torch.Tensor, N: int) -> torch.Tensor:
    Dp = msg.shape[1]
    out = torch.empty(N, Dp, device=msg.device, dtype=torch.float32)
    call("hg_segment_sum", strided(msg), msg.stride(0), rowptr, perm, N, Dp, out, Dp)
    return out


@_on_tensor_device
def attention_aggregate(K: torch.Tensor, V: torch.Tensor, geo: "Geometry", rowptr, perm, head_tab: torch.Tensor, H: int, head_dim: int,
                        cut_param: torch.Tensor, cutoff: float) -> torch.Tensor:
    """AttentionAggregation of the reference (hamgnn/nn/attention.py:126-164) with key = K[sender], query = K[receiver] and the soft
    cutoff weight: [N, Dp] planar node rows from [E, Dp] planar value rows."""
    N, Dp, E = int(K.shape[0]), int(K.shape[1]), geo.E
    assert V.shape == (E, Dp)
    logits = torch.empty(E, H, device=K.device, dtype=torch.float32)
    call("hg_attn_logits", strided(K), K.stride(0), geo.src, geo.dst, geo.length, head_tab, Dp, H, cut_param, cutoff, 1.0 / math.sqrt(head_dim), E, logits)
    out = torch.empty(N, Dp, device=K.device, dtype=torch.float32)
    call("hg_attn_aggregate", logits, H, strided(V), V.stride(0), rowptr, perm, head_tab, N, Dp, out, Dp)
    return out


@_on_tensor_device
def attention_logits(K: torch.Tensor, geo: "Geometry", head_tab: torch.Tensor, H: int, head_dim: int, cut_param: torch.Tensor, cutoff: float) -> torch.Tensor:
    """[E, H] soft-cutoff-weighted per-head dot products of the two gathered key rows (the first half of attention_aggregate; used on its
    own by the edge-sharded attention, which needs the per-node soft-max statistics of the rank's edges)"""
    Dp, E = int(K.shape[1]), geo.E
    logits = torch.empty(E, H, device=K.device, dtype=torch.float32)
    call("hg_attn_logits", strided(K), K.stride(0), geo.src, geo.dst, geo.length, head_tab, Dp, H, cut_param, cutoff, 1.0 / math.sqrt(head_dim), E, logits)
    return logits


@_on_tensor_device
def gate(x: torch.Tensor, tabs, consts: torch.Tensor) -> torch.Tensor:
    """tabs = (act_tab [nact,2], out_tab [Dout,2]) device int32 tensors of plan.gate_tables_compact"""
    act_tab, out_tab = tabs
    rows, Dout = x.shape[0], int(out_tab.shape[0])
    out = torch.empty(rows, Dout, device=x.device, dtype=torch.float32)
    call("hg_gate", strided(x), x.stride(0), act_tab, act_tab.shape[0], out_tab, Dout, consts, rows, out, Dout)
    return out


NORM_ACT_EPS = 1e-8          # epsilon of the reference's NormActivation (interaction_blocks.py:329)


def norm_act(x: torch.Tensor, chan_tab: torch.Tensor) -> torch.Tensor:
    """e3nn NormActivation (ssp, normalize, eps 1e-8) on planar rows; chan_tab = plan.norm_act_table(irreps) on the device"""
    rows, D = x.shape
    out = torch.empty(rows, D, device=x.device, dtype=torch.float32)
    call("hg_norm_act", strided(x), x.stride(0), chan_tab, chan_tab.shape[0], NORM_ACT_EPS, rows, out, D, D)
    return out


def norm_act_backward(x: torch.Tensor, gy: torch.Tensor, chan_tab: torch.Tensor) -> torch.Tensor:
    assert gy.shape == x.shape
    rows, D = x.shape
    gx = torch.empty(rows, D, device=x.device, dtype=torch.float32)
    call("hg_norm_act_backward", strided(x), x.stride(0), strided(gy), gy.stride(0), chan_tab, chan_tab.shape[0], NORM_ACT_EPS, rows, gx, D, D)
    return gx


@_on_tensor_device
def add_rows(a, b, c=None):
    """a + b (+ c) on [rows, D] rows; column windows of wider rows pass as they are (pointer and row stride), the sum comes back contiguous"""
    rows, D = a.shape
    out = torch.empty(rows, D, device=a.device, dtype=a.dtype)
    call("hg_add_rows", strided(a), a.stride(0), strided(b), b.stride(0), strided(c), c.stride(0) if c is not None else 0, rows, D, out, D)
    return out


@_on_tensor_device
def to_planar(x: torch.Tensor, imap: torch.Tensor, Dp: int) -> torch.Tensor:
    x = x.contiguous().float()
    out = torch.empty(x.shape[0], Dp, device=x.device, dtype=torch.float32)
    call("hg_to_planar", x, x.shape[0], x.shape[1], imap, out, Dp)
    return out


@_on_tensor_device
def from_planar(xp: torch.Tensor, imap: torch.Tensor) -> torch.Tensor:
    D = int(imap.shape[0])
    out = torch.empty(xp.shape[0], D, device=xp.device, dtype=torch.float32)
    call("hg_from_planar", xp, xp.shape[0], xp.shape[1], imap, out, D)
    return out


@_on_tensor_device
def embed_lookup(Ta, Tb, z, idx_a, idx_b, rows, T, Tp):
    out = torch.empty(rows, Tp, device=Ta.device, dtype=torch.float32)
    call("hg_embed_lookup", Ta, Tb, z, idx_a, idx_b, rows, T, Tp, out)
    return out


@_on_tensor_device
def gate_backward(x: torch.Tensor, gy: torch.Tensor, tabs, consts: torch.Tensor) -> torch.Tensor:
    """data gradient of gate(x, tabs, consts): [rows, Din] from the gate input rows and the gradient of the gate output rows"""
    act_tab, out_tab = tabs
    rows, Din, Dout = x.shape[0], int(x.shape[1]), int(out_tab.shape[0])
    assert gy.shape == (rows, Dout)
    gx = torch.empty(rows, Din, device=x.device, dtype=torch.float32)
    call("hg_gate_backward", strided(x), x.stride(0), strided(gy), gy.stride(0), act_tab, act_tab.shape[0], out_tab, Dout, consts, rows, Din, gx, Din)
    return gx


@_on_tensor_device
def ham_merge(coeff, geo: Optional[Geometry], slot_tab, cg_ptr, cg_idx, cg_val, nout):
    rows = coeff.shape[0]
    out = torch.empty(rows, nout, device=coeff.device, dtype=torch.float32)
    call("hg_ham_merge", strided(coeff), coeff.stride(0), *_wigner(geo), slot_tab, slot_tab.shape[0], cg_ptr, cg_idx, cg_val, nout, rows, out)
    return out


@_on_tensor_device
def ham_finish(Hraw, inv, H0, orb_mask, z, idx_a, idx_b, nao, sign=1.0, symmetrize=True, h0_after_mask=False, out=None):
    """Hraw: [rows, >= nao^2] (a column slice of a wider buffer is fine: the row stride is passed on).
    out: optional contiguous [rows, nao^2] destination (e.g. the row range of the [N+E, nao^2] result: no torch.cat afterwards)."""
    rows = Hraw.shape[0]
    if out is None:
        out = torch.empty(rows, nao * nao, device=Hraw.device, dtype=torch.float32)
    assert out.shape == (rows, nao * nao)
    mask_w = int(orb_mask.shape[1]) if orb_mask is not None else 0
    call("hg_ham_finish", strided(Hraw), Hraw.stride(0), inv, H0, orb_mask, mask_w, z, idx_a, idx_b, nao, sign, bool(symmetrize) | 2 * bool(h0_after_mask), rows, out)
    return out


@_on_tensor_device
def ham_readout(coeff, geo: Optional[Geometry], slot_tab, cg_ptr, cg_idx, cg_val, nao, pairs, H0, orb_mask, z, idx_a, idx_b, out,
                lmax_ham, sign=1.0, symmetrize=True, h0_after_mask=False):
    """one-pass non-SOC read-out of `coeff` rows into `out` [rows, nao^2]; pairs = (pair_a, pair_b) int64 row indices or None (rows pair
    with themselves: on-site)."""
    rows = coeff.shape[0]
    assert out.shape == (rows, nao * nao)
    pa, pb = pairs if pairs is not None else (None, None)
    npairs = rows if pa is None else pa.shape[0]
    mask_w = int(orb_mask.shape[1]) if orb_mask is not None else 0
    call("hg_ham_readout", strided(coeff), coeff.stride(0), coeff.shape[1], *_wigner(geo), lmax_ham, slot_tab, slot_tab.shape[0], cg_ptr, cg_idx, cg_val, cg_idx.shape[0], nao,
         pa, pb, npairs, H0, orb_mask, mask_w, z, idx_a, idx_b, sign, bool(symmetrize) | 2 * bool(h0_after_mask), out)
    return out


@_on_tensor_device
def block_mean(x, tab, nao):
    rows = x.shape[0]
    out = torch.empty(rows, nao * nao, device=x.device, dtype=torch.float32)
    call("hg_block_mean", strided(x), x.stride(0), tab, nao, rows, out)
    return out


@_on_tensor_device
def soc_assemble(H, ksi, L, inv, H0r, H0i, nao, symmetrize=True, zero_diag=False):
    rows = H.shape[0]
    outr = torch.empty(rows, 4 * nao * nao, device=H.device, dtype=torch.float32)
    outi = torch.empty_like(outr)
    call("hg_soc_assemble", H, ksi, L, inv, H0r, H0i, nao, bool(symmetrize), bool(zero_diag), rows, outr, outi)
    return outr, outi


@_on_tensor_device
def hk_assemble(on, off, nbr_shift, kvec, pair_ptr, pair_edges, pair_ij, n_atoms, nao, orank, ooff, M):
    """[nk, M, M] complex64 k-space matrix of one crystal in the compact orbital basis (see include/hamgnn_hip.h:hg_hk_assemble)"""
    nk = int(kvec.shape[0])
    out = torch.zeros(nk, M, M, 2, device=on.device, dtype=torch.float32)
    call("hg_hk_assemble", on, off, nbr_shift, kvec, nk, pair_ptr, pair_edges, pair_ij, pair_ij.shape[0], n_atoms, nao, orank.to(torch.int32).contiguous(), ooff, M, out)
    return torch.view_as_complex(out)


@_on_tensor_device
def hk_assemble_adjoint(G, nbr_shift, kvec, pair_ptr, pair_edges, pair_ij, n_atoms, n_edges, nao, orank, ooff, M):
    """(g_on [n_atoms, nao^2], g_off [n_edges, nao^2]) from the gradient G [nk, M, M] complex64 with respect to H(k) of one crystal: the
    adjoint of hk_assemble on the same pair tables (see include/hamgnn_hip.h:hg_hk_assemble_adjoint); every output element is written"""
    _require_gpu(G)
    nk = int(kvec.shape[0])
    if G.dtype != torch.complex64 or tuple(G.shape) != (nk, M, M):
        raise ValueError(f"hk_assemble_adjoint: G must be complex64 [{nk}, {M}, {M}], got {G.dtype} {tuple(G.shape)}")
    if nk <= 0 or M <= 0 or n_atoms <= 0:                      # (the entry point launches nothing then)
        return (torch.zeros(n_atoms, nao * nao, device=G.device, dtype=torch.float32), torch.zeros(n_edges, nao * nao, device=G.device, dtype=torch.float32))
    Gr = torch.view_as_real(G.contiguous())
    g_on = torch.empty(n_atoms, nao * nao, device=G.device, dtype=torch.float32)
    g_off = torch.empty(n_edges, nao * nao, device=G.device, dtype=torch.float32)
    call("hg_hk_assemble_adjoint", Gr, nbr_shift, kvec, nk, pair_ptr, pair_edges, pair_ij, pair_ij.shape[0], n_atoms, n_edges, nao,
         orank.to(torch.int32).contiguous(), ooff, M, g_on, g_off)
    return g_on, g_off


@_on_tensor_device
def mulliken_weights(C_, SC, perm, gptr, wk, Gp):
    """W [ns, Gp] fp32 from the eigenvector rows C_ and S(k) c rows SC, both [ns, M] complex64: column 0 = wk, column 1 + g = wk * the Mulliken
    weight of orbital group g (perm / gptr int32), pad columns 0 (see include/hamgnn_hip.h:hg_mulliken_weights); every element is written"""
    ns, M = int(C_.shape[0]), int(C_.shape[1])
    G = int(gptr.shape[0]) - 1
    if C_.dtype != torch.complex64 or SC.dtype != torch.complex64 or tuple(SC.shape) != (ns, M) or tuple(wk.shape) != (ns,):
        raise ValueError(f"mulliken_weights: C and SC must be complex64 [{ns}, {M}] and wk [{ns}], got {C_.dtype} {tuple(C_.shape)}, {SC.dtype} {tuple(SC.shape)}, {tuple(wk.shape)}")
    if perm.dim() != 1 or gptr.dim() != 1 or G < 0:
        raise ValueError("mulliken_weights: perm and gptr must be 1-d tensors, gptr with at least one entry")
    if Gp < 1 + G:
        raise ValueError(f"mulliken_weights: Gp = {Gp} holds no room for the state weight and {G} groups")
    W = torch.empty(ns, Gp, device=C_.device, dtype=torch.float32)
    call("hg_mulliken_weights", torch.view_as_real(C_.contiguous()), torch.view_as_real(SC.contiguous()), ns, M, perm, gptr, G, Gp, wk, W)
    return W


def _dos_out(who, D, ne, Gp, accumulate, device):
    """the D [ne, Gp] fp32 that dos_broaden / dos_tetra write: the caller's, checked, or a new one (which accumulate cannot add to)"""
    if D is None:
        if accumulate:
            raise ValueError(f"{who}: accumulate needs the D to add to")
        return torch.empty(ne, Gp, device=device, dtype=torch.float32)
    if tuple(D.shape) != (ne, Gp):
        raise ValueError(f"{who}: D must be [{ne}, {Gp}], got {tuple(D.shape)}")
    return D


@_on_tensor_device
def dos_broaden(eps, W, E0, dE, ne, sigma, D=None, accumulate=False):
    """D [ne, Gp] fp32 (+)= Gaussians of width sigma around the ASCENDING eps [ns], weighted by W [ns, Gp], on the grid E0 + j dE (see
    include/hamgnn_hip.h:hg_dos_broaden).  accumulate adds to the given D; otherwise every element of D is written."""
    if W.dim() != 2 or tuple(eps.shape) != (W.shape[0],):
        raise ValueError(f"dos_broaden: W must be [ns, Gp] and eps [ns], got {tuple(W.shape)}, {tuple(eps.shape)}")
    ns, Gp = int(W.shape[0]), int(W.shape[1])
    D = _dos_out("dos_broaden", D, ne, Gp, accumulate, W.device)
    call("hg_dos_broaden", eps, W, ns, Gp, E0, dE, ne, sigma, bool(accumulate), D)
    return D


@_on_tensor_device
def dos_tetra(eps, W, tet, kt, band_lo, band_hi, E0, dE, ne, mode=0, D=None, accumulate=False):
    """D [ne, Gp] fp32 (+)= the linear tetrahedron method's DOS (mode 0) or number of states (mode 1) on the grid E0 + j dE: eps [nk, nb] ascending in b,
    W [nk, nb, Gp], tet int32 [nt, 4], kt = (kt_ptr [nk + 1], kt_tet [4 nt], kt_corner [4 nt]) int32 (dos.corner_table), band_lo / band_hi [nb] = min / max
    of eps over k (see include/hamgnn_hip.h:hg_dos_tetra).  accumulate adds to the given D; otherwise every element of D is written."""
    if W.dim() != 3 or eps.dim() != 2 or tet.dim() != 2 or len(kt) != 3:
        raise ValueError(f"dos_tetra: eps must be [nk, nb], W [nk, nb, Gp], tet [nt, 4] and kt three tensors, got {tuple(eps.shape)}, {tuple(W.shape)}, {tuple(tet.shape)}")
    nk, nb, Gp = (int(v) for v in W.shape)
    nt = int(tet.shape[0])
    kt_ptr, kt_tet, kt_corner = kt
    if any(t.dtype != torch.float32 for t in (eps, W, band_lo, band_hi)) or any(t.dtype != torch.int32 for t in (tet, kt_ptr, kt_tet, kt_corner)):
        raise ValueError("dos_tetra: eps, W, band_lo and band_hi must be float32, tet and the corner table int32")          # (tests/test_dos_tetra_cpu.py matches these words)
    if (tuple(eps.shape) != (nk, nb) or tuple(tet.shape) != (nt, 4) or tuple(kt_ptr.shape) != (nk + 1,) or tuple(kt_tet.shape) != (4 * nt,)
            or tuple(kt_corner.shape) != (4 * nt,) or tuple(band_lo.shape) != (nb,) or tuple(band_hi.shape) != (nb,)):
        raise ValueError(f"dos_tetra: shapes do not fit nk = {nk}, nb = {nb}, nt = {nt}: eps {tuple(eps.shape)}, tet {tuple(tet.shape)}, kt_ptr {tuple(kt_ptr.shape)}, "
                         f"kt_tet {tuple(kt_tet.shape)}, kt_corner {tuple(kt_corner.shape)}, band_lo {tuple(band_lo.shape)}, band_hi {tuple(band_hi.shape)}")
    if Gp < 1 or mode not in (0, 1):
        raise ValueError(f"dos_tetra: Gp = {Gp} must be at least 1 and mode = {mode!r} 0 (DOS) or 1 (number of states)")
    D = _dos_out("dos_tetra", D, ne, Gp, accumulate, W.device)
    call("hg_dos_tetra", eps, W, nk, nb, Gp, tet, nt, kt_ptr, kt_tet, kt_corner, band_lo, band_hi, E0, dE, ne, mode, bool(accumulate), D)
    return D


@_on_tensor_device
def bond_weights(C_, kidx, kvec, X_on, X_off, erow, ecol, shift, orank, ooff, eptr, eidx, aptr, aidx, wk, Gp):
    """W [ns, Gp] fp32 of bond groups from the eigenvector rows C_ [ns, M] complex64 and the real-space rows X_on [N, nao^2] / X_off [E, nao^2]: column 0 =
    wk, column 1 + g = wk * (sum of Re(phase c_i^+ X_off[e] c_j) over the edges eidx[eptr[g]:eptr[g + 1]] + sum of Re(c_i^+ X_on[i] c_i) over the atoms
    aidx[aptr[g]:aptr[g + 1]]), pad columns 0 (see include/hamgnn_hip.h:hg_bond_weights); every element is written.  kidx int32 [ns] -> rows of kvec
    [nk, 3]; erow / ecol int32 [E], shift [E, 3]; orank int32 [N, nao], ooff int32 [N].  All tables are checked here, on the host, before the launch."""
    _require_gpu(C_)               # (the tables are read below, ahead of the launch)
    G = int(eptr.shape[0]) - 1 if eptr.dim() else -1
    i32, f32 = torch.int32, torch.float32
    ns, M, N, nao, E, nk = check_state_tables("bond_weights", C_, kidx, kvec, erow, ecol, shift, orank, ooff, extra=(
        ("X_on", X_on, ("N", "nao2"), f32), ("X_off", X_off, ("E", "nao2"), f32), ("wk", wk, ("ns",), f32), ("eptr", eptr, (G + 1,), i32),
        ("aptr", aptr, (G + 1,), i32), ("eidx", eidx, (int(eidx.numel()),), i32), ("aidx", aidx, (int(aidx.numel()),), i32)))
    if G < 0 or Gp < 1 + G:
        raise ValueError(f"bond_weights: Gp = {Gp} holds no room for the state weight and {G} groups")
    for name, p, iname, idx, n in (("eptr", eptr, "eidx", eidx, E), ("aptr", aptr, "aidx", aidx, N)):
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError(f"bond_weights: {iname} has entries outside [0, {n})")
        ph = p.cpu()
        if int(ph[0]) != 0 or int(ph[-1]) != idx.numel() or bool((ph[1:] < ph[:-1]).any()):
            raise ValueError(f"bond_weights: {name} must ascend from 0 to the {idx.numel()} entries of its index list")
    W = torch.empty(ns, Gp, device=C_.device, dtype=torch.float32)
    call("hg_bond_weights", torch.view_as_real(C_), ns, M, kidx, kvec, nk, X_on, X_off, erow, ecol, shift, E, N, nao, orank, ooff, eptr, eidx, aptr, aidx, G, Gp, wk, W)
    return W


def check_state_tables(who, C_, kidx, kvec, erow, ecol, shift, orank, ooff, extra=()):
    """The host checks the kernels on eigenvector rows share (hg_bond_weights, hg_density_rows, hg_kgrad_elements; any device, so the torch paths run them too): C_ complex64
    [ns, M]; kidx int32 [ns] -> rows of kvec fp32 [nk, 3]; erow / ecol int32 [E] -> atoms, shift fp32 [E, 3]; orank int32 [N, nao], ooff int32 [N] inside the
    M columns of C_.  extra: (name, tensor, shape, dtype) of the caller's further tensors, a shape entry either a number or one of "ns", "M", "N", "nao",
    "nao2", "E", "nk".  dtype, shape, device and contiguity of every tensor, then the index ranges (a device-to-host copy of two scalars each).  Each
    ValueError starts with `who` and names its argument -> (ns, M, N, nao, E, nk)"""
    if not isinstance(C_, torch.Tensor) or C_.dim() != 2 or C_.dtype != torch.complex64:
        raise ValueError(f"{who}: C must be complex64 [ns, M], got {getattr(C_, 'dtype', type(C_).__name__)} {tuple(getattr(C_, 'shape', ()))}")
    ns, M = int(C_.shape[0]), int(C_.shape[1])
    if orank.dim() != 2:
        raise ValueError(f"{who}: orank must be [N, nao], got {tuple(orank.shape)}")
    N, nao = int(orank.shape[0]), int(orank.shape[1])
    E, nk = int(erow.shape[0]) if erow.dim() else -1, int(kvec.shape[0]) if kvec.dim() else -1
    dims = {"ns": ns, "M": M, "N": N, "nao": nao, "nao2": nao * nao, "E": E, "nk": nk}
    i32, f32 = torch.int32, torch.float32
    named = (("kidx", kidx, ("ns",), i32), ("kvec", kvec, ("nk", 3), f32), ("erow", erow, ("E",), i32), ("ecol", ecol, ("E",), i32),
             ("shift", shift, ("E", 3), f32), ("orank", orank, ("N", "nao"), i32), ("ooff", ooff, ("N",), i32)) + tuple(extra)
    for name, t, shape, dtype in named:
        shape = tuple(dims.get(d, d) for d in shape)
        if t.dtype != dtype:
            raise ValueError(f"{who}: {name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)}, got {list(t.shape)}")
        if t.device != C_.device:                              # (the typed call asks for a GPU tensor, not for this GPU)
            raise ValueError(f"{who}: {name} is on {t.device}, C on {C_.device}")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
    if N < 1 or nk < 1 or M < 1 or not 1 <= nao <= 48:
        raise ValueError(f"{who}: needs at least one atom, one k-point and one orbital and nao <= 48, got N = {N}, nk = {nk}, M = {M}, nao = {nao}")
    for name, t, n in (("kidx", kidx, nk), ("erow", erow, N), ("ecol", ecol, N)):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
            raise ValueError(f"{who}: {name} has entries outside [0, {n})")
    top = torch.where(orank >= 0, ooff[:, None] + orank, torch.zeros_like(orank))
    if int(orank.min()) < -1 or int(ooff.min()) < 0 or int(top.max()) >= M:
        raise ValueError(f"{who}: orank / ooff point outside the {M} compact orbitals of C")
    return ns, M, N, nao, E, nk


def density_rows_check(C_, kidx, kvec, f, erow, ecol, shift, orank, ooff, out, accumulate):
    """the host checks of density_rows (any device; the torch path of hamgnn_amd/density.py runs them too): check_state_tables with f and, where given,
    `out` = (P_on, P_off), which accumulate needs -> (ns, M, N, nao, E, nk)"""
    extra = [("f", f, ("ns",), torch.float32)]
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("density_rows: out must be the pair (P_on, P_off)")
        extra += [("out[0] (P_on)", out[0], ("N", "nao2"), torch.float32), ("out[1] (P_off)", out[1], ("E", "nao2"), torch.float32)]
    elif accumulate:
        raise ValueError("density_rows: accumulate needs the out = (P_on, P_off) to add to")
    return check_state_tables("density_rows", C_, kidx, kvec, erow, ecol, shift, orank, ooff, extra)


@_on_tensor_device
def density_rows(C_, kidx, kvec, f, erow, ecol, shift, orank, ooff, out=None, accumulate=False):
    """(P_on [N, nao^2], P_off [E, nao^2]) fp32 (+)= the density matrix sum_s f[s] Re(phase conj(c_ia) c_jb) sampled on the on-site and edge rows of one crystal
    from the eigenvector rows C_ [ns, M] complex64 (see include/hamgnn_hip.h:hg_density_rows).  kidx int32 [ns] -> rows of kvec [nk, 3]; f fp32 [ns]; erow /
    ecol int32 [E], shift [E, 3]; orank int32 [N, nao], ooff int32 [N].  accumulate adds to the given out = (P_on, P_off); otherwise every element is
    written (into out if given).  All tables are checked here, on the host, before the launch."""
    _require_gpu(C_)               # (the tables are read below, ahead of the launch)
    ns, M, N, nao, E, nk = density_rows_check(C_, kidx, kvec, f, erow, ecol, shift, orank, ooff, out, accumulate)
    P_on, P_off = out if out is not None else (torch.empty(N, nao * nao, device=C_.device, dtype=torch.float32),
                                               torch.empty(E, nao * nao, device=C_.device, dtype=torch.float32))
    if ns == 0 and accumulate:                                 # no state: nothing to add (without accumulate the launch writes the zero rows)
        return P_on, P_off
    if not C_.is_contiguous():
        raise ValueError("density_rows: C must be contiguous")
    call("hg_density_rows", torch.view_as_real(C_), ns, M, kidx, kvec, nk, f, erow, ecol, shift, E, N, nao, orank, ooff, bool(accumulate), P_on, P_off)
    return P_on, P_off


def kgrad_elements_check(C_, bra, ket, kidx, kvec, X_off, erow, ecol, shift, rvec, orank, ooff):
    """the host checks of kgrad_elements (any device; the torch path of hamgnn_amd/velocity.py runs them too): check_state_tables with the rows, rvec and the
    pair lists, then bra / ket inside the states of C and both states of every pair at one k-point -> (ns, M, N, nao, E, nk, np)"""
    for name, t in (("bra", bra), ("ket", ket)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"kgrad_elements: {name} must be int32 [np], got {tuple(getattr(t, 'shape', ()))}")
    npair = int(bra.shape[0])
    i32, f32 = torch.int32, torch.float32
    ns, M, N, nao, E, nk = check_state_tables("kgrad_elements", C_, kidx, kvec, erow, ecol, shift, orank, ooff, extra=(
        ("X_off", X_off, ("E", "nao2"), f32), ("rvec", rvec, ("E", 3), f32), ("bra", bra, (npair,), i32), ("ket", ket, (npair,), i32)))
    for name, t in (("bra", bra), ("ket", ket)):
        if npair and (int(t.min()) < 0 or int(t.max()) >= ns):
            raise ValueError(f"kgrad_elements: {name} has entries outside the {ns} states of C")
    if npair and bool((kidx[bra.long()] != kidx[ket.long()]).any()):
        raise ValueError("kgrad_elements: bra and ket of a pair must lie at the same k-point (kidx[bra] != kidx[ket] somewhere)")
    return ns, M, N, nao, E, nk, npair


@_on_tensor_device
def kgrad_elements(C_, bra, ket, kidx, kvec, X_off, erow, ecol, shift, rvec, orank, ooff):
    """out [np, 3] complex64: out[p, alpha] = sum_e i rvec[e, alpha] phase_e(k_p) c_bra^+ X_off[e] c_ket, the elements of d X(k) / d k_alpha between the rows
    bra[p] and ket[p] of C_ [ns, M] complex64 at the k-point kvec[kidx[ket[p]]] (see include/hamgnn_hip.h:hg_kgrad_elements).  bra / ket int32 [np]; kidx
    int32 [ns] -> rows of kvec [nk, 3]; X_off [E, nao^2], rvec [E, 3] fp32; erow / ecol int32 [E], shift [E, 3]; orank int32 [N, nao], ooff int32 [N].  All
    tables are checked here, on the host, before the launch.  The scratch of the edge split is allocated here, its size asked of the library."""
    _require_gpu(C_)               # (the tables are read below, ahead of the launch)
    ns, M, N, nao, E, nk, npair = kgrad_elements_check(C_, bra, ket, kidx, kvec, X_off, erow, ecol, shift, rvec, orank, ooff)
    out = torch.empty(npair, 3, device=C_.device, dtype=torch.complex64)
    if npair == 0:
        return out
    if not C_.is_contiguous():
        raise ValueError("kgrad_elements: C must be contiguous")
    nbytes = call("hg_scratch_bytes", b"hg_kgrad_elements", npair, E)
    part = torch.empty(nbytes // 4, device=C_.device, dtype=torch.float32) if nbytes > 0 else None
    call("hg_kgrad_elements", torch.view_as_real(C_), ns, M, bra, ket, npair, kidx, kvec, nk, X_off, erow, ecol, shift, rvec, E, N, nao, orank, ooff, part,
         torch.view_as_real(out))
    return out


@_on_tensor_device
def zero_point_shift(H, Href, S, nao, soc=False, threshold=1e-6):
    """in place on H; returns the shift (device scalar)."""
    rows = S.shape[0]
    nparts = 256
    scratch = torch.empty(2 * nparts, device=H.device, dtype=torch.float64)
    shift = torch.empty(1, device=H.device, dtype=torch.float32)
    call("hg_zero_point_shift", H, Href, S, rows, nao, bool(soc), threshold, scratch, nparts, shift)
    return shift


@_on_tensor_device
def sym_contraction3(h, z, C, tab, W3, out):
    """adds the nu = 3 term of a `correlation: 3` block to the rows `out` that sym_contraction returned (in place; csrc/sym_contraction.hip)"""
    call("hg_sym_contraction3", h, h.stride(0), z, h.shape[0], C, tab["num_ell"], tab["ell_off"], tab["nout"], tab["out_off"], tab["ptr3"], tab["ent3"], W3, W3.shape[1],
         out, out.stride(0))
    return out


@_on_tensor_device
def sym_contraction_nu(nu, h, z, C, tab, W, out):
    """adds the term of order nu (1 ... 4) of the symmetric contraction to the rows `out` (in place; csrc/sym_contraction.hip): the nu = 4 term of a
    `correlation: 4` block onto what sym_contraction / sym_contraction3 wrote, or every term onto zeros (HG_CORR_KERNEL=nu)"""
    h = h.contiguous()
    call("hg_sym_contraction_nu", nu, h, h.stride(0), z, h.shape[0], C, tab["num_ell"], tab["ell_off"], tab["nout"], tab["out_off"], tab[f"ptr{nu}"], tab[f"ent{nu}"],
         W, W.shape[1], out, out.stride(0))
    return out


SYM_NU_RUN = 32        # nodes of one element a lane of the weight-gradient kernel walks; the runs of an element are added in order afterwards


def _element_runs(z, T, run):
    """nodes sorted by element (stably: index order inside an element) and cut into runs of at most `run` nodes of ONE element, without a host
    sync: (run_ptr int32[G + 1], nodes int32[N], element of every run int64[G], G) with G = ceil(N / run) + T >= the runs in use (the rest are empty)"""
    N, dev = int(z.shape[0]), z.device
    zl = z.long()
    order = torch.sort(zl, stable=True).indices
    zs = zl[order]
    counts = torch.bincount(zl, minlength=T)
    if counts.shape[0] != T:
        raise IndexError(f"sym_contraction_nu_backward: an element index beyond the {T} weight blocks")
    nrun = (counts + run - 1) // run
    run_end = torch.cumsum(nrun, 0)
    rank = torch.arange(N, device=dev) - (torch.cumsum(counts, 0) - counts)[zs]
    G = (N + run - 1) // run + T
    gid = (run_end - nrun)[zs] + rank // run
    run_ptr = torch.zeros(G + 1, device=dev, dtype=torch.int64)
    run_ptr[1:] = torch.cumsum(torch.bincount(gid, minlength=G), 0)
    elem = torch.searchsorted(run_end, torch.arange(G, device=dev), right=True).clamp_(max=T - 1)
    return run_ptr.to(torch.int32), order.to(torch.int32), elem, G


@_on_tensor_device
def sym_contraction_nu_backward(nu, h, z, C, tab, W, g_out, g_h, per_node=False):
    """adjoint of the term of order nu (hg_sym_contraction_nu_backward): the gradient with respect to the hidden rows is ADDED onto g_h [N, Dp] in
    place, the gradient with respect to W [T, K, C] returned.  tab holds the transposed tables ptrH{nu} / entH{nu} / ptrW{nu} / entW{nu}
    (plan.sym_contraction_adjoint_tables).  per_node: one weight block per node (z = arange(N), charge doping) -> one gradient block per node.
    Otherwise a lane sums a run of SYM_NU_RUN nodes of one element in index order and the runs of an element are added in order
    (scatter_rows: a fixed order, no atomics)."""
    _require_gpu(h)
    h, g_out = h.contiguous(), g_out.contiguous()
    N, T, K = int(h.shape[0]), int(W.shape[0]), int(W.shape[1])
    if N == 0:
        return torch.zeros_like(W)
    if per_node:
        assert T == N, "per-node weights: one block per node"
        run_ptr = nodes = elem = None
        G = N
    else:
        run_ptr, nodes, elem, G = _element_runs(z, T, SYM_NU_RUN)
    gW = torch.empty(G, K, C, device=h.device, dtype=torch.float32)
    call("hg_sym_contraction_nu_backward", nu, h, h.stride(0), g_out, g_out.stride(0), z, N, C, tab["num_ell"], tab["ell_off"], tab["nout"], tab["out_off"],
         tab[f"ptrH{nu}"], tab[f"entH{nu}"], tab[f"ptrW{nu}"], tab[f"entW{nu}"], W, K, G, run_ptr, nodes, g_h, g_h.stride(0), gW)
    if per_node:
        return gW
    return scatter_rows(elem, gW.reshape(G, K * C), T, persistent=False).reshape(T, K, C)


@_on_tensor_device
def sym_contraction(h, z, C, tab, W1, W2, out_dim):
    """tab: device tensors of plan.sym_contraction_tables; W1 [nel, K1, C], W2 [nel, K2, C]; returns planar hidden rows [N, out_dim]"""
    N = h.shape[0]
    out = torch.zeros(N, out_dim, device=h.device, dtype=torch.float32)           # channel padding stays zero
    call("hg_sym_contraction", h, h.stride(0), z, N, C, tab["num_ell"], tab["ell_off"], tab["nout"], tab["out_off"], tab["ptr1"], tab["ent1"], tab["ptr2"], tab["ent2"],
         W1, W1.shape[1], W2, W2.shape[1], out, out_dim)
    return out


# ------------------------------------------------------------------------------------------------ periodic neighbour list (HamGNN_pre.build_internal_graph)
class CellList:
    """what hg_neighbour_bin leaves for the pair passes: per-crystal parameters, the bin of every atom and its wrap into the home cell, and (filled by the caller
    from a sort of bin_id) the atoms in bin order with the first slot of every bin"""

    def __init__(self, cpar, ipar, bin_id, wrap, bins_cap, B):
        self.cpar, self.ipar, self.bin_id, self.wrap, self.bins_cap, self.B = cpar, ipar, bin_id, wrap, int(bins_cap), int(B)
        self.bin_atoms = self.bin_start = None


@_on_tensor_device
def neighbour_bin(pos: torch.Tensor, cell: torch.Tensor, batch, atom_ptr: torch.Tensor, rcut: torch.Tensor, flags: torch.Tensor) -> CellList:
    """hg_neighbour_bin: pos [N, 3] fp32, cell [B, 3, 3] fp32, batch [N] int64 or None (one crystal), atom_ptr [B + 1] int64, rcut: fp64 device scalar (the largest
    r_i + r_j), flags: int32 device error word"""
    N, B = int(pos.shape[0]), int(cell.shape[0])
    assert (batch is None or batch.shape[0] == N) and tuple(cell.shape[1:]) == (3, 3) and atom_ptr.shape[0] == B + 1
    dev = pos.device
    bins_cap = N + 27 * B
    cl = CellList(torch.empty(B, 20, device=dev, dtype=torch.float64), torch.empty(B, 8, device=dev, dtype=torch.int32), torch.empty(N, device=dev, dtype=torch.int64),
                  torch.empty(N, 3, device=dev, dtype=torch.int32), bins_cap, B)
    call("hg_neighbour_bin", pos, cell, batch, atom_ptr, rcut, N, B, bins_cap, cl.cpar, cl.ipar, cl.bin_id, cl.wrap, flags)
    return cl


@_on_tensor_device
def neighbour_pairs(pos: torch.Tensor, radius: torch.Tensor, batch, cl: CellList, flags: torch.Tensor, seg_ptr=None, capacity: int = 0) -> torch.Tensor:
    """hg_neighbour_pairs: seg_ptr None -> the count pass, edges per centre [N] int64; else the fill pass, one packed key per edge [capacity] int64 (centre i's in
    seg_ptr[i] .. seg_ptr[i + 1], unordered inside)"""
    _require_gpu(pos)              # (ahead of the return that launches nothing)
    N = int(pos.shape[0])
    assert radius.shape[0] == N and cl.bin_atoms.shape[0] == N and cl.bin_start.shape[0] == cl.bins_cap + 1
    if seg_ptr is None:
        out = torch.empty(N, device=pos.device, dtype=torch.int64)
        counts, keys = out, None
    else:
        assert seg_ptr.shape[0] == N + 1
        out = torch.empty(int(capacity), device=pos.device, dtype=torch.int64)
        counts, keys = None, out
        if capacity == 0:
            return out
    call("hg_neighbour_pairs", pos, radius, batch, cl.cpar, cl.ipar, cl.bin_id, cl.wrap, cl.bin_start, cl.bin_atoms, N, cl.B, cl.bins_cap, seg_ptr, capacity, counts, keys, flags)
    return out


@_on_tensor_device
def neighbour_decode(keys: torch.Tensor, cell: torch.Tensor, batch, N: int):
    """hg_neighbour_decode: sorted packed keys -> (edge_index [2, E] int64, cell_shift [E, 3] int64, nbr_shift [E, 3] fp32 = S @ cell in fp64, rounded once)"""
    E, dev = int(keys.shape[0]), keys.device
    ei = torch.empty(2, E, device=dev, dtype=torch.int64)
    cs = torch.empty(E, 3, device=dev, dtype=torch.int64)
    ns = torch.empty(E, 3, device=dev, dtype=torch.float32)
    call("hg_neighbour_decode", keys, E, cell, batch, N, cell.shape[0], ei, cs, ns)
    return ei, cs, ns
