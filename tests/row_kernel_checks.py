"""Case builders and the comparison for the row-streaming kernels (csrc/row_ops.hip, attention.hip, head.hip) -- shared by tests/test_row_kernels_gpu.py
(the HIP kernels through hamgnn_amd.ops) and tests/test_row_kernels_cpu.py (the stand-ins of tests/cpu_ops.py, the coverage conditions, the sharpness of the
comparison).  Device-agnostic: `B` below is the module that provides the entry points (hamgnn_amd.ops or tests.cpu_ops), `dev` the device of its tensors.

A CASE is seeded inputs plus tables, on the CPU, and nothing else (built once per process and shared by every test that needs it; nobody writes to it): a dict with "args" (what the entry point takes), "cover" (its coverage conditions, computed
from the inputs and the fp64 twin alone) and "require" (the conditions that have to hold for this case: a case that misses one is a broken test).  Tables come
from the planner where it can produce them (plan.gate_tables, plan.norm_act_table, plan.attention_head_table -- the `_head_tab_np` of an AttentionBlockE3 --,
the `_slot`, `_cg`, `_mask`, `_blk` of a HamGNNPlusPlusOut); hand-made tables, valid by construction, cover what the planner never emits.

compare(out, ref, scale) is the measure: the largest per-row value of max_p |out - ref| / max_p scale, scale = the twin's sum of absolute terms (|ref| for
element-wise operations).  The bound is gpu_checks.TOL, per row -- per irrep copy for the norm activation."""
import functools
import math
import types

import numpy as np
import torch

from hamgnn_amd import plan as P
from tests import gpu_checks as G
from tests import row_kernel_refs as R

TOL = G.TOL
F32 = torch.float32


def gen(seed):
    return torch.Generator().manual_seed(9000 + seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def compare(out, ref, scale):
    """the largest per-row value of max_p |out - ref| / max_p scale over [rows, P] arrays.  A row whose scale is 0 everywhere (in-degree 0, a masked block,
    a cut weight of exactly 0) has no rounding freedom: any non-zero output there is an infinite error.  NaN / inf on either side: infinite error."""
    out, ref, scale = (torch.as_tensor(t).detach().cpu().double().reshape(ref.shape[0], -1) for t in (out, ref, scale))
    if not (torch.isfinite(out).all() and torch.isfinite(ref).all()):
        return float("inf")
    num, den = (out - ref).abs().amax(1), scale.abs().amax(1)
    err = torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))
    return float(err.max()) if err.numel() else 0.0


def by_channel(t, chan_tab):
    """[rows, D] -> [rows * nchan, max components]: one row per irrep copy (zero-filled), the unit the norm activation is compared on"""
    t = torch.as_tensor(t).detach().cpu().double()
    cols = R._chan_cols(chan_tab)
    width = max(len(c) for c in cols)
    out = torch.zeros(t.shape[0], len(cols), width, dtype=torch.float64)
    for k, c in enumerate(cols):
        out[:, k, :len(c)] = t[:, c]
    return out.reshape(-1, width)


def window(t, lead=4, tail=8):
    """the same values as a column window of a wider buffer: row stride = width + lead + tail (a multiple of 4 when the width is), first column 16-byte aligned"""
    buf = torch.full((t.shape[0], t.shape[1] + lead + tail), float("nan"), dtype=t.dtype)
    buf[:, lead:lead + t.shape[1]] = t
    return buf[:, lead:lead + t.shape[1]]


def to_dev(t, dev):
    """a tensor on the device WITH its strides (a column window stays a window of a wider device buffer)"""
    if t is None or not torch.is_tensor(t):
        return t
    if t.is_contiguous() or dev == "cpu":
        return t.to(dev)
    base = t._base
    assert base is not None and base.is_contiguous()
    return torch.as_strided(base.to(dev), t.shape, t.stride(), t.storage_offset())


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def twice(fn, dev):
    """every kernel is launched twice on the same inputs: returns the first result and whether the second is bit-identical"""
    a = fn()
    a = tuple(t.clone() for t in a) if isinstance(a, tuple) else a.clone()
    b = fn()
    sync(dev)
    if isinstance(a, tuple):
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
        return tuple(t.cpu() for t in a), same
    return a.cpu(), torch.equal(a.view(torch.int32), b.view(torch.int32))


def wrap_rows(rows, wrap, edge=40):
    """rows are independent: for the launches that go round a persistent loop the twin is taken on the first rows, the rows around the wrap and the tail"""
    if rows <= wrap:
        return torch.arange(rows)
    return torch.unique(torch.cat([torch.arange(edge), torch.arange(wrap - edge, min(rows, wrap + edge)), torch.arange(rows - edge, rows)]).clamp(0, rows - 1))


# ================================================================================================ segment_sum
SEG_DEGREES = (0, 1, 3, 4, 5, 2, 8, 9, 0, 13)


def csr(degrees, g, extra=0):
    """receiver CSR with the given in-degrees over a SHUFFLED edge list (perm is no identity); `extra` edges of the list belong to no node"""
    deg = torch.tensor(degrees)
    E = int(deg.sum()) + extra
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
    perm = torch.randperm(E, generator=g)[:int(deg.sum())].contiguous()
    return rowptr, perm, E


@functools.lru_cache(None)
def segment_sum_cases():
    out = {}
    for Dp in (8, 260, 1028):
        for strided in (False, True):
            g = gen(Dp + strided)
            rowptr, perm, E = csr(SEG_DEGREES, g, extra=3)
            msg = randn(g, E, Dp) * torch.exp(2.0 * randn(g, E, 1))          # rows of very different size: the order of the fp32 sum matters
            if strided:
                msg = window(msg)
            cover = {"degrees": sorted(set(SEG_DEGREES)), "second_column_pass": int(Dp > 1024), "msg_stride_differs": int(msg.stride(0) != Dp),
                     "perm_is_shuffled": int(not torch.equal(perm, torch.arange(perm.numel())))}
            req = ["perm_is_shuffled"] + (["second_column_pass"] if Dp > 1024 else []) + (["msg_stride_differs"] if strided else [])
            out[f"Dp{Dp}" + ("_strided" if strided else "")] = {"args": (msg, rowptr, perm, len(SEG_DEGREES)), "cover": cover, "require": req}
    return out


def segment_sum_fp32(msg, rowptr, perm):
    """the sum the kernel's comment promises: sequential, in list order, in fp32 (no fast-math, adds are not contracted): exact to the bit"""
    msg = msg.float()
    N = rowptr.numel() - 1
    out = torch.zeros(N, msg.shape[1], dtype=F32)
    for n in range(N):
        for q in range(int(rowptr[n]), int(rowptr[n + 1])):
            out[n] = out[n] + msg[perm[q]]
    return out


def check_segment_sum(case, B, dev, defect=None):
    msg, rowptr, perm, N = case["args"]
    ref, scale = R.segment_sum(msg, rowptr, perm, defect=defect)
    if B is None:
        return {"err": compare(R.segment_sum(msg, rowptr, perm)[0], ref, scale)}
    a = [to_dev(t, dev) for t in (msg, rowptr, perm)]
    out, same = twice(lambda: B.segment_sum(a[0], a[1], a[2], N), dev)
    return {"err": compare(out, ref, scale), "exact": bool(torch.equal(out, segment_sum_fp32(msg, rowptr, perm))), "repeat": same}


# ================================================================================================ gate
def hand_gate_table():
    """what plan.gate_tables never emits, valid by construction (every input column feeds at most one output; a gate column carries one activation):
    activation ids 3 and 4, activated scalars that are gated as well, structural zeros, input columns no output reads.  Din = 150, Dout = 139."""
    rows, src = [], 0
    for k in range(12):                                        # activated scalars, ids 1..4
        rows.append((src, 1 + k % 4, -1, 0)); src += 1
    gates = list(range(100, 110))                              # ten gate channels, ids 1..4 (and one plain 'gate': id 0)
    gact = [1, 2, 3, 4, 1, 2, 3, 4, 1, 0]
    for k in range(8):                                         # activated scalars that are gated as well
        rows.append((src, 1 + k % 4, gates[k], gact[k])); src += 1
    for k in range(70):                                        # gated components
        rows.append((src, 0, gates[k % 10], gact[k % 10])); src += 1
        if k % 9 == 4:
            rows.append((-1, -1, -1, -1))                      # structural zeros in between
    for k in range(6):                                         # plain copies
        rows.append((src, 0, -1, 0)); src += 1
    for k in range(36):                                        # a tail that takes Dout past two wave passes
        rows.append((110 + k, 0, -1, 0) if k % 5 else (-1, -1, -1, -1))
    return np.asarray(rows, np.int32), 150                     # columns 96..99 and 146..149 are read by nobody


def plain_gate_table():
    """nact = 0: a pure column gather (reversed), one structural zero"""
    rows = [(9 - k, 0, -1, 0) for k in range(10)] + [(-1, -1, -1, -1)]
    return np.asarray(rows, np.int32), 12


def gate_inputs(g, rows, Din, act_cols):
    """3 randn; the activated columns of the first rows sit around the softplus threshold 20 (below, at, above) and far out"""
    x = 3.0 * randn(g, rows, Din)
    special = torch.tensor([19.5, 20.0, 20.000002, 20.5, 35.0, -30.0, 0.0, 1e-4])
    for r in range(min(rows, 4)):
        for j, c in enumerate(act_cols):
            x[r, c] = special[(j + j // 4 + r) % special.numel()]
    return x


@functools.lru_cache(None)
def gate_cases():
    consts = torch.from_numpy(P.ACT_CONSTS.copy())
    tabs = {"planner": (P.gate_tables(G.MINI)[2], P.PlanarLayout(P.gate_tables(G.MINI)[0]).dim), "hand": hand_gate_table(), "plain": plain_gate_table()}
    out = {}
    for tname, (tab4, Din) in tabs.items():
        act_tab, out_tab = P.gate_tables_compact(tab4)
        for rows in ((1, 3, 4, 5, 67, 8192 + 5) if tname != "plain" else (5,)):
            for strided in ((False, True) if rows == 67 else (False,)):
                g = gen(rows + 17 * len(tname) + strided)
                x = gate_inputs(g, rows, Din, [int(c) for c, _ in act_tab])
                gy = randn(g, rows, tab4.shape[0])
                if strided:
                    x, gy = window(x), window(gy)
                ids = {int(a) for s, a, _, _ in tab4 if s >= 0} | {int(ga) for s, _, gt, ga in tab4 if s >= 0 and gt >= 0}
                ssp_cols = [int(c) for c, a in act_tab if a == P.ACT_SSP]
                read = {int(s) for s, _, _, _ in tab4 if s >= 0} | {int(gt) for s, _, gt, _ in tab4 if s >= 0 and gt >= 0}
                cover = {"act_ids": sorted(ids), "nact": int(act_tab.shape[0]), "Dout": int(tab4.shape[0]), "Din": Din,
                         "ssp_above_20": int((x[:, ssp_cols] > 20).sum()) if ssp_cols else 0, "ssp_below_20": int((x[:, ssp_cols] < 20).sum()) if ssp_cols else 0,
                         "ssp_at_20": int((x[:, ssp_cols] == 20).sum()) if ssp_cols else 0,
                         "structural_zeros": int((tab4[:, 0] < 0).sum()), "unread_columns": Din - len(read),
                         "gated_activated": int(((tab4[:, 0] >= 0) & (tab4[:, 1] != 0) & (tab4[:, 2] >= 0)).sum()),
                         "not_multiples_of_64": int(all(v % 64 for v in (tab4.shape[0], Din) + ((act_tab.shape[0],) if act_tab.shape[0] else ()))),
                         "strip_reused": int(rows > 2048 * 4), "strided": int(x.stride(0) != Din)}
                req = ["not_multiples_of_64", "structural_zeros", "unread_columns"] if tname != "plain" else ["structural_zeros", "unread_columns"]
                if tname != "plain":
                    req += ["ssp_above_20", "ssp_below_20", "ssp_at_20"]
                if tname == "hand":
                    req += ["gated_activated"]
                if rows > 8192:
                    req += ["strip_reused"]
                if strided:
                    req += ["strided"]
                out[f"{tname}_rows{rows}" + ("_strided" if strided else "")] = {
                    "args": (x, gy, tab4, (torch.from_numpy(act_tab.copy()), torch.from_numpy(out_tab.copy())), consts), "cover": cover, "require": req,
                    "want_ids": {"planner": [0, 1, 2], "hand": [0, 1, 2, 3, 4], "plain": [0]}[tname]}
    return out


def check_gate(case, B, dev, defect=None, backward=False):
    x, gy, tab4, tabs, consts = case["args"]
    idx = wrap_rows(x.shape[0], 8192)
    zeros = torch.from_numpy(tab4[:, 0] < 0)
    read = {int(s) for s, _, _, _ in tab4 if s >= 0} | {int(gt) for s, _, gt, _ in tab4 if s >= 0 and gt >= 0}
    unread = torch.tensor([c not in read for c in range(x.shape[1])])
    if backward:
        ref, scale = R.gate_backward(x[idx], gy[idx], tab4, consts)
    else:
        ref = R.gate(x[idx], tab4, consts, defect=defect)
        scale = ref.abs()
    if B is None:
        good = R.gate(x[idx], tab4, consts)
        return {"err": compare(good, ref, scale)}
    xd, gyd, cd = to_dev(x, dev), to_dev(gy, dev), consts.to(dev)
    td = tuple(t.to(dev) for t in tabs)
    out, same = twice((lambda: B.gate_backward(xd, gyd, td, cd)) if backward else (lambda: B.gate(xd, td, cd)), dev)
    exact = bool((out[:, unread] == 0).all()) if backward else bool((out[:, zeros] == 0).all())
    return {"err": compare(out[idx], ref, scale), "exact": exact, "repeat": same}


# ================================================================================================ norm activation
NORM_IRREPS = {"mini": G.MINI, "l4": "5x0e+3x1o+2x2e+2x3o+3x4e"}
NORM_SMALL = (1e-4, 1e-3, 1e-2, 3e-2, 0.06, 0.09, 0.0999, 0.1001, 0.11, 0.15, 0.3)      # small norms, and both sides of the kernel's series threshold 0.1


@functools.lru_cache(None)
def norm_cases():
    out = {}
    for name, irr in NORM_IRREPS.items():
        tab = P.norm_act_table(irr)
        D = P.PlanarLayout(irr).dim
        cols = R._chan_cols(tab)
        for rows in (1, 3, 5, 67):
            for strided in ((False, True) if rows == 67 else (False,)):
                g = gen(rows + 1000 * len(name) + strided)
                x, gy = randn(g, rows, D), randn(g, rows, D)
                k = 0
                for r in range(rows):                          # every third irrep copy of a row gets a prescribed norm (direction random), cycling through the classes
                    for c in range(r % 3, len(cols), 3):
                        cls = k % (len(NORM_SMALL) + 7)
                        v = x[r, cols[c]]
                        u = v / v.norm()
                        if cls == 0:
                            x[r, cols[c]] = 0.0                               # clamped: exactly zero
                        elif cls == 1:
                            x[r, cols[c]] = 2e-9 * u                          # clamped: n^2 = 4e-18 < eps^2 = 1e-16
                        elif cls == 2:
                            x[r, cols[c]] = 2e-8 * u                          # just above the clamp
                        elif cls == 3:
                            x[r, cols[c]] = 1e-6 * u
                        elif cls in (4, 5):
                            x[r, cols[c]] = (21.0 + 15.0 * (cls - 4)) * u     # n > 20: the linear branch of the softplus
                        elif cls == 6:
                            x[r, cols[c]] = 19.9 * u
                        else:
                            x[r, cols[c]] = NORM_SMALL[cls - 7] * u
                        k += 1
                if strided:
                    x, gy = window(x), window(gy)
                n = R.norm_classes(x, tab)
                pad = torch.ones(D, dtype=torch.bool)
                pad[[c for cc in cols for c in cc]] = False
                cover = {"clamped": int((n < 1e-8).sum()), "exact_zero": int((n == 0).sum()), "near_clamp": int(((n >= 1e-8) & (n < 1e-7)).sum()),
                         "small": int(((n >= 1e-7) & (n < 0.05)).sum()), "above_20": int((n > 20).sum()), "padding_slots": int(pad.sum()),
                         "lmax": max((len(c) - 1) // 2 for c in cols), "strided": int(x.stride(0) != D)}
                req = ["padding_slots"] + (["clamped", "exact_zero", "near_clamp", "small", "above_20"] if rows >= 5 else []) + (["strided"] if strided else [])
                out[f"{name}_rows{rows}" + ("_strided" if strided else "")] = {"args": (x, gy, torch.from_numpy(tab.copy()), pad), "cover": cover, "require": req}
    return out


def norm_subsets(x, tab):
    """[rows * nchan] masks of the irrep copies by class: what the per-class figures of the norm activation are reported on"""
    n = R.norm_classes(x, tab).reshape(-1)
    return {"clamped": n < 1e-8, "small": (n >= 1e-8) & (n < 0.05), "regular": n >= 0.05}


def check_norm_act(case, B, dev, defect=None, backward=False):
    x, gy, tab, pad = case["args"]
    if backward:
        ref, scale = R.norm_act_backward(x, gy, tab)
    else:
        ref = R.norm_act(x, tab, defect=defect)
        scale = ref.abs() if defect is None else R.norm_act(x, tab).abs()
    if B is None:
        return {"err": compare(by_channel(R.norm_act(x, tab), tab), by_channel(ref, tab), by_channel(scale, tab))}
    xd, gyd, td = to_dev(x, dev), to_dev(gy, dev), tab.to(dev)
    out, same = twice((lambda: B.norm_act_backward(xd, gyd, td)) if backward else (lambda: B.norm_act(xd, td)), dev)
    oc, rc, sc = by_channel(out, tab), by_channel(ref, tab), by_channel(scale, tab)
    res = {"err": compare(oc, rc, sc), "exact": bool((out[:, pad] == 0).all()), "repeat": same}
    for name, m in norm_subsets(x, tab).items():
        res["err_" + name] = compare(oc[m], rc[m], sc[m]) if bool(m.any()) else 0.0
    return res


# ================================================================================================ adds, layout, embedding: exact results
@functools.lru_cache(None)
def exact_cases():
    out = {}
    lay = P.PlanarLayout(G.MINI)
    imap = torch.from_numpy(lay.index_map().astype(np.int32))
    D, Dp = int(imap.numel()), lay.dim
    for rows in (1, 5, 67):
        g = gen(rows)
        out[f"to_planar_rows{rows}"] = {"op": "to_planar", "args": (randn(g, rows, D), imap, Dp), "cover": {"padding_columns": Dp - D}, "require": ["padding_columns"]}
        gmap = imap.clone()
        gmap[torch.randperm(D, generator=g)[:7]] = -1          # the column gathers of the gradient layouts carry -1 entries
        out[f"from_planar_rows{rows}"] = {"op": "from_planar", "args": (randn(g, rows, Dp), gmap), "cover": {"minus_one_entries": int((gmap < 0).sum())},
                                          "require": ["minus_one_entries"]}
        for c3 in (False, True):
            for strided in (False, True):
                a, b, c = (randn(g, rows, 37) * 10.0 ** float(k) for k in (0, -3, 2))
                if strided:
                    a, b, c = window(a, 4, 3), window(b, 8, 3), window(c, 0, 7)
                out[f"add_rows_rows{rows}" + ("_c" if c3 else "") + ("_strided" if strided else "")] = {
                    "op": "add_rows", "args": (a, b, c if c3 else None), "cover": {"strided": int(a.stride(0) != 37), "third": int(c3)},
                    "require": (["strided"] if strided else []) + (["third"] if c3 else [])}
        T, Tp, ntypes = 13, 16, 7
        Ta, Tb = randn(g, ntypes, T), randn(g, ntypes, T) * 1e-2
        z = torch.randint(0, ntypes, (rows,), generator=g)      # (as many atoms as rows: an absent index list is the identity)
        ia, ib = (torch.randint(0, rows, (rows,), generator=g) for _ in range(2))
        for name, (tb, a_, b_) in {"a": (None, None, None), "a_idx": (None, ia, None), "ab_idx": (Tb, ia, ib), "ab_idx_b_only": (Tb, None, ib),
                                   "ab_idx_a_only": (Tb, ia, None), "ab_no_idx": (Tb, None, None)}.items():
            out[f"embed_{name}_rows{rows}"] = {"op": "embed_lookup", "args": (Ta, tb, z, a_, b_, rows, T, Tp),
                                               "cover": {"padding_columns": Tp - T, "second_table_without_idx_b": int(tb is not None and b_ is None)},
                                               "require": ["padding_columns"] + (["second_table_without_idx_b"] if name in ("ab_idx_a_only", "ab_no_idx") else [])}
    return out


def exact_fp32(case):
    """these outputs have no rounding freedom: a copy, or one or two fp32 adds in a fixed order"""
    op, a = case["op"], case["args"]
    if op == "to_planar":
        out = torch.zeros(a[0].shape[0], a[2], dtype=F32)
        out[:, a[1].long()] = a[0]
        return out
    if op == "from_planar":
        out = a[0][:, a[1].long().clamp(min=0)].clone()
        out[:, a[1] < 0] = 0.0
        return out
    if op == "add_rows":
        out = a[0] + a[1]
        return out if a[2] is None else out + a[2]
    Ta, Tb, z, ia, ib, rows, T, Tp = a
    r = torch.arange(rows)
    out = torch.zeros(rows, Tp, dtype=F32)
    out[:, :T] = Ta[z[r if ia is None else ia]]
    if Tb is not None:
        out[:, :T] = out[:, :T] + Tb[z[r if ib is None else ib]]
    return out


def check_exact(case, B, dev):
    op, a = case["op"], case["args"]
    twin = getattr(R, op)(*a)
    if not hasattr(B, op):                                     # (tests/cpu_ops.py has no stand-in for add_rows: nothing calls it on the CPU path)
        return {"err": compare(exact_fp32(case), twin, twin.abs()), "exact": True, "repeat": True}
    ad = [to_dev(t, dev) for t in a]
    out, same = twice(lambda: getattr(B, op)(*ad), dev)
    return {"err": compare(out, twin, twin.abs()), "exact": bool(torch.equal(out, exact_fp32(case))), "repeat": same}


# ================================================================================================ attention
ATTN_DEGREES = (0, 1, 3, 4, 5, 127, 128, 129, 257, 2)
ATTN_CUTOFF, ATTN_CUT_PARAM = 6.0, 10.0                        # cut_param: the initial value of the reference's SoftUnitStepCutoff


def hand_head_table(Dp, H, g):
    """random heads with padding columns (-1) in between: any map column -> head is legal for the kernels"""
    t = torch.randint(0, H, (Dp,), generator=g, dtype=torch.int32)
    t[torch.randperm(Dp, generator=g)[:max(1, Dp // 16)]] = -1
    return t.numpy()


def attn_tables():
    """(head table, H, head_dim) by name: plan.attention_head_table is what an AttentionBlockE3 keeps as _head_tab_np"""
    t = {}
    for name, irr, H in (("Dp8_H1", "8x0e", 1), ("Dp260_H2", "18x0e+14x1o+14x2e+14x3o", 2), ("Dp72_H8", "8x0e+8x1o+8x2e", 8), ("Dp68_H4", "16x0e+8x0o+8x1o+4x2e", 4)):
        tab, hd = P.attention_head_table(irr, H)
        t[name] = (tab, H, hd)
    g = gen(77)
    t["Dp1028_H8_hand"] = (hand_head_table(1028, 8, g), 8, 120)
    t["Dp1028_H3_hand"] = (hand_head_table(1028, 3, g), 3, 330)
    return t


def attn_geo(src, dst, length, dev="cpu"):
    return types.SimpleNamespace(src=src.to(dev), dst=dst.to(dev), length=length.to(dev), E=int(src.numel()))


def attn_lengths(g, E):
    """0.1 .. 0.9 of the cutoff, and a sixth of the edges at the cutoff, just inside it (exp(-1 / x) underflows to 0) and beyond: weight exactly 0.
    Why not 0.9 .. 1: the weight is exp(-1 / x), x = cut_param (1 - r / r_cut); the fp32 quotient r / r_cut is rounded to 6e-8, which is 6e-8 / (1 - r / r_cut)
    of x and (1 / x) times that of the weight -- 6e-7 at 0.9 r_cut, past TOL from 0.97 r_cut on for ANY fp32 evaluation of this input (the reference's included)."""
    length = ATTN_CUTOFF * (0.1 + 0.8 * torch.rand(E, generator=g))
    k = torch.arange(E)
    length[k % 6 == 1] = ATTN_CUTOFF
    length[k % 12 == 3] = ATTN_CUTOFF * 1.25
    length[k % 12 == 9] = ATTN_CUTOFF * (1.0 - 1e-4)
    return length.float()


@functools.lru_cache(None)
def attn_cases():
    out = {}
    for name, (tab, H, hd) in attn_tables().items():
        for strided in ((False, True) if name == "Dp260_H2" else (False,)):
            g = gen(len(name) + 31 * H + strided)
            Dp, N = int(tab.shape[0]), len(ATTN_DEGREES)
            rowptr, perm, E = csr(ATTN_DEGREES, g)
            dst = torch.empty(E, dtype=torch.long)
            dst[perm] = torch.repeat_interleave(torch.arange(N), torch.tensor(ATTN_DEGREES))
            src = torch.randint(0, N, (E,), generator=g)
            K, V = randn(g, N, Dp) * (2.0 / math.sqrt(max(hd, 1)) ** 0.5), randn(g, E, Dp)
            length = attn_lengths(g, E)
            K[4] = 0.0                                          # node 4 (in-degree 5) as receiver: every logit equal (0)
            hub = 7                                             # node 7 (in-degree 129): one logit far above the rest, through one sender that no other edge uses
            e_big = int(perm[int(rowptr[hub]) + 70])
            length[e_big] = 0.3 * ATTN_CUTOFF
            src[src == 9] = 8
            src[e_big] = 9
            w = float(R.soft_cut(length[e_big:e_big + 1], ATTN_CUT_PARAM, ATTN_CUTOFF)) / math.sqrt(hd)
            M = R._head_matrix(tab, H)
            K[9] = (K[hub].double() * ((30.0 + 3.0 * torch.arange(H, dtype=torch.float64)) / (w * ((K[hub].double() ** 2) @ M)))[torch.from_numpy(tab).long().clamp(min=0)]).float()
            if strided:
                K, V = window(K), window(V)
            lg, _ = R.attn_logits(K, src, dst, length, tab, H, hd, ATTN_CUT_PARAM, ATTN_CUTOFF)
            top2 = lg[perm[int(rowptr[hub]):int(rowptr[hub + 1])]].topk(2, 0).values
            e4 = perm[int(rowptr[4]):int(rowptr[5])]
            cover = {"degrees": sorted(set(ATTN_DEGREES)), "zero_weight_edges": int((R.soft_cut(length, ATTN_CUT_PARAM, ATTN_CUTOFF) == 0).sum()),
                     "edges_at_cutoff": int((length == ATTN_CUTOFF).sum()), "edges_beyond": int((length > ATTN_CUTOFF).sum()),
                     "padding_columns": int((tab < 0).sum()), "second_lane_pass": int(Dp > 256), "second_column_pass": int(Dp > 1024), "idle_head_slots": 8 - H,
                     "all_equal_node": int((lg[e4] == lg[e4][0]).all()), "dominant_logit_gap": float((top2[0] - top2[1]).min()), "strided": int(K.stride(0) != Dp)}
            req = ["zero_weight_edges", "edges_at_cutoff", "edges_beyond", "all_equal_node"] + (["strided"] if strided else [])
            req += ["padding_columns"] if "Dp260" in name or "hand" in name else []
            req += ["second_lane_pass"] if Dp > 256 else []
            req += ["second_column_pass"] if Dp > 1024 else []
            out[name + ("_strided" if strided else "")] = {"args": (K, V, src, dst, length, rowptr, perm, torch.from_numpy(tab.copy()), H, hd), "cover": cover, "require": req}
    return out


@functools.lru_cache(None)
def attn_wrap_case():
    """more than 65536 blocks x 4 waves of edges: the grid cap of hg_attn_logits.  Dp = 8, one head."""
    g = gen(4242)
    tab, hd = P.attention_head_table("8x0e", 1)
    E, N = 262144 + 3, 50
    src, dst = torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)
    K = randn(g, N, 8)
    return {"args": (K, None, src, dst, attn_lengths(g, E), None, None, torch.from_numpy(tab.copy()), 1, hd), "cover": {"edges_beyond_grid": E - 65536 * 4},
            "require": ["edges_beyond_grid"]}


def check_attn_logits(case, B, dev, defect=None):
    K, V, src, dst, length, rowptr, perm, tab, H, hd = case["args"]
    idx = wrap_rows(int(src.numel()), 65536 * 4)
    ref, scale = R.attn_logits(K, src[idx], dst[idx], length[idx], tab, H, hd, ATTN_CUT_PARAM, ATTN_CUTOFF, defect=defect)
    if B is None:
        return {"err": compare(R.attn_logits(K, src[idx], dst[idx], length[idx], tab, H, hd, ATTN_CUT_PARAM, ATTN_CUTOFF)[0], ref, scale)}
    Kd, geo, td, cp = to_dev(K, dev), attn_geo(src, dst, length, dev), tab.to(dev), torch.tensor([ATTN_CUT_PARAM], dtype=F32).to(dev)
    out, same = twice(lambda: B.attention_logits(Kd, geo, td, H, hd, cp, ATTN_CUTOFF), dev)
    zero = R.soft_cut(length, ATTN_CUT_PARAM, ATTN_CUTOFF) == 0
    return {"err": compare(out[idx], ref, scale), "exact": bool((out[zero] == 0).all()), "repeat": same, "logits": out}


def check_attn_aggregate(case, B, dev, defect=None, logits=None):
    """hg_attn_aggregate alone: the twin starts from the logits the aggregate kernel itself reads (`logits`: those of hg_attn_logits, checked on their own;
    None: the twin's)"""
    K, V, src, dst, length, rowptr, perm, tab, H, hd = case["args"]
    lg = R.attn_logits(K, src, dst, length, tab, H, hd, ATTN_CUT_PARAM, ATTN_CUTOFF)[0] if logits is None else logits
    ref, scale = R.attn_aggregate(lg, V, rowptr, perm, tab, H, defect=defect)
    if B is None:
        return {"err": compare(R.attn_aggregate(lg, V, rowptr, perm, tab, H)[0], ref, scale)}
    Kd, Vd, geo, td, cp = to_dev(K, dev), to_dev(V, dev), attn_geo(src, dst, length, dev), tab.to(dev), torch.tensor([ATTN_CUT_PARAM], dtype=F32).to(dev)
    out, same = twice(lambda: B.attention_aggregate(Kd, Vd, geo, rowptr.to(dev), perm.to(dev), td, H, hd, cp, ATTN_CUTOFF), dev)
    deg0 = (rowptr[1:] == rowptr[:-1])
    return {"err": compare(out, ref, scale), "exact": bool((out[deg0] == 0).all() and (out[:, tab < 0] == 0).all()), "repeat": same}


# ================================================================================================ read-out head
_HEAD = {}


def planner_head_tables():
    """_slot, _cg, _mask, _blk of a HamGNNPlusPlusOut (openmx, nao 19) compiled for the CPU: nslots = nao^2 = 361 (<= 512), coefficient rows of 300 (<= 512),
    l <= 4: 165 Wigner floats (<= 256)"""
    if not _HEAD:
        from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
        m = HamGNNPlusPlusOut(G.MINI, G.MINI, nao_max=19, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=True, soc_switch=False).compile("cpu")
        _HEAD.update(slot=m._slot.numpy(), cg=tuple(t.numpy() for t in m._cg), mask=m._mask.clone(), blk=m._blk.numpy(), nao=19,
                     cw=P.PlanarLayout(m.onsite_hamiltonian_network.girr).dim, lmax=int(m.hamiltonian_irreps.lmax), Z=sorted(int(k) for k in m.basis_def))
    return _HEAD


def hand_head_tables(nao, cw, lmax, nslots, g):
    """random slot / CSR tables, valid by construction: slot {L <= lmax, a <= 2 L, base, stride} with base + 2 L stride < cw; CSR rows of 0..4 entries"""
    L = torch.randint(0, lmax + 1, (nslots,), generator=g)
    L[:lmax + 1] = torch.arange(lmax + 1)
    a = (torch.rand(nslots, generator=g) * (2 * L + 1)).long()
    stride = torch.randint(1, 9, (nslots,), generator=g)
    base = (torch.rand(nslots, generator=g) * (cw - 2 * L * stride)).long()
    slot = torch.stack([L, a, base, stride], 1).int().numpy()
    cnt = torch.randint(0, 5, (nao * nao,), generator=g)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)]).int().numpy()
    nnz = int(ptr[-1])
    return slot, (ptr, torch.randint(0, nslots, (nnz,), generator=g).int().numpy(), randn(g, nnz).numpy())


HEAD_SHAPES = {"planner": None, "nao23_cw600_L5": (23, 600, 5, 300), "nao4_cw200_L2": (4, 200, 2, 20), "nao10_cw400_L3": (10, 400, 3, 90)}
#                 name: (sign, symmetrize, h0_after_mask, mask, H0, wig, pairs)
HEAD_OPTIONS = {"default": (1.0, True, False, True, True, True, True), "sign_minus": (-1.0, True, False, True, True, True, True),
                "h0_after_mask": (1.0, True, True, True, True, True, True), "no_symmetrize": (1.0, False, False, True, True, True, True),
                "bare": (1.0, True, False, False, False, False, True), "onsite": (1.0, True, False, True, True, False, False),
                "minus_after_nomask": (-1.0, True, True, False, True, True, True)}


def head_geo(wig, lmax, dev="cpu"):
    """what ops.ham_merge / ham_readout read of a Geometry: the packed Wigner rows and their offsets (random matrices: the kernels only contract with them)"""
    from hamgnn_amd import ops
    off, nW = ops.wig_offsets(lmax)
    assert nW == wig.shape[1]
    return types.SimpleNamespace(wig=wig.to(dev), nW=nW, wig_off=off, lmax=lmax, D=wig.double().numpy(), E=wig.shape[0])


def pairing(rows, g, nself=None):
    """every row in exactly one pair slot; about a fifth of the rows (or `nself`) pair with themselves (pair_a == pair_b); the pair count is odd, so the last
    group of two pairs is half empty"""
    nself = max(1, rows // 5) if nself is None else nself
    while (rows - nself) % 2 or ((rows - nself) // 2 + nself) % 2 == 0:
        nself += 1
    p = torch.randperm(rows, generator=g)
    selfs, rest = p[:nself], p[nself:]
    half = rest.numel() // 2
    pa, pb = torch.cat([rest[:half], selfs]), torch.cat([rest[half:], selfs])
    mix = torch.randperm(pa.numel(), generator=g)
    return pa[mix].contiguous(), pb[mix].contiguous()


@functools.lru_cache(None)
def head_cases(wrap=False):
    out = {}
    shapes = {"nao4_cw200_L2": HEAD_SHAPES["nao4_cw200_L2"]} if wrap else HEAD_SHAPES
    for sname, shp in shapes.items():
        for oname, (sign, sym, h0_last, use_mask, use_h0, use_wig, use_pairs) in (HEAD_OPTIONS.items() if not wrap else [("default", HEAD_OPTIONS["default"])]):
            for strided in ((False, True) if (sname == "nao10_cw400_L3" and oname == "default") else (False,)):
                g = gen(len(sname) * 7 + len(oname) + strided)
                if shp is None:
                    t = planner_head_tables()
                    nao, cw, lmax, slot, cg, mask, Z = t["nao"], t["cw"], t["lmax"], t["slot"], t["cg"], t["mask"], t["Z"]
                else:
                    nao, cw, lmax, nslots = shp
                    slot, cg = hand_head_tables(nao, cw, lmax, nslots, g)
                    mask, Z = (torch.rand(9, nao, generator=g) > 0.3).float(), list(range(9))
                rows = (2 * 2560 + 3) if wrap else (1 if oname == "bare" and sname == "nao4_cw200_L2" else 23)
                natoms = 9
                z = torch.tensor(Z)[torch.randint(0, len(Z), (max(natoms, rows),), generator=g)]
                ia, ib = (torch.randint(0, natoms, (rows,), generator=g) for _ in range(2))
                coeff = randn(g, rows, cw)
                nW = P.wigner_offsets(lmax)[1]
                wig = randn(g, rows, nW) if use_wig else None
                pairs = pairing(rows, g, 3 if wrap else None) if use_pairs else None
                H0 = randn(g, rows, nao * nao) if use_h0 else None
                if not use_pairs:
                    ia = ib = None
                if strided:
                    coeff = window(coeff)
                npairs = rows if pairs is None else int(pairs[0].numel())
                nWuse = nW if use_wig else 0
                cover = {"npairs": npairs, "odd_tail": npairs % 2, "self_paired": rows if pairs is None else int((pairs[0] == pairs[1]).sum()),
                         "persistent_groups": max(0, (npairs + 1) // 2 - 1280), "c_width_slot": (cw > 256) + (cw > 512), "nao2_slot": (nao * nao > 256) + (nao * nao > 512),
                         "nWuse_slot": int(nWuse > 256), "empty_csr_rows": int((np.diff(cg[0]) == 0).sum()), "strided": int(coeff.stride(0) != cw),
                         "masked_orbitals": int((mask[z] == 0).sum()) if use_mask else 0}
                req = (["self_paired"] if rows > 1 else []) + (["odd_tail"] if use_pairs and rows > 1 else []) + (["persistent_groups"] if wrap else [])
                req += ["masked_orbitals"] if use_mask else []
                req += ["strided"] if strided else []
                out[f"{sname}_{oname}" + ("_strided" if strided else "") + ("_wrap" if wrap else "")] = {
                    "args": dict(coeff=coeff, wig=wig, lmax=lmax, slot=slot, cg=cg, nao=nao, pairs=pairs, H0=H0, mask=mask if use_mask else None, z=z, ia=ia, ib=ib,
                                 sign=sign, sym=sym, h0_last=h0_last), "cover": cover, "require": req, "want_slots": None if shp is None else
                    ((cw > 256) + (cw > 512), (nao * nao > 256) + (nao * nao > 512), int(lmax == 5 and use_wig))}
    return out


def _head_dev(a, dev):
    geo = head_geo(a["wig"], a["lmax"], dev) if a["wig"] is not None else None
    tabs = (torch.from_numpy(a["slot"].copy()).to(dev),) + tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in a["cg"])
    return geo, tabs


def check_ham_readout(case, B, dev, defect=None, two_launches=False):
    """hg_ham_readout, or the two-launch route hg_ham_merge + hg_ham_finish with the same options (`two_launches`)"""
    a = case["args"]
    rows, nao = a["coeff"].shape[0], a["nao"]
    woff = P.wigner_offsets(a["lmax"])[0]
    idx = torch.arange(rows)
    if a["pairs"] is not None and a["pairs"][0].numel() > 2560:                # the twin on the rows of the first pairs, the pairs around the wrap of the persistent loop, the tail
        sel = wrap_rows(int(a["pairs"][0].numel()), 2560, edge=24)
        idx = torch.unique(torch.cat([a["pairs"][0][sel], a["pairs"][1][sel]]))
    ref, scale = R.ham_readout(a["coeff"], a["wig"], woff, a["slot"], *a["cg"], nao, a["pairs"], a["H0"], a["mask"], a["z"], a["ia"], a["ib"], a["sign"], a["sym"],
                               a["h0_last"], defect=defect) if idx.numel() == rows else _readout_subset(a, idx, woff)
    if B is None:
        good = R.ham_readout(a["coeff"], a["wig"], woff, a["slot"], *a["cg"], nao, a["pairs"], a["H0"], a["mask"], a["z"], a["ia"], a["ib"], a["sign"], a["sym"], a["h0_last"])[0]
        return {"err": compare(good, ref, scale)}
    geo, tabs = _head_dev(a, dev)
    d = {k: to_dev(a[k], dev) for k in ("coeff", "H0", "mask", "z", "ia", "ib")}
    pairs = None if a["pairs"] is None else tuple(t.to(dev) for t in a["pairs"])

    def run():
        if two_launches:
            raw = B.ham_merge(d["coeff"], geo, *tabs, nao * nao)
            inv = None if pairs is None else R.pairs_to_inv(a["pairs"], rows).to(dev)
            return B.ham_finish(raw, inv, d["H0"], d["mask"], d["z"], d["ia"], d["ib"], nao, a["sign"], a["sym"], a["h0_last"])
        out = torch.full((rows, nao * nao), float("nan"), dtype=F32).to(dev)
        return B.ham_readout(d["coeff"], geo, *tabs, nao, pairs, d["H0"], d["mask"], d["z"], d["ia"], d["ib"], out, a["lmax"], a["sign"], a["sym"], a["h0_last"])
    out, same = twice(run, dev)
    return {"err": compare(out[idx], ref, scale), "exact": bool(torch.isfinite(out).all()), "repeat": same}


def _readout_subset(a, idx, woff):
    """the twin on the rows `idx` (closed under the pairing) of a long launch"""
    pos = torch.full((a["coeff"].shape[0],), -1, dtype=torch.long)
    pos[idx] = torch.arange(idx.numel())
    inv = pos[R.pairs_to_inv(a["pairs"], a["coeff"].shape[0])[idx]]
    assert (inv >= 0).all()
    sub = lambda t: None if t is None else t[idx]
    raw, sc = R.ham_merge(a["coeff"][idx], sub(a["wig"]), woff, a["slot"], *a["cg"], a["nao"] ** 2)
    return R.ham_finish(raw, sc, inv, sub(a["H0"]), a["mask"], a["z"], sub(a["ia"]) if a["ia"] is not None else idx, sub(a["ib"]) if a["ib"] is not None else idx,
                        a["nao"], a["sign"], a["sym"], a["h0_last"])


@functools.lru_cache(None)
def finish_cases():
    """hg_ham_finish on its own: the su2 wrap (mask narrower than the matrix), inv = None, a column window of a wider raw buffer"""
    out = {}
    for name, (nao, w, use_inv, sign, h0_last, strided) in {"su2_wrap": (8, 4, True, -1.0, True, False), "no_inv": (6, 6, False, 1.0, False, False),
                                                             "window": (8, 4, True, 1.0, False, True), "single": (1, 1, False, 1.0, False, False)}.items():
        g = gen(len(name) + nao)
        rows = 14
        raw = randn(g, rows, nao * nao)
        if strided:
            raw = window(raw)
        p = torch.randperm(rows, generator=g)
        inv = torch.arange(rows)
        inv[p[:6]], inv[p[6:12]] = p[6:12], p[:6]
        mask = (torch.rand(5, w, generator=g) > 0.3).float()
        z = torch.randint(0, 5, (9,), generator=g)
        ia, ib = (torch.randint(0, 9, (rows,), generator=g) for _ in range(2))
        out[name] = {"args": (raw, inv if use_inv else None, randn(g, rows, nao * nao), mask, z, ia, ib, nao, sign, True, h0_last),
                     "cover": {"mask_narrower": int(w < nao), "strided": int(raw.stride(0) != nao * nao), "no_inv": int(not use_inv)},
                     "require": (["mask_narrower"] if w < nao else []) + (["strided"] if strided else []) + ([] if use_inv else ["no_inv"])}
    return out


def check_ham_finish(case, B, dev, defect=None):
    a = case["args"]
    raw = a[0]
    ref, scale = R.ham_finish(raw, raw.abs(), *a[1:], defect=defect)
    if B is None:
        return {"err": compare(R.ham_finish(raw, raw.abs(), *a[1:])[0], ref, scale)}
    ad = [to_dev(t, dev) for t in a]
    out, same = twice(lambda: B.ham_finish(*ad), dev)
    return {"err": compare(out, ref, scale), "exact": True, "repeat": same}


@functools.lru_cache(None)
def soc_cases():
    out = {}
    t = planner_head_tables()
    for name, (nao, tab) in {"planner_nao19": (19, t["blk"]), "one_full_block": (5, np.tile(np.asarray([[0, 5, 0, 5]], np.int32), (25, 1))),
                             "all_1x1": (4, np.asarray([[q // 4, q // 4 + 1, q % 4, q % 4 + 1] for q in range(16)], np.int32)),
                             "single_orbital": (1, np.asarray([[0, 1, 0, 1]], np.int32))}.items():
        for strided in ((False, True) if name == "planner_nao19" else (False,)):
            g = gen(nao + strided)
            x = randn(g, 7, nao * nao)
            sizes = (tab[:, 1] - tab[:, 0]) * (tab[:, 3] - tab[:, 2])
            out["block_mean_" + name + ("_strided" if strided else "")] = {
                "op": "block_mean", "args": (window(x) if strided else x, torch.from_numpy(tab.copy()), nao),
                "cover": {"blocks_1x1": int((sizes == 1).sum()), "full_block": int((sizes == nao * nao).any()), "largest_block": int(sizes.max()), "strided": int(strided)},
                "require": {"planner_nao19": ["blocks_1x1"], "one_full_block": ["full_block"], "all_1x1": ["blocks_1x1"], "single_orbital": ["blocks_1x1", "full_block"]}[name] +
                (["strided"] if strided else [])}
    for name, (nao, sym, use_inv, zd, h0r, h0i) in {"default": (5, True, True, False, True, True), "zero_diag": (5, True, True, True, True, True),
                                                      "no_symmetrize": (5, False, True, False, True, True), "no_inv": (3, True, False, False, True, True),
                                                      "no_H0r": (5, True, True, True, False, True), "no_H0i": (5, True, True, False, True, False),
                                                      "nao1": (1, True, True, True, True, True)}.items():
        g = gen(100 + len(name) + nao)
        E = 8
        p = torch.randperm(E, generator=g)
        inv = torch.arange(E)
        inv[p[:3]], inv[p[3:6]] = p[3:6], p[:3]
        out["soc_" + name] = {"op": "soc_assemble", "args": (randn(g, E, nao * nao), randn(g, E, nao * nao), randn(g, E, nao * nao, 3).reshape(E, -1), inv if use_inv else None,
                                                              randn(g, E, 4 * nao * nao) if h0r else None, randn(g, E, 4 * nao * nao) if h0i else None, nao, sym, zd),
                              "cover": {"zero_diag": int(zd), "self_paired": int((inv == torch.arange(E)).sum()), "H0r_absent": int(not h0r), "H0i_absent": int(not h0i)},
                              "require": ["self_paired"] + (["zero_diag"] if zd else [])}
    return out


def check_soc(case, B, dev, defect=None):
    op, a = case["op"], case["args"]
    ref, scale = getattr(R, op)(*a, defect=defect)
    if B is None:
        good = getattr(R, op)(*a)[0]
        cat = lambda t: torch.cat(t, 1) if isinstance(t, tuple) else t
        return {"err": compare(cat(good), cat(ref), cat(scale))}
    ad = [to_dev(t, dev) for t in a]
    out, same = twice(lambda: getattr(B, op)(*ad), dev)
    if op == "block_mean":
        return {"err": compare(out, ref, scale), "exact": True, "repeat": same}
    return {"err": max(compare(o, r, s) for o, r, s in zip(out, ref, scale)), "exact": True, "repeat": same}
