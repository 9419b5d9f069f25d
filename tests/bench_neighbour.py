"""Micro-benchmark of the device neighbour list of HamGNN_pre.build_internal_graph (hamgnn_amd/internal_graph.py, hg_neighbour_* in csrc/neighbour.hip) on
sio2_10k, at radius_scale 1.01 (the reference's config default) and 1.5 (and on sio2_3000 at 1.5, where the forward's edge rows stay below 2^31 elements):
  * the whole build (build_internal_graph: binning, count, prefix sum, fill, key sort, decode, matching, with its two read-backs), host clock around a
    device synchronise, median over `reps` after `warmup` builds;
  * its passes one by one, each between a synchronise before and after (so the pass times do not add up to the build exactly);
  * synthetic.build_graph (cKDTree on the host) of the same crystal at the same scale, once;
  * one backbone forward (set-A irreps, 3 layers) on the internal graph -- the work the build feeds -- median over `reps`;
  * the edge counts, and that the device list equals the host list.
One JSON line per scale; --md writes the table of profiles/internal_graph.md."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from hamgnn_amd import internal_graph as IG, ops
from hamgnn_amd.data import synthetic as S
from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3

ap = argparse.ArgumentParser(); ap.add_argument("--cases", default="sio2_10k:1.01,sio2_10k:1.5,sio2_3000:1.5", help="workload:radius_scale, ...")
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--no-forward", action="store_true"); ap.add_argument("--md", default="")
a = ap.parse_args()
dev = torch.device("cuda")


def wall(fn, reps=a.reps, warmup=a.warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), out


def passes(g, scale):
    """the passes of IG.neighbour_list + IG.match_edges, one by one"""
    pos, cell, batch = g.pos.contiguous(), g.cell.reshape(-1, 3, 3).contiguous(), g.batch
    N = pos.shape[0]
    radius = IG.radius_table("openmx", scale, dev)[g.z].contiguous()
    atom_ptr = torch.tensor([0, N], device=dev)
    rcut = (2.0 * radius.max()).reshape(1)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    t = {}
    t["bin"], *_, cl = wall(lambda: ops.neighbour_bin(pos, cell, batch, atom_ptr, rcut, flags))

    def sort_bins():
        o = torch.sort(cl.bin_id, stable=True)
        cl.bin_atoms = o.indices.contiguous()
        cl.bin_start = torch.searchsorted(o.values, torch.arange(cl.bins_cap + 1, device=dev)).contiguous()
    t["bin_sort"], *_ = wall(sort_bins)
    t["count"], *_, counts = wall(lambda: ops.neighbour_pairs(pos, radius, batch, cl, flags))
    seg_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    t["prefix_and_readback"], *_, total = wall(lambda: (seg_ptr[1:].copy_(torch.cumsum(counts, 0)), int(seg_ptr[-1]))[1])
    t["fill"], *_, keys = wall(lambda: ops.neighbour_pairs(pos, radius, batch, cl, flags, seg_ptr=seg_ptr, capacity=total))
    t["key_sort"], *_, skeys = wall(lambda: torch.sort(keys).values.contiguous())
    t["decode"], *_ = wall(lambda: ops.neighbour_decode(skeys, cell, batch, N))
    t["match"], *_ = wall(lambda: int((IG.match_edges(skeys, g.edge_index, g.cell_shift) < 0).sum()))
    assert int(flags[0]) == 0
    return {k: round(v, 3) for k, v in t.items()}, [int(v) for v in cl.ipar[0].tolist()]


rows, graphs = [], {}
for workload, scale in ((c.split(":")[0], float(c.split(":")[1])) for c in a.cases.split(",")):
    if workload not in graphs:
        graphs[workload] = bench.make_graph(workload, 19)
    graph = graphs[workload]
    gd = graph.to(dev)
    t0 = time.perf_counter()
    host = S.build_graph(graph.pos.numpy().astype(np.float64), graph.cell[0].numpy().astype(np.float64), graph.z.numpy(), radius_scale=scale)
    host_ms = (time.perf_counter() - t0) * 1e3
    med, lo, hi, ig = wall(lambda: IG.build_internal_graph(gd, "openmx", scale))
    equal = all(torch.equal(ig[k].cpu(), host[k]) for k in ("edge_index", "cell_shift", "nbr_shift"))
    per_pass, ipar = passes(gd, scale)
    r = {"workload": workload, "radius_scale": scale, "atoms": graph.num_nodes, "edges_data": graph.num_edges, "edges_internal": int(ig.edge_index.shape[1]),
         "bins": ipar[:3], "device_build_ms_median": round(med, 3), "device_build_ms_min": round(lo, 3), "device_build_ms_max": round(hi, 3), "passes_ms": per_pass,
         "host_build_graph_ms": round(host_ms, 1), "equals_host_list": equal}
    # the edge kernels have been run up to 822 350 rows of 868 floats; a row tensor of 2^31 elements or more (sio2_10k at 1.5: 2.8 M rows) is beyond what they
    # were validated at, so that forward is not run here -- the same crystal type at 3 000 atoms gives the build / forward ratio at 1.5
    Dp = 868
    if not a.no_forward and r["edges_internal"] * Dp >= 2 ** 31:
        r.update(forward_on_internal_graph_ms_median="not measured (edge rows of 2^31 elements or more)")
    elif not a.no_forward:
        torch.manual_seed(666)
        m = HamGNNConvE3(dict(bench.make_cfg(bench.IRREPS["A"]), build_internal_graph=True, radius_scale=scale))
        with torch.no_grad():
            fwd, flo, fhi, rep = wall(lambda: m(gd), reps=max(3, a.reps // 2), warmup=2)       # (the internal graph is cached on gd after the first call)
        r.update(forward_on_internal_graph_ms_median=round(fwd, 2), forward_ms_min=round(flo, 2), forward_ms_max=round(fhi, 2), build_over_forward=round(med / fwd, 4),
                 checksum=float(rep["_node_planar"].double().abs().mean()))
        del m, rep
        torch.cuda.empty_cache()
    rows.append(r)
    print(json.dumps(r), flush=True)

if a.md:
    with open(a.md, "w") as f:
        f.write("| workload | radius_scale | atoms | data edges | internal edges | bins | device build, median ms (min .. max) | host build_graph ms | forward on the internal graph, median ms | build / forward | dominant pass |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            dom = max(r["passes_ms"], key=r["passes_ms"].get)
            f.write(f"| {r['workload']} | {r['radius_scale']} | {r['atoms']} | {r['edges_data']} | {r['edges_internal']} | {r['bins']} | {r['device_build_ms_median']} ({r['device_build_ms_min']} .. {r['device_build_ms_max']}) | "
                    f"{r['host_build_graph_ms']} | {r.get('forward_on_internal_graph_ms_median', 'not measured')} | {r.get('build_over_forward', 'not measured')} | {dom} {r['passes_ms'][dom]} ms |\n")
        f.write("\nPasses, ms (each between two synchronises):\n\n")
        for r in rows:
            f.write(f"* {r['workload']}, radius_scale {r['radius_scale']}: " + ", ".join(f"{k} {v}" for k, v in r["passes_ms"].items()) + "\n")
