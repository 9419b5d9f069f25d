"""Micro-benchmark of hg_kan_hidden (csrc/kan.hip) and of what use_kan costs downstream.
  (a) the kernel: 9 and 13 KAN weight generators 64 -> 64 -> 64 (grid size 3) on 822 350 basis rows, one launch, next to hg_radial_hidden_multi on the same rows;
      TF and the fraction of the fp32 MFMA peak for 2 E (448 * 64 + 448 * 64) flop per generator; checked against the fp64 restatement on the tail rows.
  (b) --forward: the sio2_10k backbone forward (set-A irreps, 3 layers) with use_kan against the FullyConnectedNet model, same script, same graph; the time inside
      the edge-kernel launches from HIP events.
Warm-up launches first, then `reps` repetitions of the same call between two events.  HG_LIB_PATH selects the .so.  One JSON line per measurement."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hamgnn_amd import ops, plan as P
from tests import kan_ref as K

PEAK_FP32_TFLOPS = 157.3
ap = argparse.ArgumentParser(); ap.add_argument("--rows", type=int, default=822350); ap.add_argument("--nmlp", default="9,13")
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--forward", action="store_true"); ap.add_argument("--tag", default="")
a = ap.parse_args()
dev = torch.device("cuda")


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps, out


if not a.forward:
    g = torch.Generator().manual_seed(0)
    rbf = torch.randn(a.rows, 64, generator=g).to(dev)
    for n in (int(x) for x in a.nmlp.split(",")):
        refs = [K.KANRef((64, 64, 64, 8), generator=g).scale_(4.0) for _ in range(n)]
        gens = [ops.KanGenerator(P.kan_layers({"g." + k: v for k, v in K.state_dict_np(r).items()}, "g"), dev) for r in refs]
        assert gens[0].packed
        ms, Phi = timed(lambda: ops.kan_hidden_multi(rbf, gens))
        sl = slice(a.rows - 200, a.rows)
        err = max(float((Phi[m][sl].double().cpu() - refs[m].features(rbf[sl].double().cpu())).abs().max()) for m in (0, n - 1))
        flop = 2.0 * a.rows * (448 * 64 + 448 * 64) * n
        fcn = [[(torch.randn(64, 64, generator=g) / 8).to(dev) for _ in range(2)] for _ in range(n)]
        del Phi
        ms_fcn, _ = timed(lambda: ops.radial_hidden_multi(rbf, fcn, 1.679))
        print(json.dumps({"tag": a.tag, "what": "hg_kan_hidden", "rows": a.rows, "nmlp": n, "ms": ms, "TF": flop / ms / 1e9, "frac_of_fp32_mfma_peak": flop / ms / 1e9 / PEAK_FP32_TFLOPS,
                          "out_GB": n * a.rows * 448 * 4 / 1e9, "write_GBs": n * a.rows * 448 * 4 / ms / 1e6, "max_abs_err_vs_fp64_tail": err,
                          "hg_radial_hidden_multi_ms": ms_fcn, "hg_radial_hidden_multi_TF": a.rows * n * 2 * 2 * 64 * 64 / ms_fcn / 1e9}), flush=True)
else:
    import bench
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    graph = bench.make_graph("sio2_10k", 19).to(dev)
    for use_kan in (False, True):
        torch.manual_seed(666)
        m = HamGNNConvE3(dict(bench.make_cfg(bench.IRREPS["A"]), use_kan=use_kan))
        with torch.no_grad():
            ms, rep = timed(lambda: m(graph))
            ops.PROFILE_EVENTS = []
            m(graph)
            torch.cuda.synchronize()
            ev, ops.PROFILE_EVENTS = ops.PROFILE_EVENTS, None
        edge = sum(e0.elapsed_time(e1) for e0, e1, rows, tag in ev if tag in ("message_pack", "embedding"))
        print(json.dumps({"tag": a.tag, "what": "sio2_10k backbone forward", "use_kan": use_kan, "edges": int(graph.edge_index.shape[1]), "ms": ms, "edge_kernel_ms": edge,
                          "edge_launches": sum(tag in ("message_pack", "embedding") for *_, tag in ev), "hidden_rows": int(m.convolutions[0].conv_tp._dp.hidden),
                          "checksum": float(rep["_node_planar"].double().abs().mean())}), flush=True)
        del m, rep
        torch.cuda.empty_cache()
