"""Micro-benchmark of the order-generic symmetric-contraction kernels (csrc/sym_contraction.hip), one JSON line per measurement:
  (a) nu = 4: time per launch of hg_sym_contraction_nu and of hg_sym_contraction_nu_backward (element weights and per-node weights) on `--nodes` nodes
      of `--irreps` with `--hidden` channels, the planner's default (reference) path list;
  (b) nu = 3, what HG_CORR_KERNEL=nu exchanges: the generic forward against hg_sym_contraction3 (csrc/sym_contraction.hip), the generic adjoint against the torch
      backward of hamgnn_amd/corr3.py, same tables, same inputs; the largest difference between the two routes is printed with the times.
Warm-up launches first, then `reps` repetitions of the same call between two events.  HG_LIB_PATH selects the .so."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hamgnn_amd import ops, plan as P
from hamgnn_amd.corr3 import sym3_backward

ap = argparse.ArgumentParser(); ap.add_argument("--nodes", type=int, default=4096); ap.add_argument("--irreps", default="4x0e+3x1o+2x2e"); ap.add_argument("--hidden", type=int, default=16)
ap.add_argument("--elements", type=int, default=3); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--tag", default="")
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


hid = P.corr_hidden_irreps(a.irreps, a.hidden)
t0 = time.time()
tab_np = P.sym_contraction_tables(hid, 4)
for nu in (3, 4):
    tab_np.update({f"{k}{nu}": v for k, v in P.sym_contraction_adjoint_tables(tab_np, nu).items()})
plan_s = time.time() - t0
tab = {k: (torch.from_numpy(v).to(dev) if hasattr(v, "dtype") else v) for k, v in tab_np.items()}
Dp, C, N, T = P.PlanarLayout(hid).dim, a.hidden, a.nodes, a.elements
g = torch.Generator().manual_seed(0)
h, go = torch.randn(N, Dp, generator=g).to(dev), torch.randn(N, Dp, generator=g).to(dev)
z = torch.randint(0, T, (N,), generator=g).to(dev)
zn = torch.arange(N, device=dev)
base = dict(tag=a.tag, irreps=a.irreps, hidden=C, nodes=N, elements=T, plan_s=round(plan_s, 2))
for nu in (4, 3):
    K, E = sum(tab_np[f"K{nu}"]), int(tab_np[f"ptr{nu}"][-1])
    W = (torch.randn(T, K, C, generator=g) / K).to(dev)
    Wn = W[z].contiguous()
    out = torch.zeros(N, Dp, device=dev)
    ms_f, _ = timed(lambda: ops.sym_contraction_nu(nu, h, z, C, tab, W, out))
    gh = torch.zeros(N, Dp, device=dev)
    ms_b, _ = timed(lambda: ops.sym_contraction_nu_backward(nu, h, z, C, tab, W, go, gh))
    ms_bn, _ = timed(lambda: ops.sym_contraction_nu_backward(nu, h, zn, C, tab, Wn, go, gh, per_node=True))
    rec = dict(base, what=f"hg_sym_contraction_nu nu={nu}", entries=E, paths=K, forward_ms=ms_f, adjoint_ms=ms_b, adjoint_per_node_ms=ms_bn,
               forward_Gentry_channel_per_s=N * E * C / ms_f / 1e6)
    if nu == 3:
        out3 = torch.zeros(N, Dp, device=dev)
        ms_f3, _ = timed(lambda: ops.sym_contraction3(h, z, C, tab, W, out3))
        ms_b3, (gh3, gW3) = timed(lambda: sym3_backward(tab, h, z, W, C, go))
        o_a, o_b = ops.sym_contraction_nu(3, h, z, C, tab, W, torch.zeros(N, Dp, device=dev)), ops.sym_contraction3(h, z, C, tab, W, torch.zeros(N, Dp, device=dev))
        gh_a = torch.zeros(N, Dp, device=dev)
        gW_a = ops.sym_contraction_nu_backward(3, h, z, C, tab, W, go, gh_a)
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
        rec.update(hg_sym_contraction3_ms=ms_f3, torch_backward_ms=ms_b3, forward_vs_corr3_rel=rel(o_a, o_b), g_h_vs_torch_rel=rel(gh_a, gh3), g_W_vs_torch_rel=rel(gW_a, gW3))
    print(json.dumps(rec), flush=True)
