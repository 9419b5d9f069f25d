"""Micro-benchmark of the k-space adjoint (csrc/kspace.hip: hg_hk_assemble_adjoint) inside kspace.band_energy_backward: one synthetic crystal (default 64 atoms,
nao 19, 16 k-points), once with the kernel and once with HG_HK_ADJOINT=torch (the gathers + complex multiply-reduce the kernel replaces), same process, warm,
median of `reps` wall-clock times after torch.cuda.synchronize(), and the peak allocated device memory of each path.  Also times the adjoint call alone (the
eigen-chain under autograd is common to both paths).  One JSON line; --md prints the table of profiles/kspace_adjoint.md."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hamgnn_amd import kspace
from hamgnn_amd.data import synthetic as S
from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut

ap = argparse.ArgumentParser(); ap.add_argument("--atoms", type=int, default=64); ap.add_argument("--nao", type=int, default=19); ap.add_argument("--nk", type=int, default=16)
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--md", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")
nao = a.nao
head = HamGNNPlusPlusOut("4x0e", "4x0e", nao_max=nao, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=False, soc_switch=False,
                         calculate_band_energy=True, num_k=a.nk, k_path=None, calculate_sparsity=False)
head.compile(dev)
g = S.add_random_targets(S.random_cell(a.atoms, [14, 8, 6, 1], seed=0, density=0.004), nao, seed=0)      # Hermitian-consistent random blocks
g["Son"] = torch.eye(nao).reshape(1, -1).repeat(g.num_nodes, 1)                                            # S(k) = 1: positive definite
gen = torch.Generator().manual_seed(0)
g["k_vecs"] = 0.05 * torch.randn(1, a.nk, 3, generator=gen)
g = g.to(dev)
Hon, Hoff = g["Hon"].contiguous(), g["Hoff"].contiguous()
n, e = g.num_nodes, g.num_edges
tab = kspace.CrystalTables.from_graph(g, 0, n, 0, e, head._orank.to(dev)[g.z])      # (the adjoint alone reuses it, as the backward does inside one call)
M = tab.M
cot = torch.randn(M, a.nk, generator=gen).to(dev)
Gk = torch.complex(torch.randn(a.nk, M, M, generator=gen), torch.randn(a.nk, M, M, generator=gen)).to(dev)


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


res = {"atoms": n, "edges": e, "nao": nao, "nk": a.nk, "M": M, "reps": a.reps}
outs = {}
for path in ("kernel", "torch"):
    os.environ.pop("HG_HK_ADJOINT", None)
    if path == "torch":
        os.environ["HG_HK_ADJOINT"] = "torch"
    ms, mib, outs[path] = timed(lambda: kspace.band_energy_backward(head, Hon, Hoff, g, cot))
    ms_a, mib_a, _ = timed(lambda: kspace.assemble_k_adjoint(Gk, tab, g["k_vecs"][0]))
    res.update({f"{path}_backward_ms": ms, f"{path}_backward_peak_MiB": mib, f"{path}_adjoint_ms": ms_a, f"{path}_adjoint_peak_MiB": mib_a})
os.environ.pop("HG_HK_ADJOINT", None)
res["paths_max_rel_diff"] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(outs["kernel"], outs["torch"]))
res["kernel_not_slower"] = bool(res["kernel_backward_ms"] <= res["torch_backward_ms"])
print(json.dumps(res), flush=True)
if a.md:
    print("| path | band_energy_backward ms (median) | peak MiB | adjoint alone ms | adjoint peak MiB |\n|---|---|---|---|---|")
    for path in ("kernel", "torch"):
        print(f"| {path} | {res[path + '_backward_ms']:.2f} | {res[path + '_backward_peak_MiB']:.1f} | {res[path + '_adjoint_ms']:.3f} | {res[path + '_adjoint_peak_MiB']:.1f} |")
