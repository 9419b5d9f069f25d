"""Micro-benchmark of the density-row kernel (csrc/spectra.hip: hg_density_rows) against the torch path of hamgnn_amd/density.py (chunked gathers + einsum), on
the same device: a synthetic cell of data.synthetic.random_cell (H / Si / Se of the 19-orbital OpenMX head: 5 / 13 / 19 orbitals per atom) with random
eigenvector rows for nk k-points x nb states each and random weights of both signs -- no solver runs.  The dense route (P(k) = C^T diag(f) conj(C) by a library
bmm, then kspace.assemble_k_adjoint) is not timed: the JSON line carries its operation count, 8 M^2 ns flops and M^2 complex elements per k-point.

    python tests/bench_density.py [--atoms 216] [--nk 8] [--nb 256] [--reps 5]

Prints one JSON line: kernel ms (ops.density_rows: host checks + launch), the launch alone, torch ms (median, min, max), ratio, the useful flop
8 sum_members n_i n_j ns and their fraction of the fp32-MFMA peak (157.3 TFLOP/s) in the launch alone, the bytes of C read once per member
and of the rows written, and the largest difference between the two paths."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_F32_MFMA = 157.3e12


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def bench(atoms, nk, nb, reps):
    from hamgnn_amd import _lib, bonds, density, ops
    from hamgnn_amd.data.synthetic import random_cell
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    nao = 19
    head = HamGNNPlusPlusOut("1x0e", "1x0e", nao_max=nao, ham_type="openmx", ham_only=True, calculate_sparsity=False)
    g = random_cell(atoms, (1, 14, 34), seed=0)
    z, ei, sh = g.z.numpy(), g.edge_index.numpy(), g.cell_shift.numpy()
    N, E = len(z), ei.shape[1]
    tab = bonds.bond_tables(head, z, ei, sh, "cuda")
    M = tab.M
    ns = nk * nb
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    C = torch.complex(rnd(ns, M), rnd(ns, M)) / np.sqrt(2 * M)
    f = rnd(ns) / nk
    kvec = torch.rand(nk, 3, device="cuda", generator=gen) - 0.5
    kidx = torch.arange(nk, device="cuda", dtype=torch.int32).repeat_interleave(nb)
    args = (C, kidx, kvec, f, tab.erow, tab.ecol, tab.shift, tab.orank, tab.ooff)
    norb = (tab.orank >= 0).sum(1).cpu().numpy()
    pairs = float((norb[ei[0]] * norb[ei[1]]).sum() + (norb * norb).sum())
    flop = 8.0 * pairs * ns
    k_ms = timed(lambda: ops.density_rows(*args), 2, reps)
    t_ms = timed(lambda: density._density_rows_torch(*args), 1, max(2, reps // 2))
    Pk, Pt = ops.density_rows(*args), density._density_rows_torch(*args)
    Cr = torch.view_as_real(C)                                  # the launch alone, without the wrapper's host checks of the tables (a dozen scalar read-backs)
    l_ms = timed(lambda: _lib.call("hg_density_rows", Cr, ns, M, kidx, kvec, nk, f, tab.erow, tab.ecol, tab.shift, E, N, nao, tab.orank, tab.ooff, 0, Pk[0], Pk[1]), 2, reps)
    diff = max(float((Pk[0] - Pt[0]).abs().max()), float((Pk[1] - Pt[1]).abs().max()))
    return {"atoms": N, "edges": E, "M": M, "nao": nao, "nk": nk, "ns": ns, "kernel_ms": k_ms, "launch_only_ms": l_ms, "torch_ms": t_ms, "torch_over_kernel": t_ms[0] / k_ms[0], "flop": flop,
            "fraction_of_f32_mfma_peak": flop / (l_ms[0] * 1e-3) / PEAK_F32_MFMA, "bytes_C_per_member_pass": 8.0 * float((norb[ei[0]] + norb[ei[1]]).sum() + norb.sum()) * ns,
            "bytes_rows": 4.0 * (N + E) * nao * nao, "dense_route_flop": 8.0 * float(M) * M * ns, "dense_route_complex_per_k": float(M) * M,
            "max_abs_diff_vs_torch": diff, "max_abs": max(float(Pt[0].abs().max()), float(Pt[1].abs().max()))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=216)
    ap.add_argument("--nk", type=int, default=8)
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(bench(a.atoms, a.nk, a.nb, a.reps)), flush=True)
