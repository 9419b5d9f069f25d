"""Micro-benchmark of the DOS broadening (csrc/spectra.hip: hg_dos_broaden) against the torch path it replaces (dos._broaden_torch: exp of an [energies, states]
matrix in chunks + matmul), on synthetic sorted states of the size of a real call -- Si-64 and Si-512 with 13 orbitals per atom (M = 832 / 6656), projection "atom"
(Gp = 80 / 528 columns), 2000 energies, the states of 64 k-points in one launch.

    python tests/bench_dos.py [--sizes 64 512] [--nk 64] [--reps 5]

Prints one JSON line per size: kernel ms, torch ms, ratio, in-window FMAs, fraction of the fp32-MFMA peak (157.3 TFLOP/s)."""
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


def bench_broaden(n_atoms, nk, ne, sigma, reps):
    from hamgnn_amd import dos, ops
    from tests import dos_checks as DC
    M = 13 * n_atoms
    Gp = dos.padded_groups(n_atoms)
    ns = nk * M
    gen = torch.Generator(device="cuda").manual_seed(n_atoms)
    e_d = torch.sort(6.0 * torch.randn(ns, device="cuda", generator=gen)).values.contiguous()       # a 36 eV wide valence + conduction manifold
    W_d = torch.rand(ns, Gp, device="cuda", generator=gen) / Gp
    eps = e_d.cpu().numpy()
    E0, E1 = float(eps[0]) - 8 * sigma, float(eps[-1]) + 8 * sigma
    dE = (E1 - E0) / (ne - 1)
    fma = sum(b - a for a, b in DC.windows(eps, E0, dE, ne, sigma)) * 16 * Gp
    D = torch.empty(ne, Gp, device="cuda")
    k_ms = timed(lambda: ops.dos_broaden(e_d, W_d, E0, dE, ne, sigma, D=D), 3, reps)
    t_ms = timed(lambda: dos._broaden_torch(e_d, W_d, E0, dE, ne, sigma), 2, max(3, reps // 2))
    Dt = dos._broaden_torch(e_d, W_d, E0, dE, ne, sigma)
    return {"atoms": n_atoms, "ns": ns, "Gp": Gp, "ne": ne, "sigma": sigma, "dE": dE, "kernel_ms": k_ms, "torch_ms": t_ms, "torch_over_kernel": t_ms[0] / k_ms[0],
            "in_window_fma": fma, "dense_fma": ne * ns * Gp, "fraction_of_f32_mfma_peak": 2.0 * fma / (k_ms[0] * 1e-3) / PEAK_F32_MFMA,
            "max_abs_diff_vs_torch": float((D - Dt).abs().max()), "max_abs": float(Dt.abs().max())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--nk", type=int, default=64)
    ap.add_argument("--ne", type=int, default=2000)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for n in a.sizes:
        print(json.dumps(bench_broaden(n, a.nk, a.ne, a.sigma, a.reps)), flush=True)
