"""Micro-benchmark of the bond-weight kernel (csrc/spectra.hip: hg_bond_weights) against the torch path of hamgnn_amd/bonds.py (chunked gathers + einsum), on
a 64-atom Si cell with the 19-orbital OpenMX head (13 orbitals per Si atom, M = 832): random rows and random eigenvector rows for 8 k-points x 832 bands --
no solver runs.  Grouped by="edge" (many groups of two members) and by="species_pair" (one group of every edge): the two extremes of group size.  For scale:
ops.mulliken_weights plus the dense bmm S(k) C for the same states, what a projection on atoms costs.

    python tests/bench_bonds.py [--nk 8] [--reps 5]

Prints one JSON line per grouping: kernel ms, torch ms, ratio, the useful flop 8 sum_e n_i n_j ns and their fraction of the fp32-MFMA peak (157.3 TFLOP/s),
the bytes of C and of the rows that must move at least once."""
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


def bench(nk, reps):
    from hamgnn_amd import bonds, dos, ops
    from hamgnn_amd.data.synthetic import si_diamond
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    nao = 19
    head = HamGNNPlusPlusOut("1x0e", "1x0e", nao_max=nao, ham_type="openmx", ham_only=True, calculate_sparsity=False)
    g = si_diamond(2, 2, 2)
    z, ei, sh = g.z.numpy(), g.edge_index.numpy(), g.cell_shift.numpy()
    N, E = len(z), ei.shape[1]
    tab = bonds.bond_tables(head, z, ei, sh, "cuda")
    M = tab.M
    ns = nk * M
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    C = torch.complex(rnd(ns, M), rnd(ns, M)) / np.sqrt(2 * M)
    Xon, Xoff = rnd(N, nao * nao), rnd(E, nao * nao)
    kvec = torch.rand(nk, 3, device="cuda", generator=gen) - 0.5
    kidx = torch.arange(nk, device="cuda", dtype=torch.int32).repeat_interleave(M)
    wk = torch.full((ns,), 1.0 / nk, device="cuda")
    norb = (tab.orank >= 0).sum(1).cpu().numpy()
    flop = 8.0 * float((norb[ei[0]] * norb[ei[1]]).sum() + (norb * norb).sum()) * ns
    moved = C.numel() * 8 + (Xon.numel() + Xoff.numel()) * 4
    # for scale: the Mulliken projection on atoms of the same states, S(k) C by one bmm + the weight kernel
    Sk = torch.complex(rnd(nk, M, M), rnd(nk, M, M))
    perm, gptr, labels = dos.group_map(head, z, "atom")
    perm_d, gptr_d = torch.from_numpy(perm).cuda(), torch.from_numpy(gptr).cuda()
    GpA = dos.padded_groups(len(labels))

    def mulliken():
        SC = torch.bmm(Sk, C.reshape(nk, M, M).transpose(1, 2)).transpose(1, 2).reshape(ns, M).contiguous()
        return ops.mulliken_weights(C, SC, perm_d, gptr_d, wk, GpA)
    m_ms = timed(mulliken, 2, reps)
    out = []
    for by in ("edge", "species_pair"):
        groups = tuple(torch.from_numpy(a).cuda() for a in bonds.bond_groups(ei, sh, z, by=by, onsite=True)[:4])
        G = int(groups[0].shape[0]) - 1
        Gp = dos.padded_groups(G)
        args = (C, kidx, kvec, Xon, Xoff, tab.erow, tab.ecol, tab.shift, tab.orank, tab.ooff, *groups, wk, Gp)
        k_ms = timed(lambda: ops.bond_weights(*args), 2, reps)
        t_ms = timed(lambda: bonds._bond_weights_torch(*args), 1, max(2, reps // 2))
        Wk, Wt = ops.bond_weights(*args), bonds._bond_weights_torch(*args)
        out.append({"by": by, "atoms": N, "edges": E, "M": M, "ns": ns, "G": G, "Gp": Gp, "kernel_ms": k_ms, "torch_ms": t_ms,
                    "torch_over_kernel": t_ms[0] / k_ms[0], "mulliken_plus_bmm_ms": m_ms, "flop": flop,
                    "fraction_of_f32_mfma_peak": flop / (k_ms[0] * 1e-3) / PEAK_F32_MFMA, "bytes_C_and_rows": moved,
                    "max_abs_diff_vs_torch": float((Wk - Wt).abs().max()), "max_abs": float(Wt.abs().max())})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nk", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for line in bench(a.nk, a.reps):
        print(json.dumps(line), flush=True)
