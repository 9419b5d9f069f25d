"""Micro-benchmark of the k-gradient kernel (csrc/spectra.hip: hg_kgrad_elements) against the torch path of hamgnn_amd/velocity.py (chunked gathers + einsum,
what HG_DOS=torch selects), on the shapes of tests/bench_bonds.py: a 64-atom Si cell with the 19-orbital OpenMX head (13 orbitals per Si atom, M = 832),
random rows and random eigenvector rows for 8 k-points x 832 bands -- no solver runs.  Two pair lists: every state's diagonal pair (np = ns: one row set of
band_velocities) and 16 pairs (a degenerate block or a few interband elements: the edge split alone has to fill the device).  For scale: ops.bond_weights at
the same (ns, E, nao) with every edge in one group (by="species_pair", no on-site groups) -- the same per-edge work, one third of the outputs.

    python tests/bench_velocity.py [--nk 8] [--reps 20]

What is timed: device events around one call of ops.kgrad_elements (wrapper, host checks with their device-to-host copies, scratch allocation, both
launches) after 3 warm-up calls, the median / min / max of `reps` calls, kernel and torch path alternating in the same process; `launch_ms` is the two
launches alone (the typed call into the library on preallocated scratch and output), alternating with the wrapper.  Prints one JSON line per pair list:
kernel ms, launch ms, torch ms, ratio, the issued flop 2 * 2 * np * E * nao^2 (two real GEMMs X Re C and X Im C per edge over the full nao x nao block, the predicated zeros included) and their fraction of
the fp32-MFMA peak (157.3 TFLOP/s), the useful flop 8 sum_e n_i n_j np, and the bytes of C and of the rows that must move at least once."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_F32_MFMA = 157.3e12


def timed_pair(fa, fb, warmup, reps):
    """median / min / max ms of fa and of fb, their calls alternating"""
    for _ in range(warmup):
        fa(), fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for fn, t in ((fa, ts[0]), (fb, ts[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
    return tuple((float(np.median(t)), float(min(t)), float(max(t))) for t in ts)


def bench(nk, reps):
    from hamgnn_amd import _lib, bonds, dos, ops, velocity
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
    rvec = velocity.edge_vectors(g.cell.numpy(), sh).cuda()
    norb = (tab.orank >= 0).sum(1).cpu().numpy()
    pair_products = float((norb[ei[0]] * norb[ei[1]]).sum())
    # the yardstick: hg_bond_weights with all E edges in one group, no on-site member
    groups = tuple(torch.from_numpy(a).cuda() for a in bonds.bond_groups(ei, sh, z, by="species_pair", onsite=False)[:4])
    G = int(groups[0].shape[0]) - 1
    bw_args = (C, kidx, kvec, Xon, Xoff, tab.erow, tab.ecol, tab.shift, tab.orank, tab.ooff, *groups, wk, dos.padded_groups(G))
    out = []
    for name, npair in (("diagonal", ns), ("block", 16)):
        bra = torch.arange(npair, device="cuda", dtype=torch.int32)
        ket = bra.clone() if name == "diagonal" else torch.arange(npair, device="cuda", dtype=torch.int32).flip(0).contiguous()      # 16 states of k-point 0
        args = (C, bra, ket, kidx, kvec, Xoff, tab.erow, tab.ecol, tab.shift, rvec, tab.orank, tab.ooff)
        k_ms, t_ms = timed_pair(lambda: ops.kgrad_elements(*args), lambda: velocity._kgrad_elements_torch(*args), 3, reps)
        part = torch.empty(max(1, _lib.call("hg_scratch_bytes", b"hg_kgrad_elements", npair, E) // 4), device="cuda")
        raw = torch.empty(npair, 3, device="cuda", dtype=torch.complex64)
        launch = lambda: _lib.call("hg_kgrad_elements", torch.view_as_real(C), ns, M, bra, ket, npair, kidx, kvec, nk, Xoff, tab.erow, tab.ecol, tab.shift, rvec, E, N,
                                   nao, tab.orank, tab.ooff, part, torch.view_as_real(raw))
        l_ms = timed_pair(launch, lambda: ops.kgrad_elements(*args), 3, reps)[0]
        b_ms = timed_pair(lambda: ops.bond_weights(*bw_args), lambda: None, 3, reps)[0] if name == "diagonal" else None
        Dk, Dt = ops.kgrad_elements(*args), velocity._kgrad_elements_torch(*args)
        issued = 2.0 * 2.0 * npair * E * nao * nao
        out.append({"pairs": name, "atoms": N, "edges": E, "M": M, "ns": ns, "np": npair, "nao": nao, "kernel_ms": k_ms, "launch_ms": l_ms, "torch_ms": t_ms,
                    "torch_over_kernel": t_ms[0] / k_ms[0], "bond_weights_one_group_ms": b_ms,
                    "kernel_over_bond_weights": None if b_ms is None else k_ms[0] / b_ms[0], "issued_flop": issued,
                    "fraction_of_f32_mfma_peak": issued / (k_ms[0] * 1e-3) / PEAK_F32_MFMA,
                    "fraction_of_f32_mfma_peak_launch_only": issued / (l_ms[0] * 1e-3) / PEAK_F32_MFMA, "useful_flop": 8.0 * pair_products * npair,
                    "bytes_C_and_rows": C.numel() * 8 + Xoff.numel() * 4 + rvec.numel() * 4,
                    "max_abs_diff_vs_torch": float((Dk - Dt).abs().max()), "launch_equals_wrapper": bool(torch.equal(torch.view_as_real(raw), torch.view_as_real(Dk))), "max_abs": float(Dt.abs().max())})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nk", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for line in bench(a.nk, a.reps):
        print(json.dumps(line), flush=True)
