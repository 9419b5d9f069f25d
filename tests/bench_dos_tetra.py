"""Micro-benchmark of the linear tetrahedron method (csrc/spectra.hip: hg_dos_tetra) against the torch path of the same module (dos._tetra_torch: corner weights
of every (energy, tetrahedron, band) in fp64 + index_add_ + matmul, in chunks of energies) and, for scale, against the Gaussian broadening hg_dos_broaden at
sigma = 0.1 eV on the same states.  Synthetic bands of the size of a real call -- Si-64 and Si-512 with 13 orbitals per atom (M = 832 / 6656 bands), projection
"atom" (Gp = 80 / 528 columns), the 64 k-points of an unfolded 4 x 4 x 4 grid (384 tetrahedra), 2000 energies over the whole spectrum.

    python tests/bench_dos_tetra.py [--sizes 64 512] [--reps 5] [--torch-reps 5]

CUDA events, 3 warm-up calls, the median of --reps with (min, max).  Prints one JSON line per size."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.bench_dos import timed  # noqa: E402


def synthetic_bands(n_atoms, grid, gen):
    """eps [nk, M] fp32 ascending in b: levels of a 36 eV wide manifold, each dispersing by up to 0.3 eV over the grid with its own wave vector and phase"""
    from hamgnn_amd import dos
    M = 13 * n_atoms
    k = torch.from_numpy(dos.monkhorst_pack(grid, time_reversal=False)[0]).to("cuda")
    level = 6.0 * torch.randn(M, device="cuda", generator=gen, dtype=torch.float64)
    n = torch.randint(1, 3, (M, 3), device="cuda", generator=gen).double()
    phase = 2.0 * np.pi * torch.rand(M, device="cuda", generator=gen, dtype=torch.float64)
    eps = level[None, :] + 0.3 * torch.cos(2.0 * np.pi * (k @ n.T) + phase[None, :])
    return torch.sort(eps, dim=1).values.float().contiguous()


def bench_tetra(n_atoms, ne, sigma, reps, torch_reps):
    from hamgnn_amd import dos, ops
    grid = (4, 4, 4)
    gen = torch.Generator(device="cuda").manual_seed(n_atoms)
    eps = synthetic_bands(n_atoms, grid, gen)
    nk, M = eps.shape
    Gp = dos.padded_groups(n_atoms)
    W = torch.rand(nk, M, Gp, device="cuda", generator=gen) / Gp
    tet = dos.tetrahedra(grid, np.eye(3), time_reversal=False)
    lo, hi = float(eps.min()), float(eps.max())
    dE = (hi - lo + 1.0) / (ne - 1)
    E0 = lo - 0.5
    out = {"atoms": n_atoms, "nk": nk, "nb": M, "nt": int(tet.shape[0]), "Gp": Gp, "ne": ne, "dE": dE}
    D = torch.empty(ne, Gp, device="cuda")
    saved = os.environ.pop("HG_DOS", None)
    for mode, name in ((0, "dos"), (1, "states")):
        fn = dos.tetra_states if mode else dos.tetra_dos
        out[f"kernel_{name}_ms"] = timed(lambda: fn(eps, W, tet, E0, dE, ne, D=D), 3, reps)
        Dk = D.clone()
        os.environ["HG_DOS"] = "torch"
        out[f"torch_{name}_ms"] = timed(lambda: fn(eps, W, tet, E0, dE, ne), 3, torch_reps)
        Dt = fn(eps, W, tet, E0, dE, ne)
        del os.environ["HG_DOS"]
        out[f"torch_over_kernel_{name}"] = out[f"torch_{name}_ms"][0] / out[f"kernel_{name}_ms"][0]
        out[f"max_abs_diff_vs_torch_{name}"], out[f"max_abs_{name}"] = float((Dk - Dt).abs().max()), float(Dt.abs().max())
    if saved is not None:
        os.environ["HG_DOS"] = saved
    order = torch.sort(eps.reshape(-1)).indices
    e_s, W_s = eps.reshape(-1)[order].contiguous(), (W.reshape(nk * M, Gp)[order] / nk).contiguous()
    out["broaden_sigma"] = sigma
    out["broaden_ms"] = timed(lambda: ops.dos_broaden(e_s, W_s, E0, dE, ne, sigma, D=D), 3, reps)
    out["states_top_minus_sum_rule"] = float((Dk[-1] - W.double().sum((0, 1)).float() / nk).abs().max())      # (Dk: mode 1; the last energy is above every band)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--ne", type=int, default=2000)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=5)
    a = ap.parse_args()
    for n in a.sizes:
        print(json.dumps(bench_tetra(n, a.ne, a.sigma, a.reps, a.torch_reps)), flush=True)
