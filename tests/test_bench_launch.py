"""bench.py as ONE command for N > 1: `python bench.py --gpus N` starts its own ranks under torch.distributed.run.  Without a GPU the ranks
cannot run -- what is checked here is the launcher leg: N ranks are started, each says who it is when it dies, the exit code is non-zero, no JSON line."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(torch.cuda.is_available(), reason="the GPU twin is tests/test_gpu_parity.py::test_bench_script_two_rank_path_on_one_gpu[bare]")
def test_bare_command_launches_its_ranks_and_propagates_their_failure():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "si2", "--irreps", "B"],
                        capture_output=True, text=True, timeout=600, env=env)
    assert cp.returncode != 0
    fails = [l for l in cp.stderr.splitlines() if l.startswith("BENCH_RANK_FAILURE ")]      # (the launcher tears the other rank down as soon as the first one has died)
    assert 1 <= len(fails) <= 2 and all('"world_size": "2"' in f for f in fails), cp.stderr[-1500:]
    assert any(l.startswith("BENCH_LAUNCH_FAILURE ") for l in cp.stderr.splitlines())
    assert not [l for l in cp.stdout.splitlines() if l.startswith("{")]


def test_launcher_and_gpus_flag_must_agree():
    """under a launcher (WORLD_SIZE set) --gpus has to name the world size: a mismatch is refused before any device work"""
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert cp.returncode != 0 and "WORLD_SIZE" in cp.stderr


def test_output_dump_is_bounded_and_the_same_sample_every_time(tmp_path):
    """bench.py --dump-outputs: arrays as float32 (float64 kept), numbers as 0-d float64, None skipped; above the size limit the large arrays are cut to
    the same seeded sample of rows for every array of that length (indices beside them), small ones stay whole, and a second call on the same
    outputs writes the same files"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    outs = {"hamiltonian_real": torch.randn(4000, 36, generator=g), "hamiltonian_imag": torch.randn(4000, 36, generator=g),
            "energies": torch.randn(7, dtype=torch.float64, generator=g), "sparsity_ratio": 0.5, "band_energy": None, "parts": [torch.arange(3)]}
    limit = 200_000
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d), limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert files == ["energies.npy", "hamiltonian_imag.npy", "hamiltonian_imag.rows.npy", "hamiltonian_real.npy", "hamiltonian_real.rows.npy", "parts.0.npy",
                     "sparsity_ratio.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    rows = np.load(tmp_path / "a" / "hamiltonian_real.rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < 4000 and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(rows, np.load(tmp_path / "a" / "hamiltonian_imag.rows.npy"))
    re = np.load(tmp_path / "a" / "hamiltonian_real.npy")
    assert re.dtype == np.float32 and re.shape == (len(rows), 36)
    np.testing.assert_array_equal(re, outs["hamiltonian_real"].numpy()[rows.astype(np.int64)])
    assert np.load(tmp_path / "a" / "energies.npy").dtype == np.float64 and np.load(tmp_path / "a" / "parts.0.npy").dtype == np.float32
    assert float(np.load(tmp_path / "a" / "sparsity_ratio.npy")) == 0.5
