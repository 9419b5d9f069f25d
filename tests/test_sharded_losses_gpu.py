"""The k-space step and the `losses` list on an edge-sharded crystal on the HIP kernels: two ranks over gloo sharing cuda:0 (the launch pattern of
test_gpu_parity.py::test_two_rank_training_paths_on_one_gpu), one child invocation per mode of tests/dist_gpu_losses_check.py -- never more than two GPU
processes at a time.  The return code AND the printed figures count."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def _run(mode):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cp = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", str(port), os.path.join(root, "tests", "dist_gpu_losses_check.py")], capture_output=True, text=True,
                        timeout=600, env=dict(os.environ, HG_DIST_MODE=mode))
    tail = cp.stdout[-2000:] + cp.stderr[-2000:]
    assert cp.returncode == 0, tail
    lines = [l for l in cp.stdout.splitlines() if l.startswith("DIST_LOSSES ")]
    assert lines, tail
    r = json.loads(lines[-1][len("DIST_LOSSES "):])
    print(r)
    assert r["mode"] == mode and r["world"] == 2, r
    return r["results"]


@pytest.mark.parametrize("mode", ["bands_nonsoc", "bands_soc"])
def test_sharded_forward_bands_on_one_gpu(mode):
    """the bands of the whole crystal on both ranks (k-blocks 2 + 3): identical across the ranks, == the single-process forward within 1e-4 of the
    spectrum's scale (the bar of the band tests against their references)"""
    res = _run(mode)
    assert set(res) == ({"k_path", "random_k"} if mode == "bands_nonsoc" else {"k_path"})
    for name, r in res.items():
        assert min(r["edges_per_rank"]) > 0 and r["bands_shape"][1] == 5 and r["wavefunction_numel_ok"], (name, r)
        assert r["across_ranks_max_diff"] == 0.0 and r["k_vecs_err"] == 0.0, (name, r)
        assert r["band_energy_err"] < 1e-4 and r["target_band_energy_err"] < 1e-4, (name, r)
        if mode == "bands_nonsoc":
            assert r["band_gap_err"] < 1e-4, (name, r)


def test_sharded_losses_overlap_and_rowwise_metrics_on_one_gpu():
    """`losses` lists without a k-space term == the single-process step on the whole crystal: the bars of test_two_rank_training_paths_on_one_gpu"""
    res = _run("losses_overlap_rowwise")
    kinds = ("overlap", "soc_split", "cosine_similarity", "euclidean_loss", "sum_zero")
    assert set(res) == set(kinds) | {"two_steps"}
    for kind in kinds:
        r = res[kind]
        assert r["loss_err"] < 1e-5 and r["grad_err"] < 5e-5 and r["n"] > 100, (kind, r)
    t = res["two_steps"]
    assert t["finite"] and t["same_on_all_ranks"], t
    assert abs(t["first"] - t["second"]) > 1e-4 * abs(t["first"]), t          # a move far above the fp32 rounding of the loss (1e-7)


def test_sharded_band_energy_and_gap_losses_on_one_gpu():
    """k-space `losses` lists vs torch.autograd through the fp64 oracle: the bars of test_train_targets_gpu.py's band-gap test.  The sharded-vs-single-
    process differences (`vs_single_*`) are printed for the record (profiles/sharded_kspace.md), not asserted."""
    res = _run("losses_band_energy_gap")
    assert set(res) == {"bands_zps", "bands_gap", "soc_bands"}
    assert res["bands_gap"]["gap_isolated"], res["bands_gap"]                     # condition on the inputs, on the fp64 reference alone
    for name, r in res.items():
        assert r["loss_rel_err"] < 1e-4 and r["max_rel_err"] < 2e-3 and r["n"] > 100, (name, r)
        assert sum(r["k_points_solved_in_backward"]) == 5, (name, r)               # one eigen-chain per k-point per step
