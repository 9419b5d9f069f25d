"""The k-space step and the `losses` list on an edge-sharded crystal, on the CPU: world-size 2 / 3 over gloo, the product's host code (shard_graph,
the summed H(k) / S(k), k-points dealt to the ranks, the sharded loss helper, training_step) on the CPU stand-ins of the kernels (tests/cpu_ops.py).
The checks themselves are in tests/sharded_losses_checks.py; the same functions run on the HIP kernels in tests/test_sharded_losses_gpu.py."""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _worker(rank, world, port, tmp, fn, kwargs):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from tests import cpu_ops
    from tests import sharded_losses_checks as C

    class _MP:
        @staticmethod
        def setattr(o, n, v):
            setattr(o, n, v)
    cpu_ops.install(_MP)
    if fn == "check_unsharded_takes_the_old_path":
        r = C.check_unsharded_takes_the_old_path("cpu")
    else:
        r = getattr(C, fn)(rank, world, "cpu", **kwargs)
    if rank == 0:
        with open(tmp, "w") as f:
            json.dump(r, f)
    dist.barrier()
    dist.destroy_process_group()


def _run(tmp_path, world, fn, **kwargs):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    tmp = str(tmp_path / "result.json")
    mp.spawn(_worker, args=(world, port, tmp, fn, kwargs), nprocs=world, join=True)
    r = json.loads(open(tmp).read())
    print(r)
    return r


# ---- 1. forward bands
@pytest.mark.parametrize("soc", [False, True], ids=["nonsoc", "soc_so3"])
@pytest.mark.parametrize("world,nk", [(2, 5), (3, 2)], ids=["w2_nk5", "w3_nk2"])
def test_sharded_forward_bands(tmp_path, world, nk, soc):
    """uneven k-blocks (2 + 3), and a rank that owns no k-point (nk = 2 on three ranks): the bands of the WHOLE crystal on every rank.  Bar: 1e-4 of
    the spectrum's scale, the bar of the band tests against their references"""
    from tests import sharded_losses_checks as C
    r = _run(tmp_path, world, "check_forward_bands", soc=soc, nk=nk, k_path=C.KPATH if nk == 5 else C.KPATH2, n_atoms=3 if world == 2 else 6)
    assert r["bands_shape"][1] == nk and r["wavefunction_numel_ok"] and len(r["edges_per_rank"]) == world and min(r["edges_per_rank"]) > 0, r
    assert r["across_ranks_max_diff"] == 0.0 and r["k_vecs_err"] == 0.0, r
    assert r["band_energy_err"] < 1e-4 and r["target_band_energy_err"] < 1e-4, r
    if not soc:
        assert r["band_gap_err"] < 1e-4, r


def test_sharded_forward_bands_random_k_points(tmp_path):
    """k_path=None: the ranks' numpy generators are seeded differently on purpose; the k-vectors are rank 0's on every rank"""
    r = _run(tmp_path, 2, "check_forward_bands", soc=False, nk=5, k_path=None)
    assert r["across_ranks_max_diff"] == 0.0 and r["k_vecs_err"] == 0.0, r
    assert r["band_energy_err"] < 1e-4 and r["target_band_energy_err"] < 1e-4 and r["band_gap_err"] < 1e-4, r


# ---- 2. `losses` step vs the single-process step on the whole crystal (the bars of test_parallel_gloo.py's sharded training tests)
@pytest.mark.parametrize("kind", ["overlap", "soc_split", "cosine_similarity", "euclidean_loss", "sum_zero"])
def test_sharded_losses_step_matches_single_process(tmp_path, kind):
    r = _run(tmp_path, 2, "check_losses_vs_single", kind=kind)
    assert r["loss_err"] < 1e-6 and r["grad_err"] < 2e-5 and r["n"] > 100, r
    assert r["loss_across_ranks"] == 0.0, r


def test_sharded_losses_two_steps(tmp_path):
    """opt.step() between two sharded `losses` steps: the weights are repacked on the shards, the loss moves"""
    r = _run(tmp_path, 2, "check_two_sharded_steps")
    assert r["finite"] and r["same_on_all_ranks"], r
    assert abs(r["first"] - r["second"]) > 1e-4 * abs(r["first"]), r          # a move far above the fp32 rounding of the loss (1e-7)


# ---- 3. k-space losses vs autograd through the fp64 oracle (the bars of tests/test_cpu_end_to_end.py's band-energy tests)
@pytest.mark.parametrize("kind,zps", [("bands", False), ("bands", True), ("bands_gap", False), ("soc_bands", False)])
def test_sharded_kspace_losses_vs_oracle(tmp_path, kind, zps):
    r = _run(tmp_path, 2, "check_kspace_losses_vs_oracle", kind=kind, zps=zps)
    if kind == "bands_gap":
        assert r["gap_isolated"], r                            # condition on the inputs, on the fp64 reference alone
    assert r["loss_rel_err"] < 1e-4 and r["max_rel_err"] < 5e-4, r
    assert r["loss_across_ranks"] == 0.0 and sum(r["k_points_solved_in_backward"]) == 5, r       # one eigen-chain per k-point per step


# ---- 4. refusals; the unsharded path
def test_sharded_refusals(tmp_path):
    for got in _run(tmp_path, 2, "check_refusals"):
        assert got["export"].startswith("NotImplementedError") and "sharded" in got["export"], got
        assert got["wavefunction"].startswith("ValueError") and "not built" in got["wavefunction"], got
        assert got["peak"].startswith("ValueError") and "not built" in got["peak"], got


def test_unsharded_graph_under_a_process_group_issues_no_collective(tmp_path):
    r = _run(tmp_path, 2, "check_unsharded_takes_the_old_path")
    assert r["bands_shape"][1] == 5 and r["same_as_forward"] == 0.0, r
