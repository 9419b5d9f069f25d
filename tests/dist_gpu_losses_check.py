"""The k-space step and the `losses` list on an edge-sharded crystal ON THE HIP KERNELS, runnable on a ONE-GPU box (both ranks share cuda:0 and talk
over gloo; RCCL refuses two ranks on one device):
    HG_DIST_MODE=bands_nonsoc | bands_soc | losses_overlap_rowwise | losses_band_energy_gap
        python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 ... tests/dist_gpu_losses_check.py
  bands_nonsoc / bands_soc    the head's forward with calculate_band_energy on the shards (k-path and, non-SOC, random k-points) == the whole crystal's
  losses_overlap_rowwise      training_step(shard, losses=...) == the single-process step: hamiltonian + overlap, hamiltonian_real + hamiltonian_imag with
                              the sparsity ratio, one list per row-wise metric; two steps with an optimiser step between them
  losses_band_energy_gap      hamiltonian + band_energy (+ band_gap; SOC: real + imag + band_energy) vs torch.autograd through the fp64 oracle
The checks are those of tests/sharded_losses_checks.py (shared with the CPU run over the stand-ins); rank 0 prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
dist.init_process_group("gloo", rank=rank, world_size=world)
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
from tests import sharded_losses_checks as C

mode = os.environ.get("HG_DIST_MODE", "bands_nonsoc")
res = {}
if mode == "bands_nonsoc":
    res["k_path"] = C.check_forward_bands(rank, world, dev, soc=False, nk=C.NK, k_path=C.KPATH)
    res["random_k"] = C.check_forward_bands(rank, world, dev, soc=False, nk=C.NK, k_path=None)
elif mode == "bands_soc":
    res["k_path"] = C.check_forward_bands(rank, world, dev, soc=True, nk=C.NK, k_path=C.KPATH)
elif mode == "losses_overlap_rowwise":
    for kind in ("overlap", "soc_split", "cosine_similarity", "euclidean_loss", "sum_zero"):
        res[kind] = C.check_losses_vs_single(rank, world, dev, kind)
    res["two_steps"] = C.check_two_sharded_steps(rank, world, dev)
elif mode == "losses_band_energy_gap":
    big = dict(num_layers=2, corr=True, seed=C.GAP_SEED_LARGE)
    res["bands_zps"] = C.check_kspace_losses_vs_oracle(rank, world, dev, "bands", zps=True, **big)
    res["bands_gap"] = C.check_kspace_losses_vs_oracle(rank, world, dev, "bands_gap", zps=False, **big)
    res["soc_bands"] = C.check_kspace_losses_vs_oracle(rank, world, dev, "soc_bands", zps=False, **big)
else:
    raise SystemExit(f"unknown HG_DIST_MODE {mode!r}")
torch.cuda.synchronize()
if rank == 0:
    print("DIST_LOSSES", json.dumps({"mode": mode, "world": world, "results": res}))
dist.barrier()
dist.destroy_process_group()
