"""The fused node scatter of the single-part edge kernel without a GPU: the mask algebra of csrc/tp_stage.h:is_scan_setup / is_seg_scan restated in numpy
(tests/emu.py:seg_scan_setup / seg_scan) over EVERY cut of a 16-slot tile and every tail length, the invariants of topo.Topology.receiver_major on graphs whose run
ends sit on, before and behind tile ends, and the `-m gpu` checks of tests/test_gpu_forward_scatter.py through the CPU stand-ins (their plumbing and forced dispatch)."""
import numpy as np
import pytest
import torch

from tests import cpu_ops, emu
from tests import gpu_checks as G

U = 2.0 ** -24


@pytest.fixture
def cpu_backend(monkeypatch):
    cpu_ops.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    torch.set_num_threads(min(8, torch.get_num_threads()))


def scan_twin_figures(drop, channels=3, seed=0, setup=emu.seg_scan_setup):
    """all 32 768 cuts of a tile with the last `drop` slots a tail (ids -1 - slot, values = a copy of the last valid slot: the kernel reads a clamped edge there) through
    the twin, against a plain left-to-right float64 sum of every run.  Returns (wrong `last` flags, elements over the bar, worst error in units of u * sum |x_i|)."""
    cuts = np.arange(1 << 15, dtype=np.int64)
    head = np.ones((cuts.size, 16), dtype=bool)
    head[:, 1:] = ((cuts[:, None] >> np.arange(15)[None, :]) & 1).astype(bool)
    valid = np.arange(16) < 16 - drop
    rid = np.cumsum(head, axis=1) - 1 + 17 * cuts[:, None] % 1000            # (ids start anywhere, 0 included: tile 0 begins at run 0)
    rid = np.where(valid[None, :], rid, -1 - np.arange(16)[None, :]).astype(np.int32)
    rng = np.random.default_rng(5 + seed)
    x = (rng.normal(size=(cuts.size, 16, channels)) * np.exp(rng.normal(size=(cuts.size, 16, 1)) * 2.0)).astype(np.float32)
    x[:, ~valid] = x[:, 15 - drop][:, None]
    m, last = setup(rid)
    got = emu.seg_scan(x, m)
    # plain reference: a running float64 sum that restarts at every run head; the run closes where the next slot is a head, a tail slot or the tile's end
    acc, sab = np.zeros((cuts.size, channels)), np.zeros((cuts.size, channels))
    exact, sabs = np.zeros(x.shape), np.zeros(x.shape)
    for s in range(16):
        h = head[:, s, None]
        acc, sab = np.where(h, 0.0, acc) + x[:, s].astype(np.float64), np.where(h, 0.0, sab) + np.abs(x[:, s].astype(np.float64))
        exact[:, s], sabs[:, s] = acc, sab
    closes = np.ones((cuts.size, 16), dtype=bool)
    closes[:, :15] = head[:, 1:] | ~valid[None, 1:]
    closes &= valid[None, :]
    wrong_last = int(((last & (rid >= 0)) != closes).sum())
    diff = np.abs(got.astype(np.float64) - exact)[closes]
    over = int((~(diff <= 4.5 * U * sabs[closes])).sum())
    return wrong_last, over, float((diff / (U * sabs[closes])).max())


@pytest.mark.parametrize("drop", range(16))
def test_scan_twin_every_cut_and_tail_vs_per_run_float64_sum(drop):
    """the kernel's four masks (head flags shifted by 1, 1, 2, 4 with the `el < d` overrides), its four fused steps in float32 and its `last` flag on all 2^15 cuts x
    16 tail lengths (0 = a full tile).  Bar per element, derived as in gpu_checks.check_fused_scatter_all_run_shapes: 4.5 * 2^-24 * sum |x_i| over the run"""
    wrong_last, over, worst = scan_twin_figures(drop)
    print({"drop": drop, "worst_in_units_of_u_sum_abs": worst})
    assert wrong_last == 0 and over == 0 and worst <= 4.5, (wrong_last, over, worst)


def test_scan_twin_masks_equal_the_definition():
    """m[k][slot] = 1 exactly when no run starts in (slot - d, slot] and slot >= d, d = 1, 2, 4, 8 -- the definition the kernel's comment gives, from the run lengths"""
    cuts = np.arange(1 << 15, dtype=np.int64)
    head = np.ones((cuts.size, 16), dtype=bool)
    head[:, 1:] = ((cuts[:, None] >> np.arange(15)[None, :]) & 1).astype(bool)
    m, _ = emu.seg_scan_setup(np.cumsum(head, axis=1).astype(np.int32))
    start = np.maximum.accumulate(np.where(head, np.arange(16)[None, :], 0), axis=1)       # first slot of the run a slot belongs to
    for k, d in enumerate((1, 2, 4, 8)):
        assert np.array_equal(m[k] == 1.0, np.arange(16)[None, :] - d >= start), d


def _topology(N, src, dst):
    from hamgnn_amd.topo import Topology
    return Topology({"edge_index": torch.from_numpy(np.stack([src, dst])), "z": torch.zeros(N, dtype=torch.long)})


@pytest.mark.parametrize("graph", G.SCATTER_GRAPHS + ("empty",))
def test_receiver_major_invariants(graph):
    if graph == "empty":
        N, src, dst = 3, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    else:
        N, src, dst = G.scatter_graph(graph)
    eperm, run_id, R, prow, ident = _topology(N, src, dst).receiver_major()
    eperm, run_id, prow = eperm.numpy(), run_id.numpy().astype(np.int64), prow.numpy()
    E = dst.size
    assert sorted(eperm.tolist()) == list(range(E)) and prow.shape == (N + 1,) and prow[0] == 0 and prow[-1] == R and ident.tolist() == list(range(R))
    recv = dst[eperm]
    assert (np.diff(recv) >= 0).all()                                                   # receiver-major
    if E == 0:
        assert R == 0 and (prow == 0).all()
        return
    head = np.ones(E, dtype=bool)
    head[1:] = np.diff(run_id) != 0
    assert head[::16].all()                                                             # a head at every slot that is a multiple of 16
    assert run_id[0] == 0 and set(np.diff(run_id).tolist()) <= {0, 1} and run_id[-1] == R - 1      # non-decreasing and dense
    assert np.array_equal(head[1:], (recv[1:] != recv[:-1]) | (np.arange(1, E) % 16 == 0))         # a run = equal receivers inside one tile, and nothing else
    for n in range(N):                                                                  # the rows of each node are contiguous under prow; none for a node without edges
        rows = np.unique(run_id[recv == n])
        assert rows.tolist() == list(range(prow[n], prow[n + 1])), (n, rows, prow)
    s = G.tile_statistics(dst, N)
    assert s["tail_edges"] == E % 16 and s["straddling_receivers"] == int((np.diff(prow) > 1).sum()) and R >= -(-E // 16), (s, R)


def test_receiver_major_hub_graph_is_what_it_claims():
    N, src, dst = G.scatter_graph("hub")
    deg = np.bincount(dst, minlength=N)
    assert N == 23 and dst.size == 60 and deg[8] == 40 and deg[0] == 0 and deg[-1] == 0 and sorted(deg.tolist()) == [0, 0] + [1] * 20 + [40]
    eperm, run_id, R, prow, _ = _topology(N, src, dst).receiver_major()
    assert prow[9] - prow[8] == 3 and R == 23                  # the hub's 40 edges: slots 7 .. 46 = three runs in three tiles; 20 single-edge runs
    g = G.hub_graph()
    inv, ei = g["inv_edge_idx"], g["edge_index"]
    assert torch.equal(inv[inv], torch.arange(60)) and torch.equal(ei[:, inv], ei.flip(0)) and torch.equal(g["cell_shift"][inv], -g["cell_shift"])


@pytest.mark.parametrize("graph", G.SCATTER_GRAPHS)
def test_two_stage_sum_through_the_stand_ins_vs_oracle(cpu_backend, graph):
    """the host glue of the fused scatter (run rows, then ops.segment_sum over prow) on the stand-ins == index_add of the oracle's message rows onto the receivers"""
    r = G.check_message_pack_nodes_forward(device="cpu", graph=graph, seed=0, parts=1, reduce=True)
    assert r["kernel"] == "is" and r["parts_used"] == 1 and r["reduce_ran"] and r["rel_err"] < G.TOL, r


def test_forward_scatter_checks_run_on_the_stand_ins(cpu_backend):
    """the checks behind tests/test_gpu_forward_scatter.py through the host code on the CPU stand-ins: the launches they mean to test ARE the single-part ones with and
    without the fused scatter, the 8-part one is the 8-part one, the graph of section 1 is the intended one (asserted inside the check), and the forced parts and the
    spies are undone.  (The stand-ins build results by value and sum a run in float64: the bars hold trivially; the scan itself is pinned by the twin above.)"""
    import os
    from hamgnn_amd import ops
    blk = G.fused_scatter_block("cpu")
    r = G.check_fused_scatter_all_run_shapes("cpu", cuts=200, block=blk)
    assert r["tiles"] == 200 and r["E"] == 3200 and (r["runs_per_tile_min"], r["runs_per_tile_max"]) == (1, 16) and r["sentinel_allocations"] == 0, r
    G.assert_run_shapes(r)
    r = G.check_fused_scatter_all_run_shapes("cpu", cuts=20, drop=5, last_cut=0x7fff, block=blk)
    assert r["tail_edges"] == 11 and r["E"] == 315 and r["N"] - r["R"] == 5, r
    G.assert_run_shapes(r)
    r = G.check_message_pack_nodes_forward(device="cpu", graph="one17", seed=1, parts=1)
    assert r["kernel"] == "is" and r["parts_used"] == 1 and not r["reduce_ran"] and r["rel_err"] < G.TOL, r
    r = G.check_message_pack_nodes_forward(device="cpu", graph="hub", seed=0, parts=8)
    assert r["kernel"] == "is" and r["parts_used"] == 8 and r["part_rows"] == 4 and not r["reduce_ran"] and r["rel_err"] < G.TOL, r
    assert G.check_message_pack_nodes_forward(device="cpu", graph="hub", seed=0)["parts_used"] not in (1, 8)        # (unforced, 60 edges are split by output segment)
    r = G.oracle_vs_hip_random(device="cpu", graph="hub", parts=1, seed=2, num_layers=1)
    L = r["launches"]
    assert r["E"] == 60 and L and all(l["kernel"] == "is" and l["parts"] == 1 for l in L) and sum(l["reduce"] for l in L) == 1, r
    assert r["node_rel_err"] < G.TOL and r["edge_rel_err"] < G.TOL and r["H_rel_err"] < G.TOL, r
    assert ops.tp_fused.__name__ != "spy_fused" and "HG_IS_PARTS" not in os.environ and torch.empty.__name__ == "empty"
