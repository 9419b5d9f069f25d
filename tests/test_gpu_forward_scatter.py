"""-m gpu: the node scatter fused into the epilogue of the single-part edge kernel (`tp_is_kernel<false, false>`, csrc/tp_stage.h:is_scan_setup / is_seg_scan) --
what every ConvBlock of a large crystal, and the benchmark, runs -- on every shape a 16-slot tile of receiver-sorted edges can take (tests/gpu_checks.py).

1. the scan in isolation: all 2^15 cuts of a tile into runs in ONE launch, and fifteen tail lengths, against the unfused rows summed per run in float64, under a
   bar derived from the four-step tree (check_fused_scatter_all_run_shapes);
2. the same launches (node rows gathered and rotated in the kernel: MessagePackBlock.run_nodes), with and without the fused scatter, against the fp64 oracle on
   graphs that put run ends on, before and behind tile ends (check_message_pack_nodes_forward), and one whole model on such a graph.
Every test says in its output which launch it ran and asserts it.  Tolerance of the oracle comparisons: G.TOL (1e-5 relative, max-norm)."""
import time

import pytest
import torch

from tests import gpu_checks as G

SH4 = "0e+1o+2e+3o+4e"                     # the harmonics of the "lmax = 4" set (bench.IRREPS["B"])

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def block():
    return G.fused_scatter_block()


# ---------------------------------------------------------------------------------------------- 1. every run shape, the scan in isolation


def test_fused_node_scatter_all_run_shapes(block):
    """all 32 768 cuts of a tile in one launch: 524 288 edges, 278 528 runs / receivers, 147 456 of them single-edge runs (one launch, so the full set stays)"""
    t0 = time.time()
    r = G.check_fused_scatter_all_run_shapes(block=block)
    print(r, {"seconds_whole_case": round(time.time() - t0, 2)})
    assert r["tiles"] == 32768 and r["E"] == 524288 and r["R"] == 278528 and (r["runs_per_tile_min"], r["runs_per_tile_max"]) == (1, 16), r
    assert r["single_edge_runs"] == 147456 and r["sentinel_allocations"] > 0, r
    G.assert_run_shapes(r)


@pytest.mark.parametrize("drop", range(1, 16))
def test_fused_node_scatter_ragged_tail(block, drop):
    """the last 1 .. 15 edges removed from 300 tiles: tail slots carry the ids -1 - slot and read a clamped edge; they must neither join a run nor write a row.
    The tail only exists in the last tile, so that tile is cut three ways: one run (the tail cuts it short), sixteen runs, and whatever the sample put there"""
    for last_cut in (0, 0x7fff, None):
        r = G.check_fused_scatter_all_run_shapes(block=block, cuts=300, drop=drop, last_cut=last_cut)
        print(r)
        assert r["tail_edges"] == 16 - drop and r["E"] == 4800 - drop and r["sentinel_allocations"] > 0, r
        G.assert_run_shapes(r)


# ---------------------------------------------------------------------------------------------- 2. the same launches against the fp64 oracle at tile edges


def _shipped(case):
    import bench
    return dict(irr=bench.IRREPS[case], sh=bench.SH if case == "A" else SH4)


@pytest.mark.parametrize("reduce", [False, True], ids=["rows", "reduce"])
@pytest.mark.parametrize("graph", G.SCATTER_GRAPHS)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_message_pack_single_part_nodes_forward_vs_oracle(seed, graph, reduce):
    """random irreps, one workgroup per tile forced, the gather and the rotation of the node rows inside the kernel; with and without the fused scatter"""
    r = G.check_message_pack_nodes_forward(graph=graph, seed=seed, parts=1, reduce=reduce)
    print(r)
    assert r["kernel"] == "is" and r["parts_used"] == 1 and r["reduce_ran"] == reduce and not r["reduce_skipped"], r
    assert r["rel_err"] < G.TOL, r


@pytest.mark.parametrize("graph", G.SCATTER_GRAPHS)
def test_message_pack_single_part_nodes_forward_eight_parts_vs_oracle(graph):
    """the launch of mid-size graphs (8 workgroups per tile, the plain program) forced on the same graphs: no fused scatter there"""
    r = G.check_message_pack_nodes_forward(graph=graph, seed=0, parts=8)
    print(r)
    assert r["kernel"] == "is" and r["parts_used"] == 8 and 1 < r["part_rows"] <= 8 and not r["reduce_ran"], r
    assert r["rel_err"] < G.TOL, r


def test_message_pack_single_part_nodes_forward_eight_parts_shipped_irreps():
    """the random irreps sets have fewer than 8 output segments, so 8 parts asked for are one part per segment there (`part_rows` in the output above); the "lmax = 4"
    set has more: 8 workgroups per tile with several segments each, as the dispatch runs a mid-size crystal"""
    r = G.check_message_pack_nodes_forward(graph="hub", seed=7, radial=(64, 64), parts=8, **_shipped("B"))
    print(r)
    assert r["kernel"] == "is" and r["parts_used"] == 8 and r["part_rows"] == 8 and not r["reduce_ran"], r
    assert r["rel_err"] < G.TOL, r


@pytest.mark.parametrize("reduce", [False, True], ids=["rows", "reduce"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_message_pack_single_part_nodes_forward_shipped_irreps(case, reduce):
    """both shipped irreps sets on the hub graph, 64-wide radial MLP (the split half-precision radial scale is compiled in).  A program whose LDS tiles fix several
    workgroups per tile cannot take the fused scatter: reported, the reduce leg of that set alone is left out"""
    r = G.check_message_pack_nodes_forward(graph="hub", seed=7, radial=(64, 64), parts=1, reduce=reduce, **_shipped(case))
    print(r)
    assert r["kernel"] == "is", r
    if r["fixed_parts"] == "lds":
        print(f"set {case}: the forward program's LDS tiles force several workgroups per tile: parts_used = {r['parts_used']!r}")
        if reduce:
            assert r["reduce_skipped"], r
            return
    else:
        assert r["parts_used"] == 1, r
    assert r["reduce_ran"] == reduce and r["rel_err"] < G.TOL, r


def test_message_pack_single_part_whole_model_on_the_hub_graph():
    """backbone + head on the hub graph, every input-stationary launch single-part: both ConvBlocks scatter in the edge kernel's epilogue"""
    r = G.oracle_vs_hip_random(graph="hub", parts=1, seed=2)
    print(r)
    L = r["launches"]
    assert r["E"] == 60 and L and all(l["kernel"] == "is" and l["parts"] == 1 for l in L) and sum(l["reduce"] for l in L) == 2, r
    assert r["node_rel_err"] < G.TOL and r["edge_rel_err"] < G.TOL and r["H_rel_err"] < G.TOL, r
