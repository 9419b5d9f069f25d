"""Centre-only edge sources (plan.build_message_pack_program(centre_edge=...)): the first layer's edge rows hold, per irrep of a spherical harmonic, the
m = 0 component only, so their even super-paths are issued with ONE column and their odd super-paths not at all.  Planner + emulator (tests/emu.py) on the
CPU: the reduced programs equal the complete ones on such rows, the skipped columns really are skipped, the tables keep the kernels' invariants."""
import numpy as np
import pytest
import torch

from hamgnn_amd import nn as hnn
from hamgnn_amd import plan as P
from hamgnn_amd import so3
from tests import centre_checks as C
from tests import emu
from tests.test_plan_emu import MINI, SH, rel

# reduced against complete program on the same rows, both emulated in float64: the bound tests/test_plan_emu.py puts on two programs that issue the same
# products in another grouping (test_merged_items_shipped_irreps: merged against plain)
SAME_PROGRAM_TOL = 1e-9


def _irreps(which):
    import bench
    return (MINI, SH) if which == "mini" else (bench.IRREPS[which], bench.SH)


def _lmax(irr, sh):
    return max(l for _, l, _ in list(so3.Irreps(irr)) + list(so3.Irreps(sh)))


def _block(which, seed=0):
    irr, sh = _irreps(which)
    torch.manual_seed(seed)
    m = hnn.MessagePackBlock(irr, irr, sh, irr, 8, [16, 16])
    return irr, sh, hnn._np_sd(m)


def _inputs(irr, sh, E, seed, node_full):
    rng = np.random.default_rng(seed + 100)
    n = rng.normal(size=(E, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    lmax = _lmax(irr, sh)
    D = emu.edge_wigner_all(n, lmax)
    xs, xd, fe = C.first_layer_rows(irr, sh, E, seed, node_full)
    h = [rng.normal(size=(E, 16)) for _ in range(2)]
    return [xs, xd, fe], tuple(h), D, lmax


def _programs(which, launch):
    """(complete, reduced) programs of the first ConvBlock ("conv": 0e node rows, un-rotated output) / first PairInteractionBlock ("pair": full node rows, skip
    Linear, edge-frame output) launch, each with the merge groups chosen for its own items as nn.MessagePackBlock.compile does"""
    irr, sh, sd = _block(which)
    zn, ze, ce = C.first_layer_sets(irr, sh)
    skip = np.random.default_rng(3).normal(size=sum(m * m for m, _, _ in so3.Irreps(irr))) if launch == "pair" else None
    kw = dict(zero_node=zn if launch == "conv" else (), zero_edge=ze, centre_edge=ce)
    g0 = P.choose_merge_groups(irr, irr, sh, irr, 16)
    g1 = P.choose_merge_groups(irr, irr, sh, irr, 16, **kw) or g0
    full = P.build_message_pack_program(sd, irr, irr, sh, irr, launch == "conv", skip, merge_groups=g0)
    red = P.build_message_pack_program(sd, irr, irr, sh, irr, launch == "conv", skip, merge_groups=g1, **kw)
    return irr, sh, sd, skip, kw, full, red


@pytest.mark.parametrize("which,launch,E", [("mini", "conv", 19), ("mini", "pair", 19), ("A", "conv", 5), ("A", "pair", 5)])
def test_centre_only_programs_equal_the_complete_ones_on_centre_only_rows(which, launch, E):
    irr, sh, sd, skip, kw, full, red = _programs(which, launch)
    srcs, h, D, lmax = _inputs(irr, sh, E, 1, node_full=launch == "pair")
    Dk = (D, lmax) if launch == "conv" else (None, None)
    want = emu.run_program_is(full, P.is_schedule(full), srcs, h, *Dk)
    sc = P.is_schedule(red)
    got = emu.run_program_is(red, sc, srcs, h, *Dk)
    assert np.abs(want).max() > 0 and rel(got, want) < SAME_PROGRAM_TOL
    # ... on split launches (several work groups per tile, private tile copies) ...
    assert rel(emu.run_program_is(red, P.is_schedule(red, 8), srcs, h, *Dk), want) < SAME_PROGRAM_TOL
    # ... and without merged row tiles, on both schedules (the twin of split launches; the segment-stationary fallback reads the same records)
    plain = P.build_message_pack_program(sd, irr, irr, sh, irr, launch == "conv", skip, **kw)
    assert rel(emu.run_program_is(plain, P.is_schedule(plain, plain.seg_table.shape[0]), srcs, h, *Dk), want) < SAME_PROGRAM_TOL
    if which == "mini":
        assert rel(emu.run_program(plain, srcs, h, *Dk), want) < SAME_PROGRAM_TOL
    # fewer issued MFMAs, fewer algorithmic flops, and the counters add up over the items that are there
    assert red.mfma_per_wave < full.mfma_per_wave and red.flops_per_row < full.flops_per_row and red.mfma_radial < full.mfma_radial
    hp4 = red.hidden_pad // 4
    assert red.mfma_radial == sum(hp4 * int(r[9]) for r in red.item_table if int(r[0]) == P.IT_TP)
    # the wrong twin: a non-zero m = +1 entry in ONE marked row moves the complete program's result, not the reduced one's -- the columns are not issued
    lay = P.PlanarLayout(irr)
    i = kw["centre_edge"][0]
    l = lay.irreps[i][1]
    bad = [s.copy() for s in srcs]
    bad[2][E // 2, lay.off[i] + (l + 1) * lay.mulp[i]] = 0.75
    assert rel(emu.run_program_is(full, P.is_schedule(full), bad, h, *Dk), want) > 1e-4
    assert np.array_equal(emu.run_program_is(red, sc, bad, h, *Dk), got)


@pytest.mark.parametrize("which", ["mini", "A", "B"])
@pytest.mark.parametrize("launch", ["conv", "pair"])
def test_centre_only_tables_keep_the_kernels_invariants(which, launch):
    irr, sh, sd, skip, kw, full, red = _programs(which, launch)
    lay = P.PlanarLayout(irr)
    ce = set(kw["centre_edge"])
    centre_off = {lay.off[i] + lay.irreps[i][1] * lay.mulp[i]: i for i in ce}
    # no item with one column carries the odd flag (the kernels have no ODD case at MM = 0: it would be skipped silently) -- in either program
    for prog in (full, red):
        assert not ((prog.item_table[:, 6] == 0) & (prog.item_table[:, 7] != 0)).any()
    # every item that reads a marked irrep reads its centre component as a one-component block (l = 0 at the component's offset), one column, even
    starts = {lay.off[i]: i for i in ce}
    n_centre = 0
    for r in red.item_table:
        if int(r[1]) != 2 or int(r[2]) >= 0:                   # (source slot 2 alone: the edge rows)
            continue
        assert int(r[3]) not in starts, "a marked irrep is still read over all its components"
        if int(r[3]) in centre_off:
            assert (int(r[5]), int(r[6]), int(r[7])) == (0, 0, 0) and int(r[4]) == lay.mulp[centre_off[int(r[3])]]
            n_centre += 1
    assert n_centre > 0
    # odd super-paths of the marked irreps are gone: the complete program has odd items over them, and the planner's count of their skipped centre MFMAs falls
    odd_full = sum(1 for r in full.item_table if int(r[0]) == P.IT_TP and int(r[7]) and int(r[1]) == 2 and int(r[2]) < 0 and int(r[3]) in starts)
    assert odd_full > 0 and red.mfma_odd_skipped < full.mfma_odd_skipped
    for parts in (1, 8):
        sc = P.is_schedule(red, parts)
        assert sc.lds_floats * 4 <= P.IS_LDS_BYTES
        for pt in sc.part_table:
            stage_floats = int(pt[6]) - int(pt[5])
            for b0, b1 in sc.phase_table[int(pt[2]):int(pt[2]) + int(pt[3]), :2]:
                used = 0
                for blk in sc.block_table[b0:b1]:              # every staged block inside the staging area, one after the other
                    s0, s1, in_off, in_mulp, li, nsrc, o0, o1 = (int(v) for v in blk)
                    size = -(-((2 * li + 1) * (in_mulp // 4)) // 4) * 256
                    assert o0 == used and 0 <= o0 and o0 + nsrc * size <= stage_floats
                    assert in_off + (2 * li + 1) * in_mulp <= lay.dim      # ... and its rows inside the source row
                    if s0 == 2 and in_off in centre_off:
                        assert li == 0 and size == -(-(in_mulp // 4) // 4) * 256      # one component's pieces
                    used += nsrc * size
        # the un-rotated segments of the first ConvBlock are fed by one-column items only: flagged for the centre-only epilogue, per l all or none;
        # nothing is flagged where the output stays in the edge frame or a tile gets more than its centre column
        flagged = {int(s[0]) for s in sc.seg_table if int(s[7]) & P.SEG_CENTRE}
        if launch == "conv":
            assert flagged == {int(s[0]) for s in sc.seg_table if int(s[0]) > 0}
            assert all(bool(int(s[7]) & P.SEG_CENTRE) == (int(s[0]) > 0) for s in sc.seg_table)
        else:
            assert not flagged
        assert not any(int(s[7]) & P.SEG_CENTRE for s in P.is_schedule(full, parts).seg_table)


def test_merge_groups_are_chosen_for_the_items_the_reduced_program_has():
    """a one-column item stacks whatever its l: with the centre-only sources the chooser's cost is the reduced program's, and its choice is no dearer for that
    program than the complete program's groups"""
    irr, sh, sd = _block("A")
    zn, ze, ce = C.first_layer_sets(irr, sh)
    for kw in (dict(zero_node=zn, zero_edge=ze, centre_edge=ce), dict(zero_edge=ze, centre_edge=ce)):
        g0 = P.choose_merge_groups(irr, irr, sh, irr, 16)
        g1 = P.choose_merge_groups(irr, irr, sh, irr, 16, **kw)
        a = P.build_message_pack_program(sd, irr, irr, sh, irr, True, merge_groups=g0, **kw)
        b = P.build_message_pack_program(sd, irr, irr, sh, irr, True, merge_groups=g1, **kw)
        assert b.mfma_per_wave <= a.mfma_per_wave
    assert P.choose_merge_groups(irr, irr, sh, irr, 16, centre_edge=()) == P.choose_merge_groups(irr, irr, sh, irr, 16)


def test_set_a_counts_of_the_first_two_launches():
    """the planner's figures the profile note quotes (set-A, 64 hidden units, merge groups as compiled): fp32 GEMM1 + GEMM2 MFMAs per 16-edge tile of the
    edge-branch items, with and without the centre-only sources"""
    import bench
    irr, sh = bench.IRREPS["A"], bench.SH
    torch.manual_seed(0)
    sd = hnn._np_sd(hnn.MessagePackBlock(irr, irr, sh, irr, 64, [64, 64]))
    zn, ze, ce = C.first_layer_sets(irr, sh)

    def edge_gemm(prog):
        tot = 0
        for r in prog.item_table:
            if int(r[0]) == P.IT_TP and int(r[1]) == 2 and int(r[2]) < 0:
                nc, rto = 2 * int(r[6]) + 1, P.schedule_is._item_rto(r, prog.seg_table, prog.vsegs)
                tot += (nc - (1 if int(r[7]) and int(r[6]) > 0 else 0)) * (int(r[8]) * int(r[9]) + rto * int(r[18]))
        return tot

    for zkw in (dict(zero_node=zn, zero_edge=ze), dict(zero_edge=ze)):
        g0 = P.choose_merge_groups(irr, irr, sh, irr, 64)
        a = P.build_message_pack_program(sd, irr, irr, sh, irr, True, merge_groups=g0, **zkw)
        g1 = P.choose_merge_groups(irr, irr, sh, irr, 64, centre_edge=ce, **zkw) or g0
        b = P.build_message_pack_program(sd, irr, irr, sh, irr, True, merge_groups=g1, centre_edge=ce, **zkw)
        assert edge_gemm(a) - edge_gemm(b) == 3871 and a.mfma_radial - b.mfma_radial == 29 * 16
