"""Phase record [5] of the input-stationary schedule (plan/schedule_is.py): set exactly on the phases whose tensor-product items use both radial generators -- the
kernel keeps both generators' hidden rows resident there.  Checked on the complete and the reduced first-layer programs of set-A (64 hidden units) and of the mini
irreps; the schedules themselves (which form is_schedule picks, the phase, group, item and block tables) keep the shapes they had before the flag existed."""
import numpy as np
import pytest
import torch

from hamgnn_amd import nn as hnn
from hamgnn_amd import plan as P
from hamgnn_amd import so3
from tests import centre_checks as C
from tests.test_plan_emu import MINI, SH


def _programs(which, launch):
    """(complete, reduced) programs of the first ConvBlock ("conv") / first PairInteractionBlock ("pair") launch, merge groups chosen as nn.MessagePackBlock.compile does"""
    import bench
    irr, sh, hid = (MINI, SH, 16) if which == "mini" else (bench.IRREPS[which], bench.SH, 64)
    torch.manual_seed(0)
    sd = hnn._np_sd(hnn.MessagePackBlock(irr, irr, sh, irr, hid, [hid, hid]))
    zn, ze, ce = C.first_layer_sets(irr, sh)
    skip = np.random.default_rng(3).normal(size=sum(m * m for m, _, _ in so3.Irreps(irr))) if launch == "pair" else None
    kw = dict(zero_node=zn if launch == "conv" else (), zero_edge=ze, centre_edge=ce)
    g0 = P.choose_merge_groups(irr, irr, sh, irr, hid)
    g1 = P.choose_merge_groups(irr, irr, sh, irr, hid, **kw) or g0
    full = P.build_message_pack_program(sd, irr, irr, sh, irr, launch == "conv", skip, merge_groups=g0)
    red = P.build_message_pack_program(sd, irr, irr, sh, irr, launch == "conv", skip, merge_groups=g1, **kw)
    return full, red


def _generators_per_phase(sc):
    out = []
    for p in sc.phase_table:
        cls = set()
        for gi in range(int(p[2]), int(p[3])):
            b, e = sc.group_table[gi]
            cls |= {int(it[10]) for it in sc.item_table[b:e] if int(it[0]) == P.IT_TP}
        out.append(cls)
    return out


# (phases, flagged phases, work groups, items, staged blocks) of the single-part schedule
SHAPES = {
    ("A", "conv", "full"): (12, 0, 98, 260, 26),
    ("A", "conv", "red"): (2, 1, 10, 37, 7),
    ("A", "pair", "full"): (12, 0, 98, 273, 26),
    ("A", "pair", "red"): (8, 4, 67, 168, 19),
    ("mini", "conv", "full"): (1, 1, 4, 56, 14),
    ("mini", "conv", "red"): (1, 1, 1, 5, 5),
    ("mini", "pair", "full"): (1, 1, 4, 63, 14),
    ("mini", "pair", "red"): (1, 1, 4, 40, 11),
}


@pytest.mark.parametrize("which,launch", [("A", "conv"), ("A", "pair"), ("mini", "conv"), ("mini", "pair")])
def test_flag_marks_the_phases_that_mix_both_generators(which, launch):
    for name, prog in zip(("full", "red"), _programs(which, launch)):
        for parts in (1, 8):
            sc = P.is_schedule(prog, parts)
            pt = sc.phase_table
            assert pt.shape[1] == 8 and not pt[:, 6:].any()
            gens = _generators_per_phase(sc)
            assert pt[:, 5].tolist() == [int(g == {0, 1}) for g in gens], (which, launch, name, parts)
            # column 4 keeps its meaning: a generator the phase uses (-1: no tensor-product item)
            assert all((int(p[4]) in g) if g else int(p[4]) == -1 for p, g in zip(pt, gens))
            if parts == 1:
                got = (int(pt.shape[0]), int(pt[:, 5].sum()), int(sc.group_table.shape[0]), int(sc.item_table.shape[0]), int(sc.block_table.shape[0]))
                assert got == SHAPES[(which, launch, name)], (which, launch, name, got)
    # the complete set-A programs run one generator per phase; their reduced first-layer twins mix
    if which == "A":
        assert SHAPES[(which, launch, "full")][1] == 0 and SHAPES[(which, launch, "red")][1] > 0
