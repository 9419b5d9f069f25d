"""The pieces the post-solver modules share (kspace.padded_rows, kspace.edge_phases, dos._fold_time_reversal) against the derivations they replaced,
written out here as bonds.py, density.py, velocity.py and dos.py had them.  CPU only."""
import numpy as np
import pytest
import torch

from hamgnn_amd import bonds, dos, kspace
from tests import bond_checks as BC

GRIDS = [(1, 1, 1), (2, 2, 2), (3, 2, 1), (4, 4, 4)]


@pytest.mark.parametrize("nao", [13, 19])
@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_padded_rows_is_the_gather_of_the_three_torch_paths(nao, dtype):
    """3 atoms + 1 of two elements with different orbital counts: missing orbitals read the appended zero column"""
    c = BC.case(nao)
    t = bonds.bond_tables(c.head, c.z, c.ei, c.shift, "cpu")
    C = torch.from_numpy(c.C).to(dtype)
    ns, M = C.shape
    have = t.orank >= 0
    assert not bool(have.all()) and len({int(v) for v in have.sum(1)}) >= 2
    comp = torch.where(have, t.ooff[:, None] + t.orank, torch.full_like(t.orank, M)).long()
    CA = torch.cat([C, C.new_zeros(ns, 1)], 1)[:, comp]
    got, got_have = kspace.padded_rows(C, t.orank, t.ooff)
    assert got.dtype == dtype and tuple(got.shape) == (ns, c.N, nao) and torch.equal(got, CA)
    assert got_have.dtype == torch.bool and torch.equal(got_have, have)
    assert not bool(got[:, ~have].abs().max() > 0) and torch.equal(got[:, have], C[:, comp[have]])


@pytest.mark.parametrize("rdt", [torch.float32, torch.float64])
def test_edge_phases_forms_the_angle_in_double_and_rounds_once(rdt):
    """shifts of tens of cells: the fp32 angle would lose the fraction of a turn"""
    gen = torch.Generator().manual_seed(3)
    k = torch.rand(7, 3, generator=gen) - 0.5                                      # fp32 reduced k-points
    shift = torch.randint(-40, 41, (11, 3), generator=gen).float()
    shift[0] = torch.tensor([30.0, -37.0, 40.0])
    ang = 2.0 * np.pi * (k.double() @ shift.double().T)
    want = torch.complex(torch.cos(ang).to(rdt), torch.sin(ang).to(rdt))
    got = kspace.edge_phases(k, shift, rdt)
    assert got.dtype == want.dtype and tuple(got.shape) == (7, 11) and torch.equal(got, want)
    assert torch.equal(kspace.edge_phases(k.double(), shift.double(), rdt), want)      # (operands already in double: the same bits)
    single = 2.0 * np.pi * (k @ shift.T)                                           # the angle in fp32: its ulp at tens of turns is 1e-5
    assert float((torch.cos(single).double() - torch.cos(ang)).abs().max()) > 1e-6
    assert float((got.real.double() - torch.cos(ang)).abs().max()) <= (2.0 ** -24 if rdt == torch.float32 else 0.0)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shift", [(0, 0, 0), (0.5, 0, 0)])
@pytest.mark.parametrize("time_reversal", [True, False])
def test_folded_list_and_map_are_consistent(grid, shift, time_reversal):
    """monkhorst_pack(...)[0][monkhorst_pack_map(...)] is the full-grid point or its negative modulo 1; both are built on dos._fold_time_reversal"""
    k_full, w_full = dos.monkhorst_pack(grid, shift, time_reversal=False)
    k, w = dos.monkhorst_pack(grid, shift, time_reversal)
    m = dos.monkhorst_pack_map(grid, shift, time_reversal)
    assert m.dtype == np.int32 and m.shape == (len(k_full),) and sorted(set(m.tolist())) == list(range(len(k)))
    mod1 = lambda d: np.abs((d + 0.5) % 1.0 - 0.5).max(1)
    same, minus = mod1(k_full - k[m]) < 1e-12, mod1(k_full + k[m]) < 1e-12
    assert (same | minus).all() and (time_reversal or same.all())
    fold = list(dos._fold_time_reversal(k_full))
    assert [r for r, _ in fold] == m.tolist() or not time_reversal
    if time_reversal:
        kept = [i for i, (_, keep) in enumerate(fold) if keep]
        assert np.array_equal(k_full[kept], k) and [fold[i][0] for i in kept] == list(range(len(k)))      # kept rows are numbered in grid order
        assert all(same[i] for i in kept) and all(fold[i][0] < len(kept) and kept[fold[i][0]] < i for i in range(len(fold)) if not fold[i][1])
        assert np.array_equal(w, np.bincount(m, weights=w_full)) and abs(w.sum() - 1.0) < 1e-14
