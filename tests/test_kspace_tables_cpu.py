"""kspace.CrystalTables against the derivations it replaced, restated here in numpy, on the two-crystal batch of tests/kspace_tables_checks.py: every table
with exact equality."""
import numpy as np
import torch

from hamgnn_amd import bonds, kspace
from tests import kspace_tables_checks as KC
from tests import train_targets_checks as TT


def _old_tables(g, n0, n, e0, e, orank_all):
    """the free functions' tables in numpy: row / column atom, shift, orank, ooff, M, the pair tables (stable sort of src * n + dst) and the compact index"""
    src, dst = (g.edge_index[r][e0:e0 + e].numpy() - n0 for r in (0, 1))
    orank = orank_all[n0:n0 + n].numpy()
    norb = (orank >= 0).sum(1)
    ooff = np.cumsum(norb) - norb
    key = src * n + dst
    order = np.argsort(key, kind="stable")
    uniq, counts = np.unique(key[order], return_counts=True)
    return dict(erow=src, ecol=dst, shift=g.nbr_shift[e0:e0 + e].numpy(), orank=orank, ooff=ooff, M=int(norb.sum()),
                pair_ptr=np.concatenate([[0], np.cumsum(counts)]), pair_edges=order, pair_ij=np.stack([uniq // n, uniq % n], 1),
                compact_index=np.where(orank >= 0, ooff[:, None] + orank, -1))


def test_tables_equal_the_old_derivations():
    g = KC.batch()
    orank_all = TT.orank_table("openmx", KC.NAO)[g.z]
    slices = kspace._crystal_slices(g)
    assert slices == [(0, 2, 0, 4), (2, 3, 4, 8)]
    for n0, n, e0, e in slices:
        t = kspace.CrystalTables.from_graph(g, n0, n, e0, e, orank_all)
        want = _old_tables(g, n0, n, e0, e, orank_all)
        assert (t.n0, t.n, t.e0, t.e, t.nao, t.M) == (n0, n, e0, e, KC.NAO, want["M"])
        for name in ("erow", "ecol", "shift", "orank", "ooff", "pair_ptr", "pair_edges", "pair_ij", "compact_index"):
            got = getattr(t, name)
            assert got.is_contiguous() and np.array_equal(got.numpy(), want[name]), name
        assert t.erow.dtype == t.ecol.dtype == t.orank.dtype == t.ooff.dtype == torch.int32 and t.shift.dtype == torch.float32
        assert t.pair_ptr.dtype == t.pair_edges.dtype == t.pair_ij.dtype == t.compact_index.dtype == torch.int64
        assert t.pair_ptr is t.pair_ptr and t.compact_index is t.compact_index                      # computed once, then kept
    assert (want["orank"] < 0).any() and want["M"] == 13 + 13 + 5
    # crystal B: two edges on the pair (0, 1) in edge order, the self image (2, 2), no pair (0, 2) or (2, 0)
    pairs = [tuple(p) for p in want["pair_ij"].tolist()]
    assert pairs == [(0, 1), (1, 0), (1, 2), (2, 1), (2, 2)]
    assert t.pair_edges[t.pair_ptr[0]:t.pair_ptr[1]].tolist() == [0, 3] and t.pair_edges[t.pair_ptr[4]:t.pair_ptr[5]].tolist() == [1, 7]


def test_spin_orbit_step_builds_the_tables_once_per_crystal_on_the_cpu_twin(monkeypatch):
    """tests/test_kspace_tables_gpu.py on cpu_ops.hk_assemble, the CPU twin of hg_hk_assemble"""
    from tests import cpu_ops
    cpu_ops.install(monkeypatch)
    KC.check_built_once("cpu", monkeypatch)


def test_bond_tables_build_the_same_object_from_an_uncompiled_head():
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    g = KC.batch()
    n0, n, e0, e = kspace._crystal_slices(g)[1]
    t = kspace.CrystalTables.from_graph(g, n0, n, e0, e, TT.orank_table("openmx", KC.NAO)[g.z])
    head = HamGNNPlusPlusOut("4x0e", "4x0e", nao_max=KC.NAO, ham_type="openmx", ham_only=True, calculate_sparsity=False)
    assert head._orank is None
    b = bonds.bond_tables(head, g.z[n0:n0 + n], g.edge_index[:, e0:e0 + e] - n0, g.cell_shift[e0:e0 + e], "cpu")
    assert isinstance(b, kspace.CrystalTables) and (b.n0, b.n, b.e0, b.e, b.nao, b.M) == (0, n, 0, e, KC.NAO, t.M)
    for name in ("orank", "ooff", "erow", "ecol"):
        assert torch.equal(getattr(b, name), getattr(t, name)) and getattr(b, name).dtype == torch.int32, name
    assert b["erow"] is b.erow and b["M"] == b.M                                                   # read by field name, as from the dict it used to be
    assert torch.equal(b.shift, g.cell_shift[e0:e0 + e].float())                                # the shift it was given: integer cell shifts here
    assert torch.equal(head.compile("cpu")._orank, torch.from_numpy(TT.orank_table("openmx", KC.NAO).numpy()))
