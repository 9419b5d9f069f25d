"""hamgnn_amd/bonds.py without a GPU: bond_groups and bond_tables (host logic), the defining identity on the fp64 statement, the cross-check with the
Mulliken path, and the torch path and the numpy twin of hg_bond_weights (tests/bond_checks.py) against the fp64 statement."""
import numpy as np
import pytest
import torch

from hamgnn_amd import bonds, dos
from tests import bond_checks as BC

NAOS = sorted(BC.HEADS)


def _toy():
    """4 atoms (the last without an edge): 0 -> 1 and its inverse, a self-image pair on atom 0, an edge 2 -> 1 WITHOUT inverse, two images of 0 -> 2 with inverses"""
    ei = np.array([[0, 1, 0, 0, 2, 0, 2, 0, 2], [1, 0, 0, 0, 1, 2, 0, 2, 0]])
    sh = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, -1]])
    z = np.array([14, 8, 8, 1])
    pos = np.array([[0.0, 0, 0], [1.5, 0, 0], [0, 2.5, 0], [9.0, 9, 9]])
    return ei, sh, z, pos, 10.0 * np.eye(3)


def _members(ptr, idx):
    return [list(idx[ptr[g]:ptr[g + 1]]) for g in range(len(ptr) - 1)]


@pytest.mark.parametrize("by", bonds.BY)
def test_bond_groups_partition_the_edges_and_atoms(by):
    ei, sh, z, pos, cell = _toy()
    eptr, eidx, aptr, aidx, labels = bonds.bond_groups(ei, sh, z, by=by, onsite=True)
    assert eptr.dtype == eidx.dtype == aptr.dtype == aidx.dtype == np.int32 and len(eptr) == len(aptr) == len(labels) + 1
    assert sorted(eidx.tolist()) == list(range(ei.shape[1]))           # without rmax: every edge in exactly one group
    assert sorted(aidx.tolist()) == list(range(len(z)))                # onsite: every atom in exactly one group, the edge-less atom 3 included
    eg, ag = _members(eptr, eidx), _members(aptr, aidx)
    assert all(bool(e) != bool(a) for e, a in zip(eg, ag))             # a group holds edges or on-site blocks
    if by == "edge":
        assert [g for g in eg if g] == [[0, 1], [2, 3], [4], [5, 6], [7, 8]]      # inverse pairs, the self-image pair, the edge without an inverse alone
        for g in eg:
            if len(g) == 2:
                a, b = g
                assert (ei[0, a], ei[1, a]) == (ei[1, b], ei[0, b]) and np.array_equal(sh[a], -sh[b])
        assert labels[0] == ("Si", 0, "O", 1, (0, 0, 0)) and labels[1] == ("Si", 0, "Si", 0, (1, 0, 0)) and labels[-1] == ("H", 3)
        assert [a for a in ag if a] == [[0], [1], [2], [3]]
    elif by == "pair":
        assert [g for g in eg if g] == [[2, 3], [0, 1], [5, 6, 7, 8], [4]]          # ascending (i, j): (0, 0), (0, 1), (0, 2), (1, 2)
        assert labels[:4] == [("Si", 0, "Si", 0), ("Si", 0, "O", 1), ("Si", 0, "O", 2), ("O", 1, "O", 2)] and labels[4] == ("Si", 0)
    else:
        assert [g for g in eg if g] == [[4], [0, 1, 5, 6, 7, 8], [2, 3]]            # ascending (Z, Z'): (8, 8), (8, 14), (14, 14)
        assert labels == [("O", "O"), ("O", "Si"), ("Si", "Si"), ("H",), ("O",), ("Si",)]
        assert [a for a in ag if a] == [[3], [1, 2], [0]]


@pytest.mark.parametrize("by", bonds.BY)
def test_bond_groups_rmax_and_labels_with_lengths(by):
    ei, sh, z, pos, cell = _toy()
    with pytest.raises(ValueError, match="rmax needs pos"):
        bonds.bond_groups(ei, sh, z, by=by, rmax=3.0)
    with pytest.raises(ValueError, match="go together"):
        bonds.bond_groups(ei, sh, z, by=by, pos=pos)
    length = np.linalg.norm(pos[ei[1]] + sh @ cell - pos[ei[0]], axis=1)
    eptr, eidx, aptr, aidx, labels = bonds.bond_groups(ei, sh, z, by=by, onsite=False, pos=pos, cell=cell, rmax=3.0)
    kept = sorted(eidx.tolist())
    assert kept == [e for e in range(ei.shape[1]) if length[e] <= 3.0] == [0, 1, 4, 5, 6] and len(set(kept)) == len(kept)      # at most one group each
    assert len(aidx) == 0 and not aptr.any() and len(labels) == len(eptr) - 1
    for g, lab in enumerate(labels):                                   # the label ends with the length of the group's shortest edge
        assert isinstance(lab[-1], float) and lab[-1] == length[eidx[eptr[g]:eptr[g + 1]]].min()
    fptr, _, _, _, full = bonds.bond_groups(ei, sh, z, by=by, onsite=True, pos=pos, cell=cell)
    assert all(isinstance(lab[-1], float) == bool(fptr[g + 1] > fptr[g]) for g, lab in enumerate(full))      # on-site labels carry no length


def test_bond_groups_refuses_what_it_cannot_read():
    ei, sh, z, pos, cell = _toy()
    with pytest.raises(ValueError, match="by="):
        bonds.bond_groups(ei, sh, z, by="atom")
    with pytest.raises(ValueError, match="integer cell shifts"):
        bonds.bond_groups(ei, sh + 0.25, z)
    with pytest.raises(ValueError, match="outside"):
        bonds.bond_groups(ei + 2, sh, z)


@pytest.mark.parametrize("nao", NAOS)
def test_bond_tables_follow_the_assembly_convention(nao):
    """orank / ooff / M as kspace.CrystalTables derives them from the head's table; row / column atom = edge_index[0] / [1]"""
    c = BC.case(nao)
    t = bonds.bond_tables(c.head, c.z, c.ei, c.shift, "cpu")
    assert t.M == c.M and t.nao == nao and (t.orank < 0).any()
    assert np.array_equal(t.ooff.numpy(), c.off0[:-1]) and t.ooff.dtype == t.orank.dtype == t.erow.dtype == torch.int32
    for i, orb in enumerate(c.orbs):
        assert np.array_equal(np.nonzero(t.orank[i].numpy() >= 0)[0], orb) and np.array_equal(t.orank[i].numpy()[orb], np.arange(len(orb)))
    assert np.array_equal(t.erow.numpy(), c.ei[0]) and np.array_equal(t.ecol.numpy(), c.ei[1]) and np.array_equal(t.shift.numpy(), c.shift)
    with pytest.raises(ValueError, match="no element"):
        bonds.bond_tables(c.head, np.array([118]), np.zeros((2, 0), dtype=np.int64), np.zeros((0, 3)), "cpu")


@pytest.mark.parametrize("by", bonds.BY)
@pytest.mark.parametrize("nao", NAOS)
def test_defining_identity_on_the_fp64_statement(nao, by):
    """all edges and atoms grouped: sum_g W[s, 1 + g] = wk[s] Re(c_s^+ X(k_s) c_s), X(k) the dense complex128 assembly, to 1e-12 relative"""
    c = BC.case(nao)
    groups = BC.groupings(c)[by]
    G = len(groups[0]) - 1
    W, T, _, _ = BC.ref_bond_weights(c, groups, 1 + G)
    Cd = c.C.astype(np.complex128)
    want = np.empty(c.ns)
    for kp in range(len(c.kvec)):
        Xk = BC.dense_xk(c, c.Xon, c.Xoff, c.kvec[kp].astype(np.float64))
        rows = c.kidx == kp
        want[rows] = c.wk[rows] * np.einsum("sa,ab,sb->s", Cd[rows].conj(), Xk, Cd[rows]).real
    assert np.abs(W[:, 1:].sum(1) - want).max() <= 1e-12 * T[:, 1:].sum(1).max()


@pytest.mark.parametrize("nao", NAOS)
def test_row_atom_groups_are_the_mulliken_populations_fp64(nao):
    """every directed edge grouped by its row atom + the atom's on-site block, on overlap-like rows: the fp64 statement equals dos._mulliken_torch(C, S(k) C,
    "atom" groups) in fp64"""
    c = BC.case(nao)
    groups = BC.row_atom_groups(c)
    W, T, _, _ = BC.ref_bond_weights(c, groups, 1 + c.N)
    Cd = c.C.astype(np.complex128)
    SC = np.empty_like(Cd)
    for kp in range(len(c.kvec)):
        rows = c.kidx == kp
        SC[rows] = Cd[rows] @ BC.dense_xk(c, c.Xon, c.Xoff, c.kvec[kp].astype(np.float64)).T          # rows of (S(k) c)^T
    perm, gptr, labels = dos.group_map(c.head, c.z, "atom")
    assert len(labels) == c.N
    Wm = dos._mulliken_torch(torch.from_numpy(Cd), torch.from_numpy(SC), torch.from_numpy(perm), torch.from_numpy(gptr), torch.from_numpy(c.wk), 1 + c.N)
    terms = (Cd.real * SC.real + Cd.imag * SC.imag)
    Wd = np.stack([c.wk * terms[:, perm[gptr[g]:gptr[g + 1]]].sum(1) for g in range(c.N)], 1)       # the same group sums in fp64
    assert np.abs(W[:, 1:] - Wd).max() <= 1e-12 * T[:, 1:].max()
    assert np.abs(Wm.numpy()[:, 1:] - Wd).max() <= (c.M + 4) * BC.U * T[:, 1:].max()              # (_mulliken_torch's matmul is fp32)


@pytest.mark.parametrize("ns", [1, 17, 33])
@pytest.mark.parametrize("nao", NAOS)
def test_torch_path_within_the_bound(nao, ns):
    c = BC.case(nao)
    for name, groups in BC.groupings(c).items():
        G = len(groups[0]) - 1
        for Gp in sorted({1 + G, dos.padded_groups(G)}):
            assert BC.check_weights(BC.run(c, groups, Gp, "cpu", ns=ns), c, groups, Gp, ns=ns, kernel=False) <= 1.0, (name, Gp)


@pytest.mark.parametrize("ns", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("nao", NAOS)
def test_twin_within_the_kernel_bound(nao, ns, monkeypatch):
    """the numpy twin installed in place of ops.bond_weights: bonds.bond_weights takes its kernel route"""
    BC.install_cpu(monkeypatch)
    c = BC.case(nao)
    for name, groups in BC.groupings(c).items():
        G = len(groups[0]) - 1
        for Gp in sorted({1 + G, dos.padded_groups(G)}):
            assert BC.check_weights(BC.run(c, groups, Gp, "cpu", ns=ns), c, groups, Gp, ns=ns, kernel=True) <= 1.0, (name, Gp)


def test_bond_weights_checks_its_arguments_on_cpu():
    c = BC.case(13)
    groups = BC.groupings(c)["pair"]
    G = len(groups[0]) - 1
    with pytest.raises(ValueError, match="Gp"):
        BC.run(c, groups, G, "cpu")
    with pytest.raises(ValueError, match="orbital columns"):
        BC.run(c, groups, 1 + G, "cpu", C=c.C[:, :-1])


def test_library_exports_the_entry_point_and_needs_no_scratch():
    import ctypes as C
    from hamgnn_amd import _lib
    L = _lib.lib()
    assert "hg_bond_weights" in _lib.EXPORTS and hasattr(L, "hg_bond_weights")
    L.hg_scratch_bytes.restype, L.hg_scratch_bytes.argtypes = C.c_int64, [C.c_char_p, C.c_int64, C.c_int]
    assert L.hg_scratch_bytes(b"hg_bond_weights", 1000, 0) == 0
