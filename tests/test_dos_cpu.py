"""The DOS parts of hamgnn_amd/dos.py without a GPU: the k-grid, the orbital-group maps, the Fermi level, the energy grid, the C ABI of the two new entry
points, the numpy twins of the kernels (tests/dos_checks.py) and the plain torch path against fp64, and the chain weights -> sort -> broadening in chunks on
the exact eigenpairs of the fixture crystals."""
import os
import re

import numpy as np
import pytest
import torch

from hamgnn_amd import _lib, dos, ops
from tests import dos_checks as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_header_exports_and_zero_scratch():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "hamgnn_hip.h")).read()
    declared = set(re.findall(r"\b(hg_[a-z_0-9]+)\s*\(", hdr))
    for name in ("hg_mulliken_weights", "hg_dos_broaden"):
        assert name in declared and name in _lib.EXPORTS
    assert declared == set(_lib.EXPORTS)
    assert callable(ops.mulliken_weights) and callable(ops.dos_broaden)
    _lib.build()
    L = _lib.lib()
    L.hg_scratch_bytes.restype = C.c_int64
    L.hg_scratch_bytes.argtypes = [C.c_char_p, C.c_int64, C.c_int]
    assert L.hg_scratch_bytes(b"hg_mulliken_weights", 1000, 0) == 0 and L.hg_scratch_bytes(b"hg_dos_broaden", 1000, 0) == 0
    assert "spectra.hip" in open(os.path.join(ROOT, "hamgnn_amd", "csrc", "Makefile")).read().split("SRCS", 1)[1].split("\n", 1)[0]


def test_entry_points_check_their_arguments_and_launch_nothing_for_empty_sizes():
    """host-side argument checks of the C ABI.  Every call passes NULL pointers only, and sizes that are either empty (0 before any launch) or refused whatever
    the pointers are: no call here can reach a launch"""
    import ctypes as C
    L = _lib.lib()
    null = C.c_void_p(0)
    d = C.c_double
    assert L.hg_mulliken_weights(null, null, C.c_int64(0), 4, null, null, 1, 2, null, null, null) == 0                   # no state
    assert L.hg_mulliken_weights(null, null, C.c_int64(3), 4, null, null, 2, 2, null, null, null) == -2                  # Gp < 1 + G
    assert b"hg_mulliken_weights" in L.hg_last_error()
    assert L.hg_mulliken_weights(null, null, C.c_int64(3), 0, null, null, 0, 1, null, null, null) == -2                  # M = 0
    assert L.hg_mulliken_weights(null, null, C.c_int64(3), 4, null, null, 0, 1, null, null, null) == -2                  # good sizes, NULL tensors
    assert L.hg_dos_broaden(null, null, C.c_int64(5), 0, d(0.0), d(0.1), 10, d(0.1), 0, null, null) == 0                 # no column
    assert L.hg_dos_broaden(null, null, C.c_int64(5), 4, d(0.0), d(0.1), 0, d(0.1), 0, null, null) == 0                  # no energy
    assert L.hg_dos_broaden(null, null, C.c_int64(5), 4, d(0.0), d(0.1), 10, d(0.0), 0, null, null) == -2                # sigma = 0
    assert b"hg_dos_broaden" in L.hg_last_error()
    assert L.hg_dos_broaden(null, null, C.c_int64(5), 4, d(0.0), d(-0.1), 10, d(0.1), 0, null, null) == -2               # descending grid
    assert L.hg_dos_broaden(null, null, C.c_int64(-1), 4, d(0.0), d(0.1), 10, d(0.1), 0, null, null) == -2
    assert L.hg_dos_broaden(null, null, C.c_int64(5), 4, d(0.0), d(0.1), 10, d(0.1), 0, null, null) == -2                # good sizes, NULL tensors


def test_wrappers_refuse_sliced_tensors():
    """ops.mulliken_weights / ops.dos_broaden raise before the library is reached when a tensor is not contiguous or has the wrong type"""
    import pytest as _p
    mp = _p.MonkeyPatch()
    mp.setattr(ops, "_require_gpu", lambda t: None)
    try:
        eps, W, D = torch.zeros(6), torch.zeros(6, 8), torch.zeros(4, 8)
        for bad in (dict(eps=torch.zeros(12)[::2]), dict(W=torch.zeros(6, 16)[:, ::2]), dict(D=torch.zeros(4, 16)[:, :8])):
            kw = dict(eps=eps, W=W, D=D)
            kw.update(bad)
            with pytest.raises(ValueError, match="contiguous"):
                ops.dos_broaden(kw["eps"], kw["W"], 0.0, 0.1, 4, 0.1, D=kw["D"])
        C_ = torch.zeros(3, 4, dtype=torch.complex64)
        perm, gptr, wk = torch.arange(4, dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32), torch.ones(3)
        with pytest.raises(ValueError, match="contiguous"):
            ops.mulliken_weights(C_, C_, torch.arange(8, dtype=torch.int32)[::2], gptr, wk, 2)
        with pytest.raises(ValueError, match="contiguous"):
            ops.mulliken_weights(C_, C_, perm, gptr, torch.ones(6)[::2], 2)
        with pytest.raises(ValueError, match="Gp"):
            ops.mulliken_weights(C_, C_, perm, gptr, wk, 1)
    finally:
        mp.undo()


def test_monkhorst_pack_grid():
    k, w = dos.monkhorst_pack((1, 1, 1))
    assert k.shape == (1, 3) and not k.any() and w.tolist() == [1.0]
    for grid, shift in (((4, 4, 4), (0, 0, 0)), ((3, 2, 5), (0, 0, 0)), ((4, 4, 2), (0.5, 0.5, 0.5)), ((3, 3, 1), (0.25, 0, 0))):
        kf, wf = dos.monkhorst_pack(grid, shift, time_reversal=False)
        kr, wr = dos.monkhorst_pack(grid, shift, time_reversal=True)
        assert len(kf) == int(np.prod(grid)) and abs(wf.sum() - 1) < 1e-14 and abs(wr.sum() - 1) < 1e-14
        assert kf.min() > -0.5 - 1e-12 and kf.max() <= 0.5 + 1e-12
        if not any(shift):
            assert not kf[0].any() and len(kr) == (len(kf) + sum(1 for q in kf if np.allclose((2 * q) % 1.0, 0, atol=1e-9) or np.allclose((2 * q) % 1.0, 1, atol=1e-9))) // 2
        # every point of the full grid is a kept point or minus a kept point (modulo 1), with the weights adding up
        tot = np.zeros(len(kr))
        for q in kf:
            hit = [i for i, p in enumerate(kr) if np.allclose((q - p + 0.5) % 1.0, 0.5, atol=1e-9) or np.allclose((q + p + 0.5) % 1.0, 0.5, atol=1e-9)]
            assert len(hit) == 1, (grid, shift, q)
            tot[hit[0]] += 1.0 / len(kf)
        assert np.allclose(tot, wr, atol=1e-14)
    assert len(dos.monkhorst_pack((4, 4, 4))[0]) == 36
    with pytest.raises(ValueError):
        dos.monkhorst_pack((4, 0, 4))


def test_group_maps_of_the_three_projections():
    """the fixture's second crystal: O (13 orbitals: s s p p d), H (5: s s p), C (13)"""
    head = DC.head13()
    z = DC.fixture_crystals()[1][0]
    assert z.tolist() == [8, 1, 6]
    assert dos.orbital_shells(head).tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2]
    perm, gptr, lab = dos.group_map(head, z, "atom")
    assert lab == [("O", 0), ("H", 1), ("C", 2)] and gptr.tolist() == [0, 13, 18, 31] and perm.tolist() == list(range(31))
    perm, gptr, lab = dos.group_map(head, z, "species")
    assert lab == ["H", "C", "O"] and gptr.tolist() == [0, 5, 18, 31] and perm.tolist() == list(range(13, 18)) + list(range(18, 31)) + list(range(13))
    perm, gptr, lab = dos.group_map(head, z, "shell")
    assert lab == [("O", 0, "s"), ("O", 0, "p"), ("O", 0, "d"), ("H", 1, "s"), ("H", 1, "p"), ("C", 2, "s"), ("C", 2, "p"), ("C", 2, "d")]
    assert gptr.tolist() == [0, 2, 8, 13, 15, 18, 20, 26, 31] and perm.tolist() == list(range(31))
    perm, gptr, lab = dos.group_map(head, z, None)
    assert lab == [] and gptr.tolist() == [0] and perm.size == 0 and perm.dtype == np.int32 and gptr.dtype == np.int32
    # two atoms of one species are one non-contiguous group
    perm, gptr, lab = dos.group_map(head, np.array([6, 1, 6]), "species")
    assert lab == ["H", "C"] and perm.tolist() == list(range(13, 18)) + list(range(13)) + list(range(18, 31))
    assert dos.padded_groups(0) == 16 and dos.padded_groups(15) == 16 and dos.padded_groups(16) == 32
    with pytest.raises(ValueError):
        dos.group_map(head, z, "orbital")


def test_fermi_level_sits_in_the_gap_of_a_gapped_spectrum():
    eps = np.concatenate([np.linspace(-5.0, -1.0, 8), np.linspace(2.0, 6.0, 8)])
    w = np.full(16, 1.0)
    mu = dos.fermi_level(eps, w, 16.0, 0.1, 2)                 # 8 doubly occupied states
    assert -1.0 < mu < 2.0 and abs(mu - 0.5) < 1e-3             # the plateau ends where the two edges' tails reach 1e-12 of the count: symmetric to rounding -> mid-gap
    mu1 = dos.fermi_level(eps, w, 8.0, 0.1, 1)
    assert abs(mu1 - mu) < 1e-9
    with pytest.raises(ValueError):
        dos.fermi_level(eps, w, 40.0, 0.1, 2)


def test_twins_against_fp64_and_the_torch_path():
    """the numpy twins of both kernels on the GPU tests' own cases: inside the same bounds; the torch path likewise"""
    assert DC.check_broaden_shapes(DC.dos_broaden_cpu, "cpu", 1153) <= 1.0
    assert DC.check_broaden_shapes(DC.dos_broaden_cpu, "cpu", 3) <= 1.0
    assert DC.check_broaden_structure(DC.dos_broaden_cpu, "cpu") and DC.check_broaden_structure(DC.dos_broaden_cpu, "cpu", Gp=80)
    assert DC.check_broaden_shapes(dos._broaden_torch, "cpu", 1153) <= 1.0
    for M in (1, 18, 31, 130):
        assert DC.check_mulliken(DC.mulliken_weights_cpu, "cpu", M) <= 1.0
    assert DC.check_mulliken(dos._mulliken_torch, "cpu", 31) <= 1.0


@pytest.mark.parametrize("projection,time_reversal,k_chunk", [("atom", True, None), ("species", False, 1), ("shell", True, 5), (None, True, None)])
def test_chain_after_the_solver_on_the_twins(monkeypatch, projection, time_reversal, k_chunk):
    DC.install_cpu(monkeypatch)
    r = DC.check_chain("cpu", projection, time_reversal, k_chunk)
    assert max(r.values()) <= 1.0, r


def test_chain_after_the_solver_on_the_torch_path():
    """CPU tensors take the torch path (nothing is patched): the same bounds; chunked and unchunked, TR-reduced and full grid all meet the fp64 DOS"""
    for args in (("shell", True, 5), ("species", False, None)):
        r = DC.check_chain("cpu", *args)
        assert max(r.values()) <= 1.0, r


def test_energy_grid_and_its_refusals():
    E0, dE = dos.energy_grid(None, 1000, 0.1, -3.0, 5.0)
    assert abs(E0 - (-3.8)) < 1e-12 and abs(dE - 9.6 / 999) < 1e-15
    assert dos.energy_grid((-1.0, 1.0), 21, 0.1) == (-1.0, 0.1)
    with pytest.raises(ValueError, match="grid step"):
        dos.energy_grid((-10.0, 10.0), 50, 0.1)
    with pytest.raises(ValueError):
        dos.energy_grid((1.0, 1.0), 50, 0.1)
    with pytest.raises(ValueError):
        dos.energy_grid(None, 1, 0.1, 0.0, 1.0)
