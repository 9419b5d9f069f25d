"""The DOS kernels on the GPU: hg_dos_broaden and hg_mulliken_weights (csrc/spectra.hip) alone against fp64, the torch path against the kernel, and the chain
weights -> sort -> broadening in chunks (hamgnn_amd/dos.py) on exact eigenpairs of the fixture crystals of tests/golden/band_energies_openmx_13.npz (M = 18
and 31), which tests/dos_checks.py computes on the host in complex128.  The bounds are stated there.  Measured ratios: profiles/dos.md."""
import numpy as np
import pytest
import torch

from tests import dos_checks as DC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ns", [1, 3, 4, 1153])
def test_dos_broaden_kernel_vs_fp64(ns):
    """every ne in {1, 16, 37} x Gp in {1, 16, 17, 70, 80}: |D - D_ref| <= (K + 64) 2^-24 T + tau per element"""
    from hamgnn_amd import ops
    assert DC.check_broaden_shapes(ops.dos_broaden, "cuda", ns) <= 1.0


@pytest.mark.parametrize("Gp", [17, 80])
def test_dos_broaden_kernel_windows_accumulate_and_reproducibility(Gp):
    """both instantiations (Gp = 17: element loads, Gp = 80: 16-byte loads, two slabs, the second partly filled): a hole wider than 12 sigma (empty windows write zeros / leave D alone), 40 equal eigenvalues, states entirely below and above the grid, accumulate = 1
    == the sum of two writes, two launches 0.0 apart"""
    from hamgnn_amd import ops
    assert DC.check_broaden_structure(ops.dos_broaden, "cuda", Gp=Gp)


def test_dos_broaden_refuses_bad_arguments():
    from hamgnn_amd import ops
    eps, W = torch.zeros(4, device="cuda"), torch.zeros(4, 3, device="cuda")
    with pytest.raises(RuntimeError, match="hg_dos_broaden"):
        ops.dos_broaden(eps, W, 0.0, 0.1, 8, 0.0)
    with pytest.raises(ValueError):
        ops.dos_broaden(eps.double(), W, 0.0, 0.1, 8, 0.1)
    with pytest.raises(ValueError):
        ops.dos_broaden(eps, W, 0.0, 0.1, 8, 0.1, accumulate=True)


@pytest.mark.parametrize("M", [1, 18, 31, 130])
def test_mulliken_weights_kernel_vs_fp64(M):
    """groups of size 1, one group of everything, non-contiguous groups, G = 0; padded and unpadded Gp: (m_g + 4) 2^-24 sum |terms|; pad columns 0, column 0 == wk"""
    from hamgnn_amd import ops
    assert DC.check_mulliken(ops.mulliken_weights, "cuda", M) <= 1.0


@pytest.mark.parametrize("projection", ["atom", "species", "shell"])
@pytest.mark.parametrize("time_reversal", [True, False])
@pytest.mark.parametrize("k_chunk", [1, None])
def test_chain_after_the_solver(projection, time_reversal, k_chunk):
    """4 x 4 x 4 on both fixture crystals, exact eigenpairs from the host: (a) the broadening of the device's own weight rows vs fp64, (b) vs the fp64 DOS / PDOS,
    (c) the sum rules"""
    r = DC.check_chain("cuda", projection, time_reversal, k_chunk)
    assert max(r.values()) <= 1.0, r


def test_torch_path_vs_kernels(monkeypatch):
    """HG_DOS=torch: the same chain on torch ops meets the same bounds; exp + matmul vs the kernel on the same states within twice the kernel's bound"""
    assert DC.check_torch_vs_kernel("cuda") <= 1.0
    monkeypatch.setenv("HG_DOS", "torch")
    r = DC.check_chain("cuda", "shell", True, 7)
    assert max(r.values()) <= 1.0, r
