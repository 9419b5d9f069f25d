"""Register budget of `tp_is_two_kernel<SPLIT>` (csrc/tp_is.hip: the edge kernel of programs with phases that use both radial generators, a second set of hidden rows
resident): two waves per SIMD as the default kernel, so at most 256 VGPRs, no spills, no scratch -- read from the compiler's metadata as tests/test_isa_audit.py does."""
import os
import shutil

import pytest

from tests import isa_audit as A

pytestmark = pytest.mark.skipif(not os.path.exists(A.HIPCC) and shutil.which("hipcc") is None, reason="hipcc not found")

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hamgnn_amd", "csrc")


def test_two_generator_kernels_register_budget_and_no_scratch():
    ks = [k for k in A.audit(os.path.join(CSRC, "tp_is.hip")) if "tp_is_two_kernel" in k["name"]]
    assert len(ks) == 2                                         # <SPLIT> in {false, true}
    for k in ks:
        m = k["meta"]
        print(k["name"], m)
        assert m["vgpr_spills"] == 0 and m["scratch"] == 0 and m["vgprs"] <= 256, (k["name"], m)
