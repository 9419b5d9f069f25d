"""tools/gen_sym_table_digests.py -- TEST INFRASTRUCTURE ONLY.  Records SHA-256 digests of plan.sym_contraction_tables(irreps, correlation <= 3) as
data in tests/golden/sym_contraction_table_digests.json.  The committed file was written by this script on the commit BEFORE correlation 4 was added to the
planner; tests/test_corr4_cpu.py recomputes the digests, so any change to the bytes of a correlation <= 3 table shows.

Usage:  python tools/gen_sym_table_digests.py [output path]        (from the repo root)
        HG_DIGEST_ROOT=<checkout of another commit> python tools/gen_sym_table_digests.py      (digests of THAT commit's planner: how the committed file was made)
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("HG_DIGEST_ROOT", ROOT))

CASES = [("8x0e+4x0o+4x1o+2x1e+2x2o+3x2e+2x3o", 4, 1), ("8x0e+4x0o+4x1o+2x1e+2x2o+3x2e+2x3o", 4, 2), ("4x0e+2x0o+3x1o+2x1e+2x2e", 3, 1),
         ("4x0e+2x0o+3x1o+2x1e+2x2e", 3, 2), ("4x0e+2x0o+3x1o+2x1e+2x2e", 3, 3), ("4x0e+3x1o+2x2e", 16, 3), ("3x0e+2x0o+2x1o+2x1e", 3, 3)]


def digest(tab):
    """SHA-256 over the sorted keys of a table dict: arrays by dtype, shape and bytes, everything else by repr"""
    h = hashlib.sha256()
    for k in sorted(tab):
        v = tab[k]
        h.update(k.encode())
        if isinstance(v, np.ndarray):
            h.update(str((v.dtype.str, v.shape)).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


def compute():
    from hamgnn_amd import plan as P
    return {f"{irr}|{nh}|{corr}": digest(P.sym_contraction_tables(P.corr_hidden_irreps(irr, nh), corr)) for irr, nh, corr in CASES}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sym_contraction_table_digests.json")
    with open(out, "w") as f:
        json.dump(compute(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
