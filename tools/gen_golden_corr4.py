"""tools/gen_golden_corr4.py -- TEST INFRASTRUCTURE ONLY, build container only (needs the reference tree, like oracle/gen_golden.py whose stubs it uses).

Runs the reference's OWN CorrProductBlock(correlation=4) -- its MACE files executed unmodified from where they lie (oracle.gen_golden._load_real_mace) -- on
`4x0e+3x1o+2x2e` with 4 hidden channels and 3 elements in fp64 and writes {weights, inputs, outputs, meta} as data to
    tests/golden/corr_product_block_nu4.npz
Parameters only: the U matrices (buffers of the reference's contractions, 10^4 - 10^5 dense values per target at this order) are NOT stored -- the planner's
own tables have to reproduce the outputs.  At correlation 4 -- and at no other order -- the reference's U_matrix_real filters every coupling result to the
natural-parity irreps (cg.py:99-114), which oracle/mace_ref.py does not restate: its order-4 contraction has 55 / 124 / 148 paths per target where the
reference has 46 / 76 / 85, so the oracle block cannot take this state dict.  The script therefore ASSERTS what it can on the spot: the reference's U
matrices of order 1 ... 3 equal the oracle's, and its dense U_4 equals the planner's sparse nu = 4 table (plan.SYM4_FILTER_IR_MID) entry for entry.
One element has no node.

Usage:  python tools/gen_golden_corr4.py        (from the repo root; regenerates the file byte-identically)
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hamgnn_amd import plan as P  # noqa: E402
from oracle import e3, gen_golden as GG, mace_ref as M  # noqa: E402
from tools.gen_golden_kan import write_npz  # noqa: E402

IRREPS, HIDDEN, ELEMENTS, N = "4x0e+3x1o+2x2e", 4, 3, 7


def main():
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(1)
    GG.install_stubs()
    ref_ib = importlib.import_module("hamgnn.nn.interaction_blocks")
    real = GG._load_real_mace()
    ref_ib.EquivariantProductBasisBlock, ref_ib.reshape_irreps = real["blocks"].EquivariantProductBasisBlock, real["irreps_tools"].reshape_irreps
    torch.manual_seed(41)
    ref = ref_ib.CorrProductBlock(irreps_node_feats=e3.Irreps(IRREPS), num_hidden_features=HIDDEN, correlation=4, num_elements=ELEMENTS,
                                  use_skip_connections=True)
    mine = M.CorrProductBlock(IRREPS, HIDDEN, 3, ELEMENTS, True)           # (orders 1 ... 3 of the restatement)
    sd = dict(ref.state_dict())
    params = {k for k, _ in ref.named_parameters()}
    tab = P.sym_contraction_tables(P.corr_hidden_irreps(IRREPS, HIDDEN), 4)
    o = kg = 0
    for k, cm in enumerate(mine.prod.symmetric_contractions.contractions):
        cr = ref.prod.symmetric_contractions.contractions[k]
        for nu in (1, 2, 3):
            GG._check(cm.U(nu), cr.U_tensors(nu), f"U_matrix_{nu} of target {k} (correlation 4)", tol=1e-12)
        U4 = cr.U_tensors(4).numpy()
        U4 = U4 if U4.ndim == 6 else U4[None]                                 # [w, ell x 4, paths]
        assert U4.shape[-1] == tab["K4"][k], (U4.shape, tab["K4"])
        D = np.zeros(U4.shape)
        for w in range(U4.shape[0]):
            e = tab["ent4"][tab["ptr4"][o]:tab["ptr4"][o + 1]]
            np.add.at(D[w], (e[:, 0], e[:, 1], e[:, 2], e[:, 3], e[:, 4] - kg), np.ascontiguousarray(e[:, 5]).view(np.float32).astype(np.float64))
            o += 1
        kg += tab["K4"][k]
        GG._check(torch.from_numpy(D), torch.from_numpy(U4), f"planner's sparse nu = 4 table of target {k} vs the reference's U_matrix_4", tol=1e-6)
    gen = torch.Generator().manual_seed(42)
    x = torch.randn(N, e3.Irreps(IRREPS).dim, generator=gen)
    z = torch.tensor([2, 0, 0, 2, 0, 0, 0])[:N]
    onehot = torch.nn.functional.one_hot(z, ELEMENTS).to(x.dtype)
    gd = {"node_features": x.clone(), "node_attrs": onehot}
    ref(gd)
    flat = {}
    for group, d in dict(weights={k: v for k, v in sd.items() if k in params}, inputs=dict(node_features=x, z=z), outputs=dict(node_features=gd["node_features"]),
                         meta=dict(irreps=np.array(IRREPS), num_hidden=np.array(HIDDEN), num_elements=np.array(ELEMENTS), correlation=np.array(4),
                                   K4=np.array(tab["K4"]))).items():
        flat.update({f"{group}/{k}": v for k, v in GG._np(d).items()})
    assert not any("U_matrix" in k for k in flat)
    path = os.path.join(GG.GOLD, "corr_product_block_nu4.npz")
    size = write_npz(path, flat)
    assert size < (1 << 20), size
    print(f"  wrote tests/golden/{os.path.basename(path)}  ({size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
