"""Checks of the correlation-4 CorrProductBlock shared by tests/test_corr4_cpu.py (ops replaced by the stand-ins of tests/cpu_ops_corr.py) and
tests/test_corr4_gpu.py (the HIP kernels of csrc/sym_contraction.hip): forward and every gradient against the fp64 oracle (oracle/mace_ref.py) and
torch.autograd through it.  The oracle blocks are built once per (irreps, hidden channels) -- its dense U_4 takes seconds -- and never modified."""
import contextlib
import functools

import numpy as np
import torch

from tests import gpu_checks as G

IRREPS = ("4x0e+3x1o+2x2e", "3x0e+2x0o+2x1o+2x1e")       # 9 / 8 coupling components: 32 625 / 7 888 non-zero U_4 entries
NEL = 3                                                   # three elements; the checks leave element 1 without a node


@contextlib.contextmanager
def oracle_enumeration():
    """The oracle enumerates the order-4 couplings without the reference's natural-parity filter (oracle/mace_ref.py:wigner_nj; the reference: cg.py:99-114,
    plan.SYM4_FILTER_IR_MID): a comparison with it plans the nu = 4 table the same way.  Same kernels, same host code, a longer path list (55 / 124 / 148
    instead of 46 / 76 / 85 on IRREPS[0]) and targets of either parity; the filtered default is pinned by the reference's own fixture."""
    from hamgnn_amd.plan import tables
    prev = tables.SYM4_FILTER_IR_MID
    tables.SYM4_FILTER_IR_MID = None
    try:
        yield
    finally:
        tables.SYM4_FILTER_IR_MID = prev


@functools.lru_cache(maxsize=None)
def oracle_block(irr, nh, correlation=4, nel=NEL, seed=0):
    from oracle import mace_ref as M
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(1000 + seed)
        blk = M.CorrProductBlock(irr, nh, correlation, nel, True)
    finally:
        torch.set_default_dtype(prev)
    return blk


def product_block(blk, irr, nh, correlation=4, nel=NEL):
    from hamgnn_amd import nn as hnn
    return G.load_weights(hnn.CorrProductBlock(irr, nh, correlation, nel, True), {k: v.detach().clone() for k, v in blk.named_parameters()})


def block_inputs(irr, N, doped, seed, nel=NEL):
    from oracle.e3 import Irreps
    gen = torch.Generator().manual_seed(77 + seed)
    x = torch.randn(N, Irreps(irr).dim, generator=gen, dtype=torch.float64)
    z = torch.tensor([0, nel - 1])[torch.randint(0, 2, (N,), generator=gen)]        # element 1 absent: its node group is empty
    delta = 0.3 * torch.randn(N, nel, generator=gen, dtype=torch.float64) if doped else None
    g = torch.randn(N, Irreps(irr).dim, generator=gen, dtype=torch.float64)
    return x, z, delta, g


def run_product(m, irr, x, z, delta, g, device):
    """forward rows, gradient of the node rows and the parameter-gradient dict of the product block, back in the reference's column order"""
    from hamgnn_amd import ops, plan as P
    lay = P.PlanarLayout(irr)
    imap = torch.from_numpy(lay.index_map().astype(np.int32)).to(device)
    xp = ops.to_planar(x.float().to(device), imap, lay.dim)
    gp = ops.to_planar(g.float().to(device), imap, lay.dim)
    zd, dd = z.to(device), (None if delta is None else delta.float().to(device))
    m.compile(device)
    y = ops.from_planar(m(xp, zd, dd), imap)
    g_node, grads = m.backward(xp, zd, gp, dd)
    return y, ops.from_planar(g_node, imap), grads


def _err(got, want):
    want = want.detach().double().cpu()
    got = got.detach().double().cpu().reshape(want.shape)
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-6)


def check_block(device, irr, nh, N, doped=False, seed=0, correlation=4):
    """product block (forward + backward) vs the oracle block and autograd through it; errors relative to the largest reference value of each tensor"""
    blk = oracle_block(irr, nh, correlation)
    for p in blk.parameters():
        p.grad = None
    x, z, delta, g = block_inputs(irr, N, doped, seed)
    xr = x.clone().requires_grad_()
    attrs = torch.nn.functional.one_hot(z, NEL).double()
    if doped:
        attrs = (attrs + delta).requires_grad_()
    yr = blk(xr, attrs)
    (yr * g).sum().backward()
    m = product_block(blk, irr, nh, correlation)
    y, g_node, grads = run_product(m, irr, x, z, delta, g, device)
    errs = {"forward": _err(y, yr), "g_node": _err(g_node, xr.grad)}
    if doped:
        errs["g_delta"] = _err(grads.pop("_g_delta"), attrs.grad)
    names = dict(blk.named_parameters())
    assert set(grads) == set(names), sorted(set(grads) ^ set(names))
    for k, v in grads.items():
        errs[k] = _err(v, names[k].grad)
    worst = max(errs, key=errs.get)
    return {"N": N, "max_rel_err": errs[worst], "worst": worst, "n": len(errs), "forward": errs["forward"]}


def check_two_launches(device, irr, nh, N, doped):
    """two identical launches of the forward and of the adjoint: largest absolute difference (bit-equal runs give 0.0)"""
    blk = oracle_block(irr, nh)
    x, z, delta, g = block_inputs(irr, N, doped, 5)
    m = product_block(blk, irr, nh)
    a, b = run_product(m, irr, x, z, delta, g, device), run_product(m, irr, x, z, delta, g, device)
    d = [float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())]
    d += [float((a[2][k] - b[2][k]).abs().max()) for k in a[2]]
    return max(d)


def check_generic_vs_default(device, name, monkeypatch):
    """HG_CORR_KERNEL=nu against the default kernels on a reference fixture's block (correlation 2 / 3 / 1): forward rows, node gradient and every
    parameter gradient of the two routes against each other"""
    from hamgnn_amd import nn as hnn
    f = G.load(name)
    irr, nh, nel = str(f["meta"]["irreps"]), int(f["meta"]["num_hidden"]), int(f["meta"]["num_elements"])
    corr = int(f["meta"]["correlation"]) if "correlation" in f["meta"] else 2
    m = G.load_weights(hnn.CorrProductBlock(irr, nh, corr, nel, True), f["weights"])
    x = torch.from_numpy(f["inputs"]["node_features"]).double()
    z = torch.from_numpy(f["inputs"]["z"])
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    monkeypatch.delenv("HG_CORR_KERNEL", raising=False)
    ref = run_product(m, irr, x, z, None, g, device)
    monkeypatch.setenv("HG_CORR_KERNEL", "nu")
    got = run_product(m, irr, x, z, None, g, device)
    errs = {"forward": _err(got[0], ref[0]), "g_node": _err(got[1], ref[1])}
    errs.update({k: _err(got[2][k], ref[2][k]) for k in ref[2]})
    worst = max(errs, key=errs.get)
    return {"max_rel_err": errs[worst], "worst": worst, "correlation": corr}
