"""CPU stand-ins for the order-generic symmetric-contraction entry points (ops.sym_contraction_nu / sym_contraction_nu_backward, csrc/sym_contraction.hip)
-- TEST INFRASTRUCTURE in the style of tests/cpu_ops.py, never shipped.  They consume EXACTLY the tables the product hands to the kernels: the forward
the nu-th CSR entry list of plan.sym_contraction_tables, the adjoint the two transposed tables of plan.sym_contraction_adjoint_tables (by component and
by kappa), in float64.  `install(monkeypatch)` = cpu_ops.install + these two."""
import numpy as np
import torch

from hamgnn_amd import ops
from tests import cpu_ops


def _tab_np(tab):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in tab.items() if not str(k).startswith("_")}


def _vals(col):
    return np.ascontiguousarray(col).view(np.float32).astype(np.float64)


def contraction_nu_np(tab, nu, hp, z, W, C, out):
    """numpy twin of hg_sym_contraction_nu: ADDS the term of order nu to the planar rows `out` [N, Dp] (float64 copy returned)"""
    out = np.array(out, dtype=np.float64)
    x = np.stack([hp[:, tab["ell_off"] + c] for c in range(C)], axis=1).astype(np.float64)     # [N, C, num_ell]
    ent, ptr = tab[f"ent{nu}"], tab[f"ptr{nu}"]
    val = _vals(ent[:, -1])
    for o in range(tab["nout"]):
        e = slice(ptr[o], ptr[o + 1])
        if e.stop == e.start:
            continue
        t = val[e][None, None, :] * np.transpose(W[z][:, ent[e, nu], :], (0, 2, 1))
        for f in range(nu):
            t = t * x[:, :, ent[e, f]]
        out[:, tab["out_off"][o] + np.arange(C)] += t.sum(-1)
    return out


def contraction_nu_backward_np(tab, nu, hp, z, W, C, gp, per_node):
    """numpy twin of hg_sym_contraction_nu_backward on the transposed tables: (g_h [N, Dp], g_W like W)"""
    N = hp.shape[0]
    x = np.stack([hp[:, tab["ell_off"] + c] for c in range(C)], axis=1).astype(np.float64)     # [N, C, num_ell]
    gx = np.stack([gp[:, tab["out_off"] + c] for c in range(C)], axis=1).astype(np.float64)    # [N, C, nout]
    g_h = np.zeros(hp.shape, dtype=np.float64)
    entH, ptrH = tab[f"entH{nu}"], tab[f"ptrH{nu}"]
    valH = _vals(entH[:, nu + 1])
    for i in range(tab["num_ell"]):
        e = slice(ptrH[i], ptrH[i + 1])
        if e.stop == e.start:
            continue
        t = valH[e][None, None, :] * np.transpose(W[z][:, entH[e, nu], :], (0, 2, 1)) * gx[:, :, entH[e, 0]]
        for f in range(nu - 1):
            t = t * x[:, :, entH[e, 1 + f]]
        g_h[:, tab["ell_off"][i] + np.arange(C)] += t.sum(-1)
    entW, ptrW = tab[f"entW{nu}"], tab[f"ptrW{nu}"]
    valW = _vals(entW[:, nu + 1])
    K = W.shape[1]
    per = np.zeros((N, K, C), dtype=np.float64)
    ch = np.arange(C)
    for kap in range(K):
        e = slice(ptrW[kap], ptrW[kap + 1])
        if e.stop == e.start:
            continue
        t = valW[e][None, :, None] * gp[:, entW[e, 0][:, None] + ch[None, :]]                   # [N, rows, C]
        for f in range(nu):
            t = t * hp[:, entW[e, 1 + f][:, None] + ch[None, :]]
        per[:, kap, :] = t.sum(1)
    if per_node:
        return g_h, per
    g_W = np.zeros(W.shape, dtype=np.float64)
    np.add.at(g_W, z, per)
    return g_h, g_W


def sym_contraction_nu(nu, h, z, C, tab, W, out):
    out.copy_(cpu_ops._t(contraction_nu_np(_tab_np(tab), nu, cpu_ops._np(h), z.cpu().numpy(), cpu_ops._np(W), C, cpu_ops._np(out))))
    return out


def sym_contraction_nu_backward(nu, h, z, C, tab, W, g_out, g_h, per_node=False):
    gh, gW = contraction_nu_backward_np(_tab_np(tab), nu, cpu_ops._np(h), z.cpu().numpy(), cpu_ops._np(W), C, cpu_ops._np(g_out), per_node)
    g_h += cpu_ops._t(gh)
    return cpu_ops._t(gW)


def install(mp):
    """cpu_ops.install + the stand-ins above"""
    cpu_ops.install(mp)
    mp.setattr(ops, "sym_contraction_nu", sym_contraction_nu)
    mp.setattr(ops, "sym_contraction_nu_backward", sym_contraction_nu_backward)
