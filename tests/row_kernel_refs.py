"""fp64 twins of the row-streaming entry points of csrc/row_ops.hip, csrc/attention.hip and csrc/head.hip -- TEST INFRASTRUCTURE.

One function per entry point, float64 in and out, written from the operation's definition (the reference lines each kernel's comment cites and the
docstrings of hamgnn_amd/ops.py), not from the kernels and not from tests/cpu_ops.py (never imported here: tests/test_row_kernels_cpu.py puts the two side by
side).  Every twin that sums returns (value, scale) with scale = the sum of the absolute values of the terms of that sum: the error scale of
tests/row_kernel_checks.py:compare.  The gate twin reads the UNCOMPACTED [Dout][4] table of plan.gate_tables, so plan.gate_tables_compact is under test as
well; the backward twins are torch.autograd.grad through the forward twin.  The `defect=` keyword of a twin exists for the sharpness tests only: it names
one deliberate error, and the comparison has to reject the result."""
import math

import numpy as np
import torch

LN2 = math.log(2.0)
F64 = torch.float64


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().to(F64)


def _l(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().long()


# ------------------------------------------------------------------------------------------------ segmented node scatter
def segment_sum(msg, rowptr, perm, defect=None):
    """out[n] = sum of msg[perm[q]] over rowptr[n] <= q < rowptr[n + 1] (torch_scatter.scatter(..., reduce='sum') over the receiver CSR)"""
    msg, rowptr, perm = _d(msg), _l(rowptr), _l(perm)
    N = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    seg = torch.repeat_interleave(torch.arange(N), deg)
    rows = msg[perm[:int(rowptr[-1])]]
    if defect == "drop_tail_edge":                             # the last edge of every segment whose degree is not a multiple of 4
        last = torch.zeros(rows.shape[0], dtype=torch.bool)
        sel = (deg % 4 != 0)
        last[(rowptr[1:] - 1)[sel]] = True
        rows = rows * (~last)[:, None]
    out = torch.zeros(N, msg.shape[1], dtype=F64).index_add_(0, seg, rows)
    scale = torch.zeros(N, msg.shape[1], dtype=F64).index_add_(0, seg, rows.abs())
    return out, scale


# ------------------------------------------------------------------------------------------------ gate
def act(x, aid, consts):
    """activations of the e3nn Gate as the reference normalises them (e3nn normalize2mom constants in plan.ACT_CONSTS): 1 shifted softplus, 2 tanh, 3 silu,
    4 abs, 0 identity"""
    c = float(consts[aid])
    if aid == 1:
        return c * (torch.nn.functional.softplus(x, threshold=1e9) - LN2)
    if aid == 2:
        return c * torch.tanh(x)
    if aid == 3:
        return c * x * torch.sigmoid(x)
    if aid == 4:
        return c * x.abs()
    assert aid == 0
    return x


def gate(x, tab4, consts, defect=None):
    """e3nn Gate on planar rows from plan.gate_tables' table {source column | -1, its activation, gate column | -1, the gate's activation}:
    out[p] = act(x[src]) * gate_act(x[gate]).  A product, no sum: the scale is |out|."""
    x = x if x.requires_grad else _d(x)
    tab4 = np.asarray(tab4)
    cols = []
    for src, a, g, ga in (tuple(int(v) for v in r) for r in tab4):
        if src < 0:
            cols.append(torch.zeros_like(x[:, 0]))
            continue
        v = act(x[:, src], a, consts)
        if g >= 0:
            if defect == "gate_act_wrong_id":                  # the gate channel's activation with another id
                ga = 2 if ga != 2 else 1
            v = v * act(x[:, g], ga, consts)
        cols.append(v)
    return torch.stack(cols, 1)


def gate_backward(x, gy, tab4, consts):
    """gx = J^T gy by autograd through gate(); scale = |J|^T |gy|, written out from the two kinds of terms (through the source, through the gate)"""
    x, gy = _d(x), _d(gy)
    with torch.enable_grad():
        xr = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad(gate(xr, tab4, consts), xr, grad_outputs=gy)

    def dact(col, aid):
        with torch.enable_grad():
            c = col.clone().requires_grad_()
            (d,) = torch.autograd.grad(act(c, aid, consts).sum(), c)
        return d
    scale = torch.zeros_like(x)
    for p, (src, a, g, ga) in enumerate(tuple(int(v) for v in r) for r in np.asarray(tab4)):
        if src < 0:
            continue
        gv = act(x[:, g], ga, consts) if g >= 0 else torch.ones_like(x[:, 0])
        scale[:, src] += (gy[:, p] * dact(x[:, src], a) * gv).abs()
        if g >= 0:
            scale[:, g] += (gy[:, p] * act(x[:, src], a, consts) * dact(x[:, g], ga)).abs()
    return gx, scale


# ------------------------------------------------------------------------------------------------ norm activation
def _chan_cols(chan_tab):
    """plan.norm_act_table rows {offset, stride | components << 16} -> list of column lists, one per irrep copy"""
    return [[int(off) + a * (int(w) & 0xffff) for a in range(int(w) >> 16)] for off, w in np.asarray(chan_tab)]


def norm_act(x, chan_tab, eps=1e-8, defect=None):
    """e3nn NormActivation(ssp, normalize=True, epsilon=eps, bias=False): every irrep copy is scaled by ssp(n) / n, n = sqrt(max(sum_a x_a^2, eps^2));
    columns without a table entry (channel padding) are 0.  Element-wise up to the norm (a sum of squares: no cancellation): the scale is |out|."""
    x = x if x.requires_grad else _d(x)
    out = torch.zeros_like(x)
    for cols in _chan_cols(chan_tab):
        v = x[:, cols]
        n2 = (v * v).sum(1)
        if defect != "no_clamp":
            n2 = torch.clamp(n2, min=eps * eps)
        n = torch.sqrt(n2)
        sc = (torch.nn.functional.softplus(n, threshold=1e9) - LN2) / n     # (n >= eps > 0; without the clamp an all-zero copy is 0 / 0)
        out[:, cols] = v * sc[:, None]
    return out


def norm_act_backward(x, gy, chan_tab, eps=1e-8):
    """autograd through norm_act (below the clamp the norm is a constant, as torch.clamp differentiates it); scale: |ssp/n gy_a| + |x_a| sum_b |gy_b x_b| |k|,
    k = (sigmoid(n) - ssp(n)/n) / n^2 above the clamp, 0 below"""
    x, gy = _d(x), _d(gy)
    with torch.enable_grad():
        xr = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad(norm_act(xr, chan_tab, eps), xr, grad_outputs=gy)
    scale = torch.zeros_like(x)
    for cols in _chan_cols(chan_tab):
        v, g = x[:, cols], gy[:, cols]
        n2 = (v * v).sum(1)
        clamped = n2 < eps * eps
        n = torch.sqrt(torch.clamp(n2, min=eps * eps))
        sc = (torch.nn.functional.softplus(n, threshold=1e9) - LN2) / n
        k = torch.where(clamped, torch.zeros_like(n), (torch.sigmoid(n) - sc).abs() / n ** 2)
        scale[:, cols] = (sc[:, None] * g).abs() + v.abs() * ((g * v).abs().sum(1) * k)[:, None]
    return gx, scale


def norm_classes(x, chan_tab, eps=1e-8):
    """[rows, nchan] fp64 norms (unclamped) of every irrep copy: what the coverage conditions of the norm-activation cases count"""
    x = _d(x)
    return torch.stack([(x[:, cols] ** 2).sum(1).sqrt() for cols in _chan_cols(chan_tab)], 1)


# ------------------------------------------------------------------------------------------------ adds, layout, embedding
def add_rows(a, b, c=None):
    out = _d(a) + _d(b)
    return out if c is None else out + _d(c)


def to_planar(x, imap, Dp):
    """e3nn (irrep-major) columns -> planar columns; planar columns no e3nn column maps to are 0"""
    x = _d(x)
    out = torch.zeros(x.shape[0], Dp, dtype=F64)
    out[:, _l(imap)] = x
    return out


def from_planar(xp, imap):
    """planar -> e3nn columns; map entry -1: structural zero"""
    xp, m = _d(xp), _l(imap)
    out = xp[:, m.clamp(min=0)].clone()
    out[:, m < 0] = 0.0
    return out


def embed_lookup(Ta, Tb, z, idx_a, idx_b, rows, T, Tp):
    """out[r, :T] = Ta[z[idx_a[r]]] (+ Tb[z[idx_b[r]]]); an absent index list is the identity; columns T..Tp are padding zeros"""
    Ta, Tb, z = _d(Ta), _d(Tb), _l(z)
    r = torch.arange(rows)
    out = torch.zeros(rows, Tp, dtype=F64)
    out[:, :T] = Ta[z[r if idx_a is None else _l(idx_a)]][:, :T]
    if Tb is not None:
        out[:, :T] += Tb[z[r if idx_b is None else _l(idx_b)]][:, :T]
    return out


# ------------------------------------------------------------------------------------------------ attention
def soft_cut(length, cut_param, cutoff):
    """e3nn soft_unit_step(cut_param (1 - r / r_cut)): exp(-1 / x) for x > 0, else 0 (hamgnn/utils/cutoff_functions.py:65-100)"""
    x = float(cut_param) * (1.0 - _d(length) / float(cutoff))
    return torch.where(x > 0, torch.exp(-1.0 / torch.where(x > 0, x, torch.ones_like(x))), torch.zeros_like(x))


def _head_matrix(head_tab, H):
    ht = _l(head_tab)
    M = torch.zeros(ht.numel(), H, dtype=F64)
    cols = torch.nonzero(ht >= 0).reshape(-1)
    M[cols, ht[cols]] = 1.0
    return M


def attn_logits(K, src, dst, length, head_tab, H, head_dim, cut_param, cutoff, defect=None):
    """logits[e, h] = cut(|r_e|) / sqrt(head_dim) <K[dst_e] | K[src_e]>_h (hamgnn/nn/attention.py:126-140, 339-340); scale: the same with |products|"""
    K, M = _d(K), _head_matrix(head_tab, H)
    if defect == "swap_heads" and H > 1:
        M = M[:, [1, 0] + list(range(2, H))]
    prod = K[_l(src)] * K[_l(dst)]
    w = (soft_cut(length, cut_param, cutoff) / math.sqrt(head_dim))[:, None]
    return w * (prod @ M), w * (prod.abs() @ M)


def attn_aggregate(logits, V, rowptr, perm, head_tab, H, defect=None):
    """torch_geometric.utils.softmax of the logits over the edges into each node (max-shifted, sum + 1e-16), then out[n, col] = sum_e w[e, head(col)] V[e, col]
    (hamgnn/nn/attention.py:141-164); padding columns (head -1) are 0.  scale: sum_e w |V|."""
    logits, V, rowptr, perm = _d(logits), _d(V), _l(rowptr), _l(perm)
    N, M = rowptr.numel() - 1, _head_matrix(head_tab, H)
    out, scale = torch.zeros(N, V.shape[1], dtype=F64), torch.zeros(N, V.shape[1], dtype=F64)
    for n in range(N):
        e = perm[int(rowptr[n]):int(rowptr[n + 1])]
        if e.numel() == 0:
            continue
        lg = logits[e]
        if defect == "softmax_first_chunk":                    # statistics over the first 128 edges only
            st = lg[:128]
            w = torch.exp(lg - st.max(0).values) / (torch.exp(st - st.max(0).values).sum(0) + 1e-16)
        else:
            ex = torch.exp(lg - lg.max(0).values)
            w = ex / (ex.sum(0) + 1e-16)
        wc = w @ M.t()
        out[n] = (wc * V[e]).sum(0)
        scale[n] = (wc * V[e].abs()).sum(0)
    return out, scale


# ------------------------------------------------------------------------------------------------ read-out head
def ham_merge(coeff, wig, wig_off, slot_tab, cg_ptr, cg_idx, cg_val, nout):
    """merge_tensor_components + reorder_matrix (hamgnn_output.py:851-891, 1056-1096) as the planner folds them into tables: slot q = component a of a ham
    irrep L at planar base / stride, taken back to the global frame with D^L(e)^T when Wigner rows are given (coef[q] = sum_m D^L[m, a] c[base + m stride]);
    raw[p] = sum_k val[k] coef[idx[k]] over the CSR row of p.  wig: [rows, nW] packed row-major blocks at wig_off[L]."""
    c, D = _d(coeff), _d(wig)
    st, ptr, idx, val = np.asarray(slot_tab), np.asarray(cg_ptr), _l(cg_idx), _d(cg_val)
    rows = c.shape[0]
    coef, cabs = torch.zeros(rows, st.shape[0], dtype=F64), torch.zeros(rows, st.shape[0], dtype=F64)
    for q, (L, a, base, stride) in enumerate(tuple(int(v) for v in r) for r in st):
        if D is None:
            coef[:, q] = c[:, base + a * stride]
            cabs[:, q] = coef[:, q].abs()
        else:
            n = 2 * L + 1
            Dl = D[:, int(wig_off[L]):int(wig_off[L]) + n * n].reshape(rows, n, n)[:, :, a]
            cc = c[:, base + torch.arange(n) * stride]
            coef[:, q] = (Dl * cc).sum(1)
            cabs[:, q] = (Dl * cc).abs().sum(1)
    raw, scale = torch.zeros(rows, nout, dtype=F64), torch.zeros(rows, nout, dtype=F64)
    for p in range(nout):
        k = slice(int(ptr[p]), int(ptr[p + 1]))
        raw[:, p] = coef[:, idx[k]] @ val[k]
        scale[:, p] = cabs[:, idx[k]] @ val[k].abs()
    return raw, scale


def ham_finish(raw, raw_scale, inv, H0, orb_mask, z, idx_a, idx_b, nao, sign=1.0, symmetrize=True, h0_after_mask=False, defect=None):
    """H = mask (0.5 (raw[e] + sign raw[inv e]^T) + H0), or mask (...) + H0 with h0_after_mask (hamgnn_output.py:1231-1285, 2288-2365, 3603-3609,
    3782-3795); mask[r, c] = orb_mask[z[a_e], r mod w] orb_mask[z[b_e], c mod w] (the su2 wrap :3163-3168); absent inv / idx: the row itself"""
    raw, sc = _d(raw), _d(raw_scale)
    rows = raw.shape[0]
    H, S = raw[:, :nao * nao].reshape(rows, nao, nao), sc[:, :nao * nao].reshape(rows, nao, nao)
    if defect == "ignore_sign":
        sign = 1.0
    if symmetrize:
        iv = torch.arange(rows) if inv is None else _l(inv)
        Ho, So = H[iv], S[iv]
        if defect != "no_transpose":
            Ho, So = Ho.transpose(1, 2), So.transpose(1, 2)
        H, S = 0.5 * (H + sign * Ho), 0.5 * (S + So)
    h0 = None if H0 is None else _d(H0).reshape(rows, nao, nao)
    after = h0_after_mask if defect != "h0_wrong_side" else not h0_after_mask
    if h0 is not None and not after:
        H, S = H + h0, S + h0.abs()
    if orb_mask is not None:
        om, zz = _d(orb_mask), _l(z)
        w = om.shape[1]
        r = torch.arange(rows)
        ma = om[zz[r if idx_a is None else _l(idx_a)]].repeat(1, nao // w)
        mb = om[zz[r if idx_b is None else _l(idx_b)]].repeat(1, nao // w)
        m = ma[:, :, None] * mb[:, None, :]
        H, S = H * m, S * m
    if h0 is not None and after:
        H, S = H + h0, S + h0.abs()
    return H.reshape(rows, nao * nao), S.reshape(rows, nao * nao)


def pairs_to_inv(pairs, rows):
    """(pair_a, pair_b) row lists of hg_ham_readout -> the partner of every row (a self-paired row is its own partner); None: every row pairs with itself"""
    inv = torch.arange(rows)
    if pairs is not None and pairs[0] is not None:
        pa, pb = _l(pairs[0]), _l(pairs[1])
        inv[pa], inv[pb] = pb, pa
    return inv


def ham_readout(coeff, wig, wig_off, slot_tab, cg_ptr, cg_idx, cg_val, nao, pairs, H0, orb_mask, z, idx_a, idx_b, sign=1.0, symmetrize=True,
                h0_after_mask=False, defect=None):
    """the one-pass read-out = ham_merge then ham_finish with the partner rows given as pairs"""
    raw, sc = ham_merge(coeff, wig, wig_off, slot_tab, cg_ptr, cg_idx, cg_val, nao * nao)
    return ham_finish(raw, sc, pairs_to_inv(pairs, raw.shape[0]), H0, orb_mask, z, idx_a, idx_b, nao, sign, symmetrize, h0_after_mask, defect=defect)


def block_mean(x, tab, nao, defect=None):
    """symmetrize_orbital_coefficients (hamgnn_output.py:2367-2431): every element -> the mean over its (row shell, col shell) block tab[q] = {r0, r1, c0, c1}"""
    X = _d(x)[:, :nao * nao].reshape(-1, nao, nao)
    out, scale = torch.zeros_like(X), torch.zeros_like(X)
    tab = np.asarray(tab)
    if defect == "wrong_shell":                                # the column shell taken for the rows as well
        tab = np.stack([tab[:, 2], tab[:, 3], tab[:, 2], tab[:, 3]], 1)
    for q, (r0, r1, c0, c1) in enumerate(tuple(int(v) for v in r) for r in tab):
        out[:, q // nao, q % nao] = X[:, r0:r1, c0:c1].mean(dim=(1, 2))
        scale[:, q // nao, q % nao] = X[:, r0:r1, c0:c1].abs().mean(dim=(1, 2))
    return out.reshape(-1, nao * nao), scale.reshape(-1, nao * nao)


def soc_assemble(H, ksi, L, inv, H0r, H0i, nao, symmetrize=True, zero_diag=False, defect=None):
    """so3 SOC spin blocks (hamgnn_output.py:3076-3144, 3603-3609): A_k = ksi L_k, anti-symmetrised against the partner row (0.5 (A_k - A_k[inv]^T)) when
    symmetrize; real = [[H, A_y], [A_y, H]] + H0r (without the spin-diagonal blocks of H0r when zero_diag, :3034-3049), imag = [[A_z, A_x], [-A_x, -A_z]]
    + H0i.  Returns ((real, imag), (scale_real, scale_imag))."""
    E = _d(H).shape[0]
    Hm, K, Lm = _d(H).reshape(E, nao, nao), _d(ksi).reshape(E, nao, nao), _d(L).reshape(E, nao, nao, 3)
    iv = torch.arange(E) if inv is None else _l(inv)

    def A(k):
        M = K * Lm[..., k]
        if not symmetrize:
            return M, M.abs()
        return 0.5 * (M - M[iv].transpose(1, 2)), 0.5 * (M.abs() + M[iv].transpose(1, 2).abs())
    (Ax, Sx), (Ay, Sy), (Az, Sz) = A(0), A(1), A(2)
    blk = lambda a, b, c, d: torch.cat([torch.cat([a, b], 2), torch.cat([c, d], 2)], 1)
    real, sreal = blk(Hm, Ay, Ay, Hm), blk(Hm.abs(), Sy, Sy, Hm.abs())
    imag, simag = blk(Az, Ax, -Ax, -Az), blk(Sz, Sx, Sx, Sz)
    if H0r is not None:
        h0 = _d(H0r).reshape(E, 2 * nao, 2 * nao).clone()
        if zero_diag and defect != "ignore_zero_diag":
            h0[:, :nao, :nao] = 0
            h0[:, nao:, nao:] = 0
        real, sreal = real + h0, sreal + h0.abs()
    if H0i is not None:
        h0 = _d(H0i).reshape(E, 2 * nao, 2 * nao)
        imag, simag = imag + h0, simag + h0.abs()
    f = lambda t: t.reshape(E, -1)
    return (f(real), f(imag)), (f(sreal), f(simag))
