"""Shared by tests/test_head_pooling_wide_host.py (CPU) and tests/test_gpu_head_pooling_wide.py (GPU): the wide twins of the three oldest
kernel pairs (csrc/heads.hip at Q = 64: one wavefront per point, anchor rows of up to 256 floats) as numpy.  The float32 inputs and the float64
expressions are those of tests/head_pooling_common.py (same generators, same families); the per-element bounds are counted from the NEW
kernels, and the float32 emulations follow the new kernels' summation order.

Bounds, u = 2^-24: a sum is held to k u sum|terms| with k the float32 roundings on the longest path to the element, counted beside each
count below (see head_pooling_common for why k u covers the second-order terms).  The masked max is exact."""
import numpy as np

import head_pooling_common as H
from head_pooling_common import (ATTN_FAMILIES, MAX_FAMILIES, SLOT_FAMILIES, TINY, U, attn_inputs, max_inputs, max_reference,  # noqa: F401
                                 same_values, slot_inputs, worst_ratio, _fma, _lane4)

f32, f64 = np.float32, np.float64

B = H.B
C_GRID = (1, 5)
NA_GRID = (60, 68, 128, 240, 252, 256)          # the overlap with the narrow kernels; 17 quads; 32; the use_2d count; one idle lane; none
N_GRID = (1, 3, 4, 5, 9, 17)                    # below, at and across the block's 4 points; several wave iterations
NS_GRID = (1, 3, 8)
WAVES = 4                                       # waves per block: the point chains of the slot mean and the masked max

# The exponential term of the confidence bound, as head_pooling_common.EXP_REL takes it: 4 x the largest relative error of float32
# torch.softmax(logits * T, -1) on the device against float64 (elements of at least 2^-126), measured on an MI355X over every attention input
# of THIS file's grid, family by family (tools/head_pooling_wide_bounds.py; profiles/head_pooling_wide_bounds.txt has torch's figures, below,
# and the kernel's: KERNEL_CONF_REL_MEASURED, recorded and not used by any bound).
SOFTMAX_REL_MEASURED = {'randn_T1': 4.26e-7, 'randn_T3': 1.70e-6, 'wide_T3': 3.06e-5, 'equal_T3': 5.77e-8, 'neginf_T3': 1.78e-6}
KERNEL_CONF_REL_MEASURED = {'randn_T1': 6.81e-7, 'randn_T3': 2.27e-6, 'wide_T3': 3.32e-5, 'equal_T3': 5.77e-8, 'neginf_T3': 2.53e-6}
EXP_REL = {k: 4.0 * v for k, v in SOFTMAX_REL_MEASURED.items()}

SUM_ADDS = 3 + 6                                # a sum over the anchors of a point: 3 adds in the lane, 6 shuffle steps over the wave


# ---- anchor attention pooling ----------------------------------------------------------------------------------------------------------

def attn_reference(t, exp_rel=None):
    """float64 out [B,c,n], conf [B,n,na], dx [B,c,n,na], dlogits [B,n,na] and a bound for every element: {name: (ref, bound)}; the
    derivation is head_pooling_common.attn_reference's with the counts of anchor_attn_pool_kernel<64, BWD>:

    conf_i = e_i / S: the argument terms d_i = u (|T l_i| + |z_i|) + exp_rel + |z_i| u are unchanged (the same statements); S carries the
    conf-weighted mean of the d_j and SUM_ADDS = 9 adds (3 in a lane, 6 shuffle steps), then 1 / S and e_i * (1 / S): 11 u.
      |conf - ref| <= conf_i (d_i + sum_j conf_j d_j + 11 u)        where ref >= 2^-126;   <= 2^-126 below it (the device may flush)
    out = sum_a x_a conf_a: a product, 3 adds in the lane, 6 shuffle steps = 10 roundings, and the confidence's own error:
      sum_a |x_a| (10 u conf_a + cerr_a)
    dx = g conf: one product: |g| (u conf + cerr).
    dlogits_a = (T conf_a) (dc_a - s): dc_a a chain of c fused multiply-adds (c u A_a), s = sum_a conf_a dc_a as `out` (10 roundings) on
    operands that carry c u A_a and cerr_a; then one subtraction and two products (3 u) on |dc_a - s| <= D_a:
      |T| (conf_a (c u A_a + sum_j A_j ((10 + c) u conf_j + cerr_j)) + D_a (3 u conf_a + cerr_a))"""
    x, l, g = t['x'].astype(f64), t['logits'].astype(f64), t['g'].astype(f64)
    T = float(f32(t['T']))
    c = x.shape[1]
    exp_rel = EXP_REL[t['family']] if exp_rel is None else exp_rel
    k_sum = 1 + SUM_ADDS                                                                           # 10
    tl = T * l
    finite = np.isfinite(tl)
    z = tl - tl.max(-1, keepdims=True)
    e = np.exp(z)
    conf = e / e.sum(-1, keepdims=True)
    with np.errstate(invalid='ignore'):
        d = np.where(finite, U * (np.abs(tl) + np.abs(z)) + exp_rel + np.abs(z) * U, 0.0)          # a masked anchor is exactly 0
    rel = d + (conf * d).sum(-1, keepdims=True) + (SUM_ADDS + 2) * U
    cerr = np.where(conf >= TINY, conf * rel, TINY)
    cb, cerrb = conf[:, None], cerr[:, None]
    out = (x * cb).sum(-1)
    out_bound = (np.abs(x) * (k_sum * U * cb + cerrb)).sum(-1)
    dx = g[..., None] * cb
    dx_bound = np.abs(g)[..., None] * (U * cb + cerrb)
    dc = (g[..., None] * x).sum(1)
    A = np.abs(g[..., None] * x).sum(1)
    s = (conf * dc).sum(-1, keepdims=True)
    dl = T * conf * (dc - s)
    s_err = (A * ((k_sum + c) * U * conf + cerr)).sum(-1, keepdims=True)
    D = A + (conf * A).sum(-1, keepdims=True)
    dl_bound = abs(T) * (conf * (c * U * A + s_err) + D * (3 * U * conf + cerr))
    return dict(out=(out, out_bound), conf=(conf, cerr), dx=(dx, dx_bound), dlogits=(dl, dl_bound))


def _butterfly64(v):
    """row_sum<64>: v += shfl_xor(v, 32), 16, 8, 4, 2, 1 over the last axis (64 lanes); every lane ends with the same float32 value"""
    lanes = np.arange(64)
    for step in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ step]
    return v[..., 0]


def _quads(a, na):
    """[..., na] -> [..., 64, 4]: the 64 lanes of a point's wave, idle lanes (quad >= na / 4) zero"""
    out = np.zeros(a.shape[:-1] + (256,), a.dtype)
    out[..., :na] = a
    return out.reshape(a.shape[:-1] + (64, 4))


def attn_emulate(t, logits=None):
    """anchor_attn_pool_kernel<64, false / true> in float32, operation by operation (products and sums rounded one by one where the
    compiler may fuse them: the longest path); the exponential is the correctly rounded one.  -> out, conf, dx, dlogits"""
    x, l, g, T = t['x'], t['logits'] if logits is None else logits, t['g'], f32(t['T'])
    b, c, n, na = x.shape
    with np.errstate(invalid='ignore', over='ignore'):
        lt = l * T
        z = lt - lt.max(-1, keepdims=True)
        e = np.exp(z.astype(f64)).astype(f32)
        inv = f32(1.0) / _butterfly64(_lane4(_quads(e, na)))                                       # [b,n]
        cf = e * inv[..., None]
        out = _butterfly64(_lane4(_quads(x * cf[:, None], na)))                                    # [b,c,n]
        dc = np.zeros((b, n, na), f32)
        for ci in range(c):
            dc = _fma(np.broadcast_to(g[:, ci, :, None], dc.shape), x[:, ci], dc)
        dx = g[..., None] * cf[:, None]
        s = _butterfly64(_lane4(_quads(cf * dc, na)))
        dl = (T * cf) * (dc - s[..., None])
    return dict(out=out, conf=cf, dx=dx, dlogits=dl)


# ---- slot-masked point mean --------------------------------------------------------------------------------------------------------------

def slot_reference(t):
    """forward out[b,s,c,a] = inv_den[b,s] sum_p m[b,s,p] x[b,c,p,a] (slot_mean_fwd_kernel<64, NS>): a lane's chain over the points w, w + 4, ...
    is ceil(n / 4) fused multiply-adds, the fold of the 4 waves' partials through LDS 4 adds, the product with inv_den 1:
    k = ceil(n / 4) + 4 + 1.  backward dx[b,c,p,a] = sum_s m[b,s,p] (g[b,s,c,a] inv_den[b,s]) (slot_mean_bwd_kernel<64, NS>): the product
    g inv_den is rounded once, then a chain of ns fused multiply-adds: k = 1 + ns."""
    x, m, d, g = (t[k].astype(f64) for k in ('x', 'mask', 'inv_den', 'g'))
    n, ns = x.shape[2], m.shape[1]
    k_fwd = -(-n // WAVES) + WAVES + 1
    k_bwd = 1 + ns
    dd = d[:, :, None, None]
    fwd = dd * np.einsum('bsn,bcna->bsca', m, x)
    fwd_abs = np.abs(dd) * np.einsum('bsn,bcna->bsca', np.abs(m), np.abs(x))
    gd = g * dd
    bwd = np.einsum('bsn,bsca->bcna', m, gd)
    bwd_abs = np.einsum('bsn,bsca->bcna', np.abs(m), np.abs(gd))
    return dict(fwd=(fwd, k_fwd * U * fwd_abs), bwd=(bwd, k_bwd * U * bwd_abs))


def _chains(a, axis):
    """points axis n -> (trips, 4): point p = trip * 4 + wave; the tail is padded with zeros (weight 0 on value 0 leaves a fused
    multiply-add's accumulator as it is, as not running the trip does)"""
    n = a.shape[axis]
    trips = -(-n // WAVES)
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, trips * WAVES - n)
    a = np.pad(a, pad)
    return a.reshape(a.shape[:axis] + (trips, WAVES) + a.shape[axis + 1:]), trips


def slot_emulate(t, mask=None, inv_den=None, n_points=None):
    """slot_mean_fwd_kernel<64, NS> / slot_mean_bwd_kernel<64, NS> in float32 in the kernels' order: wave chains over w, w + 4, ..., the 4 partials
    in wave order, the product with inv_den.  n_points: the forward stops there (a mutation)."""
    x, g = t['x'], t['g']
    m = t['mask'] if mask is None else mask
    d = t['inv_den'] if inv_den is None else inv_den
    b, c, n, na = x.shape
    ns = m.shape[1]
    mf = m if n_points is None else np.where(np.arange(n) < n_points, m, f32(0.0)).astype(f32)
    xc, trips = _chains(x, 2)                                         # [b,c,trips,4,na]
    mc, _ = _chains(mf, 2)                                            # [b,ns,trips,4]
    acc = np.zeros((b, ns, c, WAVES, na), f32)
    for i in range(trips):
        acc = _fma(np.broadcast_to(mc[:, :, None, i, :, None], acc.shape), np.broadcast_to(xc[:, None, :, i], acc.shape), acc)
    tot = np.zeros((b, ns, c, na), f32)
    for j in range(WAVES):
        tot = tot + acc[:, :, :, j]
    fwd = tot * d[:, :, None, None]
    gv = g * d[:, :, None, None]                                      # [b,ns,c,na]
    bwd = np.zeros((b, c, n, na), f32)
    for s in range(ns):
        bwd = _fma(np.broadcast_to(m[:, s, None, :, None], bwd.shape), np.broadcast_to(gv[:, s, :, None, :], bwd.shape), bwd)
    return dict(fwd=fwd, bwd=bwd)


# ---- masked point max ----------------------------------------------------------------------------------------------------------------------

def max_emulate(t, mask=None, n_points=None, higher_on_tie=False):
    """masked_max_fwd_kernel<64> / masked_max_bwd_kernel<64> in float32 in the kernels' order: a wave's ascending chain w, w + 4, ... keeps the
    first of equals and the first NaN, the 4 chains are folded in wave order (larger, or equal at a lower point; a NaN beats a number, the
    lower NaN another).  n_points, higher_on_tie: mutations."""
    x, g = t['x'], t['g']
    m = t['mask'] if mask is None else mask
    b, c, n, na = x.shape
    with np.errstate(invalid='ignore'):
        prod = m[:, None, :, None] * x
    if n_points is not None:
        prod = prod[:, :, :n_points]
    trips = -(-prod.shape[2] // WAVES)
    prod = np.pad(prod, [(0, 0), (0, 0), (0, trips * WAVES - prod.shape[2]), (0, 0)], constant_values=-np.inf).reshape(b, c, trips, WAVES, na)
    best = np.full((b, c, WAVES, na), -np.inf, f32)
    at = np.zeros((b, c, WAVES, na), np.int64)
    lane = np.arange(WAVES)[None, None, :, None]
    for i in range(trips):
        a = prod[:, :, i]
        take = ((a >= best) if higher_on_tie else (a > best)) | (np.isnan(a) & ~np.isnan(best))
        take &= (i * WAVES + lane) < (n if n_points is None else n_points)
        best, at = np.where(take, a, best), np.where(take, i * WAVES + lane, at)
    bv, bk = best[:, :, 0], at[:, :, 0]
    for j in range(1, WAVES):
        u, k = best[:, :, j], at[:, :, j]
        un, bn = np.isnan(u), np.isnan(bv)
        closer = (k > bk) if higher_on_tie else (k < bk)
        take = np.where(un | bn, un & (~bn | (k < bk)), (u > bv) | ((u == bv) & closer))
        bv, bk = np.where(take, u, bv), np.where(take, k, bk)
    hit = np.arange(n)[None, None, :, None] == bk[:, :, None, :]
    dx = np.where(hit, m[:, None, :, None] * g[:, :, None, :], f32(0.0)).astype(f32)
    return dict(out=bv, arg=bk, dx=dx)
