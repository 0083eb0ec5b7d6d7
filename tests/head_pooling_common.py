"""Shared by tests/test_head_pooling_host.py (CPU) and tests/test_gpu_head_pooling.py (GPU): the three oldest kernel pairs of csrc/heads.hip --
anchor attention pooling, the slot-masked point mean, the masked point max -- as numpy: the float32 inputs of every case, the float64
reference of every output with its own per-element bound, and (for the CPU file) a float32 emulation of each kernel in the kernel's own
summation order.  Everything is evaluated from the SAME float32 operands, widened.

Bounds, u = 2^-24.  A sum is held to k u sum|terms| with k the float32 roundings on the longest path to the element, counted from the kernel
beside each count below (first order in u: every count includes at least one operation that is exact -- an add onto 0 -- and k (k - 1) u < 1,
so k u also covers the second-order terms of k - 1 roundings).  The masked max is exact.  The softmax confidence has a derived part and a
measured part, see attn_reference."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126                      # the smallest normal float32: below it the device may flush

B = 2
C_GRID = (1, 5)
NA_GRID = (4, 12, 20, 60, 64)
N_GRID = (1, 3, 15, 16, 17, 63, 64, 65, 130)
NS_GRID = (1, 3, 8)

ATTN_FAMILIES = ('randn_T1', 'randn_T3', 'wide_T3', 'equal_T3', 'neginf_T3')

# The exponential term of the confidence bound: 4 x the largest relative error of float32 torch.softmax(logits * T, -1) on the device against
# float64 (elements of at least 2^-126), measured on an MI355X over every attention input of this file, family by family (one constant for all
# would be the wide family's, 20 to 600 times what the others need).  profiles/head_pooling_bounds.txt has both measured values per family:
# torch's, below, and the kernel's.  See attn_reference for where the term enters.
SOFTMAX_REL_MEASURED = {'randn_T1': 4.14e-7, 'randn_T3': 1.71e-6, 'wide_T3': 3.06e-5, 'equal_T3': 5.3e-8, 'neginf_T3': 1.72e-6}
EXP_REL = {k: 4.0 * v for k, v in SOFTMAX_REL_MEASURED.items()}
SLOT_FAMILIES = ('hard', 'soft')
MAX_FAMILIES = ('hard', 'soft', 'all_negative', 'one_member', 'no_member', 'ties', 'zero_tie', 'nan')

f32, f64 = np.float32, np.float64


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _randn(rng, *shape):
    return rng.standard_normal(shape).astype(f32)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 = 0: an element that must be exact and is); inf when a value is not finite"""
    err = np.abs(np.asarray(got, f64) - ref)
    if not np.isfinite(err).all():
        return float('inf')
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ---- anchor attention pooling ----------------------------------------------------------------------------------------------------------

def attn_inputs(c, n, na, family):
    """x [B,c,n,na] ~ 1.7 randn + 0.4, logits [B,n,na], g [B,c,n], T.  Families: randn logits at T = 1 and 3; 40 randn at T = 3 (differences in
    the hundreds: a one-hot confidence with underflowed tails); all logits of a point equal; one logit per point -inf (a masked anchor)."""
    rng = _rng(1, c, n, na, ATTN_FAMILIES.index(family))
    x = _randn(rng, B, c, n, na) * f32(1.7) + f32(0.4)
    logits = _randn(rng, B, n, na)
    g = _randn(rng, B, c, n)
    if family == 'wide_T3':
        logits = logits * f32(40.0)
    if family == 'equal_T3':
        logits = np.ascontiguousarray(np.broadcast_to(logits[:, :, :1], logits.shape))
    if family == 'neginf_T3':
        np.put_along_axis(logits, rng.integers(0, na, (B, n, 1)), f32(-np.inf), axis=-1)
    return dict(x=x, logits=logits, g=g, T=1.0 if family == 'randn_T1' else 3.0, family=family)


def attn_reference(t, exp_rel=None):
    """float64 out [B,c,n], conf [B,n,na], dx [B,c,n,na], dlogits [B,n,na] and a bound for every element: {name: (ref, bound)}.

    conf_i = e_i / S, e_i = exp(z_i), z_i = T l_i - max_j T l_j.  The kernel (anchor_attn_pool_kernel) rounds T l_i (u |T l_i| on z_i; the
    maximum is one of those rounded products and shifts every z alike, which the quotient does not see) and the subtraction (u |z_i|): a
    relative u (|T l_i| + |z_i|) on e_i, derived.  The exponential itself: __expf scales z by log2 e before the hardware exp2 (|z_i| u more), and
    the accuracy of that instruction is not documented: exp_rel, measured (see EXP_REL).  With d_i the sum of the two, S carries the
    conf-weighted mean of the d_j and 7 adds (3 in a lane, 4 shuffle steps), then 1 / S and e_i * (1 / S): 9 u.
      |conf - ref| <= conf_i (d_i + sum_j conf_j d_j + 9 u)         where ref >= 2^-126
                   <= 2^-126                                         where ref < 2^-126 (the device may flush what it cannot represent)
    out = sum_a x_a conf_a: a product, 3 adds in the lane, 4 shuffle steps = 8 roundings, and the confidence's own error:
      sum_a |x_a| (8 u conf_a + cerr_a)
    dx = g conf: one product: |g| (u conf + cerr).
    dlogits_a = (T conf_a) (dc_a - s), dc_a = sum_c g_c x_ca a chain of c fused multiply-adds (c u A_a, A_a = sum_c |g_c x_ca|),
    s = sum_a conf_a dc_a as `out` (8 roundings) on operands that carry c u A_a and cerr_a; then one subtraction and two products (3 u) on
    |dc_a - s| <= D_a = A_a + sum_j conf_j A_j:
      |T| (conf_a (c u A_a + sum_j A_j ((8 + c) u conf_j + cerr_j)) + D_a (3 u conf_a + cerr_a))"""
    x, l, g = t['x'].astype(f64), t['logits'].astype(f64), t['g'].astype(f64)
    T = float(f32(t['T']))
    c = x.shape[1]
    exp_rel = EXP_REL[t['family']] if exp_rel is None else exp_rel
    tl = T * l
    finite = np.isfinite(tl)
    z = tl - tl.max(-1, keepdims=True)
    e = np.exp(z)
    conf = e / e.sum(-1, keepdims=True)
    with np.errstate(invalid='ignore'):
        d = np.where(finite, U * (np.abs(tl) + np.abs(z)) + exp_rel + np.abs(z) * U, 0.0)          # a masked anchor is exactly 0
    rel = d + (conf * d).sum(-1, keepdims=True) + 9 * U
    cerr = np.where(conf >= TINY, conf * rel, TINY)
    cb, cerrb = conf[:, None], cerr[:, None]
    out = (x * cb).sum(-1)
    out_bound = (np.abs(x) * (8 * U * cb + cerrb)).sum(-1)
    dx = g[..., None] * cb
    dx_bound = np.abs(g)[..., None] * (U * cb + cerrb)
    dc = (g[..., None] * x).sum(1)
    A = np.abs(g[..., None] * x).sum(1)
    s = (conf * dc).sum(-1, keepdims=True)
    dl = T * conf * (dc - s)
    s_err = (A * ((8 + c) * U * conf + cerr)).sum(-1, keepdims=True)
    D = A + (conf * A).sum(-1, keepdims=True)
    dl_bound = abs(T) * (conf * (c * U * A + s_err) + D * (3 * U * conf + cerr))
    return dict(out=(out, out_bound), conf=(conf, cerr), dx=(dx, dx_bound), dlogits=(dl, dl_bound))


def _fma(a, b, acc):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32 (a double
    rounding that differs from the single one of fmaf by at most 2^-29 u, far inside every bound the emulation is held to)"""
    return (a.astype(f64) * b.astype(f64) + acc.astype(f64)).astype(f32)


def _butterfly16(v):
    """row_sum<16>: v += shfl_xor(v, 8), 4, 2, 1 over the last axis (16 lanes); every lane ends with the same float32 value"""
    lanes = np.arange(16)
    for step in (8, 4, 2, 1):
        v = v + v[..., lanes ^ step]
    return v[..., 0]


def _quads(a, na):
    """[..., na] -> [..., 16, 4]: the 16 lanes of a point, idle lanes (quad >= na / 4) zero"""
    out = np.zeros(a.shape[:-1] + (64,), a.dtype)
    out[..., :na] = a
    return out.reshape(a.shape[:-1] + (16, 4))


def _lane4(p):
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]


def attn_emulate(t, logits=None):
    """anchor_attn_pool_kernel<false / true> in float32, operation by operation (products and sums rounded one by one where the compiler
    may fuse them: the longest path); the exponential is the correctly rounded one.  -> out, conf, dx, dlogits"""
    x, l, g, T = t['x'], t['logits'] if logits is None else logits, t['g'], f32(t['T'])
    b, c, n, na = x.shape
    with np.errstate(invalid='ignore', over='ignore'):
        lt = l * T
        z = lt - lt.max(-1, keepdims=True)
        e = np.exp(z.astype(f64)).astype(f32)
        inv = f32(1.0) / _butterfly16(_lane4(_quads(e, na)))                                       # [b,n]
        cf = e * inv[..., None]
        out = _butterfly16(_lane4(_quads(x * cf[:, None], na)))                                    # [b,c,n]
        dc = np.zeros((b, n, na), f32)
        for ci in range(c):
            dc = _fma(np.broadcast_to(g[:, ci, :, None], dc.shape), x[:, ci], dc)
        dx = g[..., None] * cf[:, None]
        s = _butterfly16(_lane4(_quads(cf * dc, na)))
        dl = (T * cf) * (dc - s[..., None])
    return dict(out=out, conf=cf, dx=dx, dlogits=dl)


# ---- slot-masked point mean --------------------------------------------------------------------------------------------------------------

def slot_inputs(c, n, na, ns, family):
    """x [B,c,n,na], mask [B,ns,n], inv_den [B,ns] (float32, made here: the reference widens this same tensor, so the denominator's rounding is
    not charged to the kernel), g [B,ns,c,na].  hard: 0/1 masks; in cloud 0 the last slot is empty and the one before it (the only one when
    ns = 1; then cloud 1 holds the empty slot) is the single point n - 1.  soft: rand + 0.05."""
    rng = _rng(2, c, n, na, ns, SLOT_FAMILIES.index(family))
    x = _randn(rng, B, c, n, na) * f32(1.7) + f32(0.4)
    g = _randn(rng, B, ns, c, na)
    if family == 'soft':
        mask = (rng.random((B, ns, n)) + 0.05).astype(f32)
    else:
        mask = (rng.random((B, ns, n)) > 0.5).astype(f32)
        single = np.zeros(n, f32)
        single[n - 1] = 1.0
        if ns == 1:
            mask[0, 0], mask[1, 0] = single, 0.0
        else:
            mask[0, ns - 2], mask[0, ns - 1] = single, 0.0
    inv_den = (f32(1.0) / np.maximum(mask.sum(-1, dtype=f32), f32(1e-8))).astype(f32)
    return dict(x=x, mask=mask, inv_den=inv_den, g=g)


def slot_reference(t):
    """forward out[b,s,c,a] = inv_den[b,s] sum_p m[b,s,p] x[b,c,p,a] (slot_mean_fwd_kernel): a lane's chain over the points p0, p0 + 16, ... is
    ceil(n / 16) fused multiply-adds, the fold of the 16 (wave, point group) partials through LDS 16 adds, the product with inv_den 1:
    k = ceil(n / 16) + 16 + 1.  backward dx[b,c,p,a] = sum_s m[b,s,p] (g[b,s,c,a] inv_den[b,s]) (slot_mean_bwd_kernel): the product g inv_den is
    rounded once, then a chain of ns fused multiply-adds: k = 1 + ns."""
    x, m, d, g = (t[k].astype(f64) for k in ('x', 'mask', 'inv_den', 'g'))
    n, ns = x.shape[2], m.shape[1]
    k_fwd = -(-n // 16) + 16 + 1
    k_bwd = 1 + ns
    dd = d[:, :, None, None]
    fwd = dd * np.einsum('bsn,bcna->bsca', m, x)
    fwd_abs = np.abs(dd) * np.einsum('bsn,bcna->bsca', np.abs(m), np.abs(x))
    gd = g * dd
    bwd = np.einsum('bsn,bsca->bcna', m, gd)
    bwd_abs = np.einsum('bsn,bsca->bcna', np.abs(m), np.abs(gd))
    return dict(fwd=(fwd, k_fwd * U * fwd_abs), bwd=(bwd, k_bwd * U * bwd_abs))


def _chains(a, axis):
    """points axis n -> (trips, 16): point p = trip * 16 + (wave * 4 + point group); the tail is padded with zeros (weight 0 on value 0 leaves a
    fused multiply-add's accumulator as it is, as not running the trip does)"""
    n = a.shape[axis]
    trips = -(-n // 16)
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, trips * 16 - n)
    a = np.pad(a, pad)
    return a.reshape(a.shape[:axis] + (trips, 16) + a.shape[axis + 1:]), trips


def slot_emulate(t, mask=None, inv_den=None, n_points=None):
    """slot_mean_fwd_kernel / slot_mean_bwd_kernel in float32 in the kernels' order: lane chains over p0, p0 + 16, ..., the 16 partials in index
    order, the product with inv_den.  n_points: the forward stops there (a mutation)."""
    x, g = t['x'], t['g']
    m = t['mask'] if mask is None else mask
    d = t['inv_den'] if inv_den is None else inv_den
    b, c, n, na = x.shape
    ns = m.shape[1]
    mf = m if n_points is None else np.where(np.arange(n) < n_points, m, f32(0.0)).astype(f32)
    xc, trips = _chains(x, 2)                                         # [b,c,trips,16,na]
    mc, _ = _chains(mf, 2)                                            # [b,ns,trips,16]
    acc = np.zeros((b, ns, c, 16, na), f32)
    for i in range(trips):
        acc = _fma(np.broadcast_to(mc[:, :, None, i, :, None], acc.shape), np.broadcast_to(xc[:, None, :, i], acc.shape), acc)
    tot = np.zeros((b, ns, c, na), f32)
    for j in range(16):
        tot = tot + acc[:, :, :, j]
    fwd = tot * d[:, :, None, None]
    gv = g * d[:, :, None, None]                                      # [b,ns,c,na]
    bwd = np.zeros((b, c, n, na), f32)
    for s in range(ns):
        bwd = _fma(np.broadcast_to(m[:, s, None, :, None], bwd.shape), np.broadcast_to(gv[:, s, :, None, :], bwd.shape), bwd)
    return dict(fwd=fwd, bwd=bwd)


# ---- masked point max ----------------------------------------------------------------------------------------------------------------------

def max_inputs(c, n, na, family):
    """x [B,c,n,na], mask [B,n], g [B,c,na].  hard / soft masks (point n - 1 of cloud 0 is a member and holds the maximum of channel 0,
    anchor 0); a channel of negative values with non-members present (pools to 0); a cloud with one member; a cloud with none; planted ties
    (the same value at two and at three member points, inside one lane's chain -- p and p + 16 -- and across lanes and waves -- p and
    p + 5); a member holding exactly 0.0 behind non-members in a negative channel; NaN at a member, at a non-member, at p = 0, at
    p = n - 1, and twice in one column."""
    rng = _rng(3, c, n, na, MAX_FAMILIES.index(family))
    x = _randn(rng, B, c, n, na)
    g = _randn(rng, B, c, na)
    mask = (rng.random((B, n)) > 0.5).astype(f32)
    if family == 'soft':
        mask = (rng.random((B, n)) + 0.05).astype(f32)
    if family in ('hard', 'soft'):
        mask[0, n - 1] = 1.0
        x[0, 0, n - 1, 0] = 900.0
    if family == 'all_negative':
        x[:, 0] = -np.abs(x[:, 0]) - f32(0.1)
        mask[:, 0] = 1.0
        if n > 1:
            mask[:, n - 1] = 0.0
    if family == 'one_member':
        mask[0] = 0.0
        mask[0, n // 2] = 1.0
    if family == 'no_member':
        mask[1] = 0.0
    if family == 'ties':
        plans = {(0, 0, 0): (1, 17), (0, 0, 1): (2, 7), (0, 0, 2): (3, 8, 19), (1, 0, 3): (0, 16, 32), (1, 0, 0): (4, 9),
                 (0, c - 1, 1): (n - 17, n - 1), (1, c - 1, 2): (n - 6, n - 1), (1, c - 1, 3): (0, n - 1)}
        for (bi, ci, ai), pts in plans.items():
            pts = sorted({p for p in pts if 0 <= p < n})
            if len(pts) >= 2:
                mask[bi, pts] = 1.0
                x[bi, ci, pts, ai] = 7.5
    if family == 'zero_tie':
        q = n // 2
        x[:, 0] = -np.abs(x[:, 0]) - f32(0.1)
        mask[:, :q] = 0.0
        mask[:, q] = 1.0
        x[:, 0, q] = 0.0
    if family == 'nan':
        pm, pn = n // 2, n // 2 + 1
        mask[:, pm] = 1.0
        x[0, 0, pm, 0] = np.nan                                       # a member
        if pn < n:
            mask[:, pn] = 0.0
            x[0, 0, pn, 1] = np.nan                                   # a non-member: 0 * NaN
        x[0, 0, 0, 2] = np.nan
        x[0, 0, n - 1, 3] = np.nan
        x[0, c - 1, n - 1, 0] = np.nan                                # twice in one column: the lower point is named
        x[0, c - 1, n // 3, 0] = np.nan
        x[1, 0, n - 1, 0] = np.nan
    return dict(x=x, mask=mask, g=g)


def max_reference(t):
    """The rule, not torch's arg-max: with prod = mask * x (one float32 product, the same on every IEEE machine), a column that holds a NaN
    gives NaN at the lowest point that has one; otherwise the maximum at the lowest point that attains it (-0.0 == +0.0).
    dx[b,c,p,a] = (p == arg) * mask[b,p] * g[b,c,a], one float32 product.  -> out, arg, dx (float64, int64, float64); all exact."""
    x, m, g = t['x'], t['mask'], t['g']
    with np.errstate(invalid='ignore'):
        prod = (m[:, None, :, None] * x).astype(f32).astype(f64)
    isn = np.isnan(prod)
    some = isn.any(2)
    finite = np.where(isn, -np.inf, prod)
    top = finite.max(2)
    arg = np.where(some, isn.argmax(2), (finite == top[:, :, None, :]).argmax(2))
    out = np.where(some, np.nan, top)
    hit = np.arange(x.shape[2])[None, None, :, None] == arg[:, :, None, :]
    dx = np.where(hit, (m[:, None, :, None] * g[:, :, None, :]).astype(f32).astype(f64), 0.0)
    return dict(out=out, arg=arg, dx=dx)


def same_values(got, ref):
    """equal by value, NaN where and only where the reference has one (-0.0 == +0.0: values, not bit patterns)"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return got.shape == ref.shape and bool(np.array_equal(np.isnan(got), np.isnan(ref))) and bool(np.all((got == ref) | np.isnan(ref)))


def max_emulate(t, mask=None, n_points=None, higher_on_tie=False):
    """masked_max_fwd_kernel / masked_max_bwd_kernel in float32 in the kernels' order: a lane's ascending chain keeps the first of equals and the
    first NaN, the 16 chains are folded in index order (larger, or equal at a lower point; a NaN beats a number, the lower NaN another).
    n_points, higher_on_tie: mutations."""
    x, g = t['x'], t['g']
    m = t['mask'] if mask is None else mask
    b, c, n, na = x.shape
    with np.errstate(invalid='ignore'):
        prod = m[:, None, :, None] * x
    if n_points is not None:
        prod = prod[:, :, :n_points]
    trips = -(-prod.shape[2] // 16)
    prod = np.pad(prod, [(0, 0), (0, 0), (0, trips * 16 - prod.shape[2]), (0, 0)], constant_values=-np.inf).reshape(b, c, trips, 16, na)
    best = np.full((b, c, 16, na), -np.inf, f32)
    at = np.zeros((b, c, 16, na), np.int64)
    lane = np.arange(16)[None, None, :, None]
    for i in range(trips):
        a = prod[:, :, i]
        take = ((a >= best) if higher_on_tie else (a > best)) | (np.isnan(a) & ~np.isnan(best))
        take &= (i * 16 + lane) < (n if n_points is None else n_points)
        best, at = np.where(take, a, best), np.where(take, i * 16 + lane, at)
    bv, bk = best[:, :, 0], at[:, :, 0]
    for j in range(1, 16):
        u, k = best[:, :, j], at[:, :, j]
        un, bn = np.isnan(u), np.isnan(bv)
        closer = (k > bk) if higher_on_tie else (k < bk)
        take = np.where(un | bn, un & (~bn | (k < bk)), (u > bv) | ((u == bv) & closer))
        bv, bk = np.where(take, u, bv), np.where(take, k, bk)
    hit = np.arange(n)[None, None, :, None] == bk[:, :, None, :]
    dx = np.where(hit, m[:, None, :, None] * g[:, :, None, :], f32(0.0)).astype(f32)
    return dict(out=bv, arg=bk, dx=dx)
