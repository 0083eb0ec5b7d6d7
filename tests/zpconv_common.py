"""Shared by tests/test_zpconv_common_host.py (CPU) and tests/test_gpu_zpconv_regimes.py (GPU): the four native zpconv operators of
csrc/zpconv.hip as plain numpy, the case table that places every dispatch regime of vgtk.cuda.zpconv, and two comparison modes.

  inter fwd : out[b,c,k,p,a]    = sum_n w[b,p,a,k,n] * feats[b,c,idx[b,p,a,k,n],a]
  inter bwd : gfeats[b,c,q,a]  += w[b,p,a,k,n] * grad[b,c,k,p,a]          (q = idx[b,p,a,k,n])
  intra fwd : out[b,c,k,p,a]    = sum_n w[a,k,n] * feats[b,c,p,idx[a,n]]
  intra bwd : gfeats[b,c,p,a'] += w[a,k,n] * grad[b,c,k,p,a]              (a' = idx[a,n])

Every reference is evaluated from the SAME operands in float64 or in int64 (`acc`), the transposes with np.add.at, and comes with T, the number of
products per output element, and A = sum |product| (the same reference on the operands' absolute values).

Exact mode: operands are non-zero integers from {+-1, +-2, +-3}.  Every partial sum in every order is an integer of magnitude <= A, and the
builder asserts A < 2^24, so float32 (and float64) arithmetic in ANY order -- MFMA, two-level partial sums, float atomics -- is exact: the kernel
must return the int64 reference bit for bit.  One dropped, repeated or misplaced term of any size changes an integer.

Float mode: randn features / gradients, w uniform in (0, 1) (random signs on every second case).  Bound per element k u A, k = 2 T: one rounding
per product and one per add, un-fused (a fused multiply-add has fewer), u = 2^-24 (2^-53 for float64 calls).  First order in u; k u <= 2^-14 is
asserted for every float case, so the second-order terms are below 2^-14 of the bound, and -- the reason for the cap -- a path that lost mantissa
bits (11 significant bits: 2^-12 per product) cannot hide below the bound.  Exact mode cannot see that: small integers survive fp16."""
import functools
import zlib

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
DT = {'f32': np.float32, 'f64': np.float64}
KU_CAP = 2.0 ** -14
EXACT_CAP = 2 ** 24

MATRIX, ROWS, SCALAR = 'zpconv_fwd_matrix', 'zpconv_fwd_rows', 'zpconv_fwd_scalar'
HOT, PRODUCTS, SCATTER, INTRA = 'zp_hot_kernel', 'zpconv_bwd_products', 'zpconv_bwd_scatter', 'intra_zpconv'

HOT_RCAP = 290                      # eap_inter_zpconv_bwd_hot_rows(): asserted on the device
HOT_TWO_STAGE_ROWS = 266            # (R + 1) * 512 + 2 * 12544 <= 158 KB: rows and the dump row, two operand stages


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 = 0: an element that must be exact and is); inf when a value is not finite"""
    err = np.abs(np.asarray(got, f64) - ref)
    if not np.isfinite(err).all():
        return float('inf')
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def float_bound(T, A, width='f32'):
    return 2.0 * T * U[width] * A


def exact_equal(got, ref):
    """bit for bit: every element of `got` (any float width) is the integer of the int64 reference; NaN / inf never are"""
    got = np.asarray(got)
    return got.shape == ref.shape and bool(np.array_equal(got.astype(f64), ref.astype(f64)))


# ---- references ------------------------------------------------------------------------------------------------------------------------

def _prep(x, acc, absolute):
    x = np.asarray(x).astype(acc)
    return np.abs(x) if absolute else x


def inter_forward(idx, w, feats, acc=f64, absolute=False):
    b, np_, na, ks, nn = idx.shape
    c = feats.shape[1]
    W, F = _prep(w, acc, absolute), _prep(feats, acc, absolute)
    out = np.zeros((b, c, ks, np_, na), acc)
    ar = np.arange(na)[:, None, None]
    for bi in range(b):
        for p in range(np_):
            G = F[bi][:, idx[bi, p], ar]                                   # [c, a, k, n]
            out[bi, :, :, p, :] = np.einsum('akn,cakn->cka', W[bi, p], G)
    return out


def inter_forward_T(idx):
    return float(idx.shape[-1])


def inter_backward(idx, w, grad, nq, acc=f64, absolute=False):
    b, np_, na, ks, nn = idx.shape
    c = grad.shape[1]
    W, G = _prep(w, acc, absolute), _prep(grad, acc, absolute)
    out = np.zeros((b, nq, na, c), acc)
    ar, cr = np.arange(na, dtype=i64)[:, None, None], np.arange(c, dtype=i64)
    for bi in range(b):
        flat_out = out[bi].reshape(-1)
        for p in range(np_):
            vals = W[bi, p][:, :, :, None] * G[bi, :, :, p, :].transpose(2, 1, 0)[:, :, None, :]      # [a, k, n, c]
            rows = (idx[bi, p].astype(i64) * na + ar)[..., None] * c + cr
            np.add.at(flat_out, rows.ravel(), vals.ravel())
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def inter_backward_T(idx, nq):
    """[b, 1, nq, na]: the number of (p, k, n) products that land on support row q at anchor a"""
    b, np_, na, ks, nn = idx.shape
    cnt = np.zeros((b, nq * na), f64)
    ar = np.arange(na, dtype=i64)[None, :, None, None]
    for bi in range(b):
        np.add.at(cnt[bi], (idx[bi].astype(i64) * na + ar).ravel(), 1.0)
    return cnt.reshape(b, 1, nq, na)


def intra_forward(idx, w, feats, acc=f64, absolute=False):
    W, F = _prep(w, acc, absolute), _prep(feats, acc, absolute)
    return np.ascontiguousarray(np.einsum('akn,bcpan->bckpa', W, F[..., idx]))


def intra_backward(idx, w, grad, na_in, acc=f64, absolute=False):
    W, G = _prep(w, acc, absolute), _prep(grad, acc, absolute)
    b, c, ks, np_, na_out = G.shape
    out = np.zeros((na_in, b, c, np_), acc)
    for k in range(ks):
        vals = W[:, k, :, None, None, None] * G[:, :, k].transpose(3, 0, 1, 2)[:, None]             # [a, n, b, c, p]
        np.add.at(out, idx.ravel(), vals.reshape((-1,) + vals.shape[2:]))
    return np.ascontiguousarray(out.transpose(1, 2, 3, 0))


def intra_backward_T(idx, ks, na_in):
    cnt = np.zeros(na_in, f64)
    np.add.at(cnt, idx.ravel(), float(ks))
    return cnt.reshape(1, 1, 1, na_in)


# ---- index builders: each asserts its own promise --------------------------------------------------------------------------------------

def lists_with_rows(b, np_, nq, R, seed, nn=64):
    """[b, np, nn] int32: one list per point, no repeats inside a list, the union of a cloud's lists exactly R rows, spread over [0, nq) (rank != row
    number), rows 0 and nq - 1 included, at least one row of nq unreferenced"""
    assert nn <= R < nq and np_ * nn >= R and R >= 2
    rng = np.random.default_rng([seed, b, np_, nq, R])
    out = np.empty((b, np_, nn), np.int32)
    for bi in range(b):
        inner = rng.permutation(np.arange(1, nq - 1))[:R - 2]
        rows = rng.permutation(np.concatenate([[0, nq - 1], inner]))
        for p in range(np_):                                               # windows of a cyclic walk: nn <= R distinct rows each, all R covered
            out[bi, p] = rng.permutation(rows[(p * nn + np.arange(nn)) % R])
        used = np.unique(out[bi])
        assert used.size == R and used[0] == 0 and used[-1] == nq - 1
        assert (np.sort(used) != np.arange(R)).any()                       # a row's rank among the referenced rows is not its number
        assert all(np.unique(out[bi, p]).size == nn for p in range(np_))
    return out


def random_lists(b, np_, nq, nn, seed):
    """[b, np, nn] int32: distinct rows inside a list when nq allows it, any rows otherwise"""
    rng = np.random.default_rng([seed, b, np_, nq, nn])
    if nq >= nn:
        return np.stack([np.stack([rng.permutation(nq)[:nn] for _ in range(np_)]) for _ in range(b)]).astype(np.int32).reshape(b, np_, nn)
    return rng.integers(0, nq, (b, np_, nn)).astype(np.int32)


def broadcast5d(lists, na, ks):
    b, np_, nn = lists.shape
    idx = np.ascontiguousarray(np.broadcast_to(lists[:, :, None, None, :], (b, np_, na, ks, nn))).astype(np.int32)
    assert (idx == idx[:, :, :1, :1, :]).all()
    return idx


def deviate(idx, where, nq):
    """a copy with ONE differing entry at where = (cloud, point, anchor, kernel point, neighbour) (negative positions count from the end)"""
    out = idx.copy()
    out[where] = (out[where] + 1) % nq
    assert (out != idx).sum() == 1
    return out


def padded(lists):
    """the second half of each list repeats its first entry (the ball query's padding of short lists)"""
    out = lists.copy()
    nn = out.shape[-1]
    out[..., nn // 2:] = out[..., :1]
    assert (out[..., nn // 2:] == out[..., :1]).all() and (out[..., :nn // 2] == lists[..., :nn // 2]).all()
    return out


def arbitrary5d(b, np_, na, ks, nn, nq, seed):
    idx = np.random.default_rng([seed, b, np_, na, ks, nn, nq]).integers(0, nq, (b, np_, na, ks, nn)).astype(np.int32)
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < nq)
    return idx


# ---- the case table --------------------------------------------------------------------------------------------------------------------

class Case:
    """kind 'fwd' / 'bwd' (inter).  index: one descriptor for every cloud or a list with one per cloud --
         int R            lists_with_rows with R referenced rows        'lists'   random lists, broadcast
         ('pad', R)       the same, padded                              'arb'     arbitrary 5-D index
         ('dev', d, pos)  descriptor d with one deviation at (p,a,k,n)  ('one', q) every entry names row q
    expect: the regime name after the Python call.  float_ok: the k u cap holds (asserted either way by the builder).
    Backward only: on_chip (vgtk.cuda.zpconv.ON_CHIP_BACKWARD), status (per cloud, of the on-chip entry), S (its point ranges per cloud),
    workspace ('slices' / 'none': BWD_WORKSPACE_BYTES of two clouds / of one cloud less a byte)."""

    def __init__(self, name, kind, b, np_, nq, na, ks, nn, c, index, expect, width='f32', float_ok=True, on_chip=True, status=None, S=None,
                 workspace=None, raises=None):
        self.name, self.kind, self.dims = name, kind, (b, np_, nq, na, ks, nn, c)
        self.index, self.expect, self.width, self.float_ok = index, expect, width, float_ok
        self.on_chip, self.status, self.S, self.workspace, self.raises = on_chip, status, S, workspace, raises
        self.seed = zlib.crc32(name.encode()) & 0x7fffffff
        self.signed_w = bool(self.seed & 1)

    def __repr__(self):
        return self.name


def _cloud_index(case, d, bi):
    b, np_, nq, na, ks, nn, c = case.dims
    seed = case.seed + 7919 * bi
    if isinstance(d, int):
        return broadcast5d(lists_with_rows(1, np_, nq, d, seed, nn), na, ks)
    if d == 'lists':
        return broadcast5d(random_lists(1, np_, nq, nn, seed), na, ks)
    if d == 'arb':
        return arbitrary5d(1, np_, na, ks, nn, nq, seed)
    if d[0] == 'pad':
        return broadcast5d(padded(lists_with_rows(1, np_, nq, d[1], seed, nn)), na, ks)
    if d[0] == 'one':
        return np.full((1, np_, na, ks, nn), d[1], np.int32)
    if d[0] == 'dev':
        return deviate(_cloud_index(case, d[1], bi), (0,) + tuple(d[2]), nq)
    raise ValueError(d)


def make_index(case):
    b, np_, nq, na, ks, nn, c = case.dims
    per = case.index if isinstance(case.index, list) else [case.index] * b
    assert len(per) == b
    if b == 0:
        return np.zeros((0, np_, na, ks, nn), np.int32)
    return np.ascontiguousarray(np.concatenate([_cloud_index(case, d, bi) for bi, d in enumerate(per)]))


def _hot(name, b, np_, nq, na, c, index, status, S, **kw):
    expect = HOT if not any(status) else PRODUCTS
    return Case('hot_' + name, 'bwd', b, np_, nq, na, 24, 64, c, index, expect, status=status, S=S, **kw)


def _cases():
    t = []
    # ---- on-chip backward (csrc/zpconv_bwd_hot.hip): ks = 24, nn = 64
    for R in (266, 267, 290, 291):                                         # two stages / one stage; the cap: 290 taken, 291 handed back
        t.append(_hot(f'rows{R}', 1, 11, 300, 4, 32, R, [int(R > HOT_RCAP)], 8))
    t.append(_hot('fewer_points_than_ranges', 1, 5, 260, 12, 32, 200, [0], 5))
    t.append(_hot('uneven_ranges', 3, 7, 200, 60, 64, 150, [0, 0, 0], 3))
    t.append(_hot('no_partial_b8', 8, 6, 200, 12, 32, 120, [0] * 8, 1))
    t.append(_hot('no_partial_b9', 9, 6, 200, 12, 32, 120, [0] * 9, 1))
    t.append(_hot('widest', 2, 9, 300, 64, 96, 250, [0, 0], 4))
    t.append(_hot('bitmap_limit', 1, 5, 16384, 4, 32, 100, [0], 5))
    t.append(Case('hot_past_bitmap_limit', 'bwd', 1, 5, 16385, 4, 24, 64, 32, 100, SCATTER))
    t.append(_hot('mixed', 5, 11, 300, 4, 32, [200, 291, ('pad', 200), ('dev', 200, (-1, -1, -1, -1)), 200], [0, 1, 1, 1, 0], 2, float_ok=False))
    # ---- product pipeline (csrc/zpconv_bwd.hip), ON_CHIP_BACKWARD off.  Base: 2 clouds, 7 points, 100 rows, 4 anchors, 24 x 64, 16 channels
    P = dict(on_chip=False)
    for c in (16, 20, 64, 80):
        t.append(Case(f'prod_c{c}', 'bwd', 2, 7, 100, 4, 24, 64, c, 'lists', PRODUCTS, **P))
    for ks in (1, 23):
        t.append(Case(f'prod_ks{ks}', 'bwd', 2, 7, 100, 4, ks, 64, 16, 'lists', PRODUCTS, **P))
    t.append(Case('prod_ks25_not_taken', 'bwd', 2, 7, 100, 4, 25, 64, 16, 'lists', SCATTER, **P))
    for nn in (4, 60):
        t.append(Case(f'prod_nn{nn}', 'bwd', 2, 7, 100, 4, 24, nn, 16, 'lists', PRODUCTS, **P))
    for na in (28, 64):
        t.append(Case(f'prod_na{na}', 'bwd', 2, 7, 100, na, 24, 64, 16, 'lists', PRODUCTS, **P))
    for np_ in (1, 9):
        t.append(Case(f'prod_np{np_}', 'bwd', 2, np_, 100, 4, 24, 64, 16, 'lists', PRODUCTS, **P))
    t.append(Case('prod_one_row', 'bwd', 2, 7, 100, 4, 24, 64, 16, ['lists', ('one', 37)], PRODUCTS, float_ok=False, **P))
    for pos in (0, 1, 2):
        index = ['lists'] * 3
        index[pos] = ('dev', 'lists', (3, 2, 11, 40))
        t.append(Case(f'prod_deviating_cloud{pos}', 'bwd', 3, 7, 100, 4, 24, 64, 16, index, PRODUCTS, **P))
    t.append(Case('prod_sliced_batch', 'bwd', 5, 7, 100, 4, 24, 64, 16, 'lists', PRODUCTS, workspace='slices', **P))
    t.append(Case('prod_no_scratch', 'bwd', 5, 7, 100, 4, 24, 64, 16, 'lists', SCATTER, workspace='none', **P))
    # ---- forward matrix path (csrc/zpconv_mfma.hip).  Base: 2 clouds, 7 points, 50 rows, 4 anchors, 3 x 16, 16 channels
    for np_ in (1, 7, 8, 9, 17):
        t.append(Case(f'matrix_np{np_}', 'fwd', 2, np_, 50, 4, 3, 16, 16, 'lists', MATRIX))
    for na in (32, 36, 60, 64):
        t.append(Case(f'matrix_na{na}', 'fwd', 2, 7, 50, na, 3, 16, 16, 'lists', MATRIX))
    for c in (64, 80, 144):
        t.append(Case(f'matrix_c{c}', 'fwd', 2, 7, 50, 4, 3, 16, c, 'lists', MATRIX))
    for ks in (1, 24, 32):
        t.append(Case(f'matrix_ks{ks}', 'fwd', 2, 7, 50, 4, ks, 16, 16, 'lists', MATRIX))
    t.append(Case('matrix_ks33_not_taken', 'fwd', 2, 7, 50, 4, 33, 16, 16, 'lists', ROWS))
    t.append(Case('matrix_nn64', 'fwd', 2, 7, 50, 4, 3, 64, 16, 'lists', MATRIX))
    t.append(Case('matrix_nn128_na28', 'fwd', 2, 7, 50, 28, 3, 128, 16, 'lists', MATRIX))
    t.append(Case('matrix_b65', 'fwd', 65, 1, 50, 4, 1, 16, 16, 'lists', MATRIX))
    dev = ('dev', 'lists', (5, 3, 2, 15))
    t.append(Case('matrix_deviating_first', 'fwd', 3, 7, 50, 4, 3, 16, 16, [dev, 'lists', 'lists'], MATRIX))
    t.append(Case('matrix_deviating_last', 'fwd', 3, 7, 50, 4, 3, 16, 16, ['lists', 'lists', dev], MATRIX))
    t.append(Case('matrix_deviating_only', 'fwd', 1, 7, 50, 4, 3, 16, 16, [dev], MATRIX))
    # ---- forward rows kernel (csrc/zpconv_rows.hip).  Base: 2 clouds, 5 points, 30 rows, 4 anchors, 3 x 4, 8 channels
    for c in (8, 9, 12, 15, 72):
        t.append(Case(f'rows_c{c}', 'fwd', 2, 5, 30, 4, 3, 4, c, 'lists', ROWS))
    for na in (8, 60, 64):
        t.append(Case(f'rows_na{na}', 'fwd', 2, 5, 30, na, 3, 4, 8, 'lists', ROWS))
    for ks in (1, 8, 9, 17):
        t.append(Case(f'rows_ks{ks}', 'fwd', 2, 5, 30, 4, ks, 4, 8, 'lists', ROWS))
    t.append(Case('rows_nn20', 'fwd', 2, 5, 30, 4, 3, 20, 8, 'lists', ROWS))
    t.append(Case('rows_nn72_na60_last_in_lds', 'fwd', 1, 3, 80, 60, 3, 72, 8, 'lists', ROWS))
    t.append(Case('rows_nn76_na60_not_taken', 'fwd', 1, 3, 80, 60, 3, 76, 8, 'lists', SCALAR))
    t.append(Case('rows_arbitrary', 'fwd', 2, 5, 30, 4, 3, 4, 8, 'arb', ROWS))
    t.append(Case('rows_deviation_in_third_tile', 'fwd', 1, 3, 30, 4, 17, 4, 8, [('dev', 'lists', (1, 2, 16, 3))], ROWS))
    # ---- scalar kernels (csrc/zpconv.hip), both widths, both directions.  Base: 2 clouds, 3 points, 9 rows, 5 anchors, 3 x 3
    for width in ('f32', 'f64'):
        for kind, expect in (('fwd', SCALAR), ('bwd', SCATTER)):
            for c in (1, 7, 9):
                t.append(Case(f'scalar_{kind}_{width}_c{c}', kind, 2, 3, 9, 5, 3, 3, c, 'arb', expect, width=width))
            for na in (1, 63, 64):
                t.append(Case(f'scalar_{kind}_{width}_na{na}', kind, 2, 3, 9, na, 3, 3, 2, 'arb', expect, width=width))
            for nn in (0, 1):
                t.append(Case(f'scalar_{kind}_{width}_nn{nn}', kind, 2, 3, 9, 5, 3, nn, 2, 'arb', expect, width=width))
            # launch_inter: (sizeof(T) + 4) * na * (2 nn + 1) <= 160 KB at na = 64 -> nn <= 159 (float32), nn <= 106 (float64)
            last = 159 if width == 'f32' else 106
            t.append(Case(f'scalar_{kind}_{width}_lds_last', kind, 1, 1, 200, 64, 1, last, 1, 'arb', expect, width=width))
            t.append(Case(f'scalar_{kind}_{width}_lds_past', kind, 1, 1, 200, 64, 1, last + 1, 1, 'arb', expect, width=width,
                          raises='neighbourhood too large for LDS staging'))
            t.append(Case(f'scalar_{kind}_{width}_empty_batch', kind, 0, 3, 9, 5, 3, 3, 2, 'arb', None, width=width))
    return t


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# misaligned operands (a contiguous view 4 bytes into its storage): a shape the aligned call serves on the matrix cores in both directions
MISALIGNED_FWD = Case('misaligned_fwd', 'fwd', 2, 5, 120, 4, 24, 64, 32, 80, MATRIX)
MISALIGNED_BWD = Case('misaligned_bwd', 'bwd', 2, 5, 120, 4, 24, 64, 32, 80, HOT, status=[0, 0], S=4)
ALL_CASES = CASES + [MISALIGNED_FWD, MISALIGNED_BWD]
BY_NAME = {c.name: c for c in ALL_CASES}

# intra: (b, c, np, a_in, a_out, ks, nn)
INTRA_CASES = [(2, 3, np_, a_in, a_out, 3, nn) for (a_in, a_out) in ((60, 60), (12, 60), (60, 64), (4, 1)) for np_ in (1, 4, 5) for nn in (1, 12)]
MODES = ('exact', 'float')


def _values(rng, shape, mode, width):
    if mode == 'exact':
        return rng.choice(np.array([-3, -2, -1, 1, 2, 3]), shape).astype(DT[width])
    return rng.standard_normal(shape).astype(f32).astype(DT[width])


def _weights(rng, shape, mode, width, signed):
    if mode == 'exact':
        return _values(rng, shape, mode, width)
    w = (1.0 - rng.random(shape, dtype=f32))                               # (0, 1]
    w = np.where(w >= 1.0, f32(0.5), w).astype(f32)                        # (0, 1)
    if signed:
        w = w * rng.choice(np.array([-1, 1], f32), shape)
    return w.astype(DT[width])


def operands(case, mode):
    """idx [b,np,na,ks,nn] int32, w, x (feats [b,c,nq,na] or grad [b,c,ks,np,na]) in the case's width"""
    b, np_, nq, na, ks, nn, c = case.dims
    rng = np.random.default_rng([case.seed, MODES.index(mode)])
    idx = make_index(case)
    w = _weights(rng, idx.shape, mode, case.width, case.signed_w)
    x = _values(rng, (b, c, nq, na) if case.kind == 'fwd' else (b, c, ks, np_, na), mode, case.width)
    return idx, w, x


def evaluate(case, idx, w, x, acc=f64, absolute=False):
    nq = case.dims[2]
    if case.kind == 'fwd':
        return inter_forward(idx, w, x, acc, absolute)
    return inter_backward(idx, w, x, nq, acc, absolute)


def products(case, idx):
    return inter_forward_T(idx) if case.kind == 'fwd' else inter_backward_T(idx, case.dims[2])


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """(ref, T, A) of a case of the table: the int64 reference in exact mode, the float64 one in float mode.  The builder's conditions are
    asserted here, on the CPU: A < 2^24 (exact mode) and k u = 2 T u <= 2^-14 on every element (float mode, where the case claims it)."""
    case = BY_NAME[name]
    idx, w, x = operands(case, mode)
    T = products(case, idx)
    A = evaluate(case, idx, w, x, f64, absolute=True)
    if mode == 'exact':
        assert A.size == 0 or A.max() < EXACT_CAP, (name, A.max())
        ref = evaluate(case, idx, w, x, i64)
    else:
        assert case.float_ok and ku_max(case, T) <= KU_CAP, (name, ku_max(case, T))
        ref = evaluate(case, idx, w, x, f64)
    for a in (ref, A):
        a.setflags(write=False)
    return ref, T, A


def ku_max(case, T):
    return 2.0 * float(np.max(T)) * U[case.width] if np.size(T) else 0.0


def modes_of(case):
    return MODES if case.float_ok else MODES[:1]


def check(got, name, mode):
    """-> (ok, figure): exact mode: bit equality (figure = number of differing elements); float mode: worst ratio <= 1"""
    case = BY_NAME[name]
    ref, T, A = reference(name, mode)
    got = np.asarray(got)
    if mode == 'exact':
        ok = exact_equal(got, ref)
        return ok, (0 if ok else int((got.astype(f64) != ref.astype(f64)).sum()) if got.shape == ref.shape else -1)
    if got.shape != ref.shape:
        return False, float('inf')
    r = worst_ratio(got, ref, float_bound(T, A, case.width))
    return r <= 1.0, r


def intra_operands(shape, mode, width):
    b, c, np_, a_in, a_out, ks, nn = shape
    rng = np.random.default_rng([11, MODES.index(mode)] + list(shape))
    idx = rng.integers(0, a_in, (a_out, nn)).astype(np.int32)
    w = _weights(rng, (a_out, ks, nn), mode, width, bool(np_ & 1))
    feats = _values(rng, (b, c, np_, a_in), mode, width)
    grad = _values(rng, (b, c, ks, np_, a_out), mode, width)
    return idx, w, feats, grad


def intra_reference(shape, mode, width):
    """{'fwd': (ref, T, A), 'bwd': (ref, T, A)}"""
    b, c, np_, a_in, a_out, ks, nn = shape
    idx, w, feats, grad = intra_operands(shape, mode, width)
    acc = i64 if mode == 'exact' else f64
    out = {'fwd': (intra_forward(idx, w, feats, acc), float(nn), intra_forward(idx, w, feats, f64, True)),
           'bwd': (intra_backward(idx, w, grad, a_in, acc), intra_backward_T(idx, ks, a_in), intra_backward(idx, w, grad, a_in, f64, True))}
    for ref, T, A in out.values():
        assert A.max() < EXACT_CAP and 2.0 * np.max(T) * U[width] <= KU_CAP
    return out


# ---- perturbations of a correct result (the comparator's sensitivity) ------------------------------------------------------------------

PERTURBATIONS = ('drop', 'twice', 'move', 'swap', 'unreferenced')


def perturbed(case, mode, kind):
    """The correct result of a case (the reference, rounded once to the case's width) with ONE wrong term, or None when the case has no such term:
    one 5-D entry (b, p, a, k, n) dropped, counted twice, moved to the neighbouring support row, its weight swapped with the next kernel
    point's; or one support row nobody references left non-zero (backward).  Among the neighbours n of the chosen (b, p, a, k) the one with the
    largest effect is taken, and only elements with at least 2 products are touched."""
    b, np_, nq, na, ks, nn, c = case.dims
    if b == 0 or nn == 0:
        return None
    idx, w, x = operands(case, mode)
    ref, T, A = reference(case.name, mode)
    W, X = w.astype(f64), x.astype(f64)
    delta = np.zeros(ref.shape, f64)
    bi, p, a, k = b - 1, np_ - 1, na - 1, ks - 1
    k2 = (k + 1) % ks
    if kind == 'unreferenced':
        if case.kind != 'bwd':
            return None
        free = np.flatnonzero(np.asarray(T)[bi, 0, :, a] == 0)
        if free.size == 0:
            return None
        delta[bi, c - 1, free[-1], a] = 1.0 if mode == 'exact' else 2.0 ** -40
    else:
        best = None
        for n in range(nn):
            d = []                                                         # (element without its channel axis, change for every channel)
            q, q2 = int(idx[bi, p, a, k, n]), int(idx[bi, p, a, k2, n])
            qm = q + 1 if q + 1 < nq else q - 1
            wk, wk2 = W[bi, p, a, k, n], W[bi, p, a, k2, n]
            if case.kind == 'fwd':
                if T < 2:
                    continue
                here, term = (bi, k, p, a), wk * X[bi, :, q, a]
                if kind in ('drop', 'twice'):
                    d = [(here, -term if kind == 'drop' else term)]
                elif kind == 'move' and qm >= 0:
                    d = [(here, wk * X[bi, :, qm, a] - term)]
                elif kind == 'swap' and ks > 1:
                    term2 = wk2 * X[bi, :, q2, a]
                    d = [(here, term2 - term), ((bi, k2, p, a), term - term2)]
            else:
                if T[bi, 0, q, a] < 2:
                    continue
                here, term = (bi, q, a), wk * X[bi, :, k, p, a]
                if kind in ('drop', 'twice'):
                    d = [(here, -term if kind == 'drop' else term)]
                elif kind == 'move' and qm >= 0:
                    d = [(here, -term), ((bi, qm, a), term)]
                elif kind == 'swap' and ks > 1 and T[bi, 0, q2, a] >= 2:
                    # the two entries exchange their weights: w[k2] grad[k] lands on q, w[k] grad[k2] on q2
                    d = [(here, (wk2 - wk) * X[bi, :, k, p, a]), ((bi, q2, a), (wk - wk2) * X[bi, :, k2, p, a])]
            merged = {}
            for where, v in d:
                merged[where] = merged.get(where, 0.0) + v
            size = max((float(np.abs(v).max()) for v in merged.values()), default=0.0)
            if size > 0.0 and (best is None or size > best[0]):
                best = (size, merged)
        if best is None:
            return None
        for where, v in best[1].items():
            delta[(where[0], slice(None)) + where[1:]] += v
    return (ref.astype(f64) + delta).astype(DT[case.width])


def round_to_bits(w, bits=11):
    """w rounded to `bits` significant bits: what a path that went through a 16-bit format would have multiplied with"""
    m, e = np.frexp(np.asarray(w, f64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)
