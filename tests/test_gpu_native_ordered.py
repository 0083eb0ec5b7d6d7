"""GPU: the ordered (atomics-free) backwards of the point gather and the two native zpconv operators (csrc/native_ordered.hip),
at float32 and float64.

The expectations are restated here on the CPU with NumPy, one term at a time in the documented order -- the product rounded in the
operand width, then added to a running sum that starts at zero:
    gather  grad_pts[b,c,q]  : j ascending over idx[b,j] == q
    intra   gfeats[b,c,p,a'] : a ascending, then k, then n ascending over idx[a,n] == a'
    inter   gfeats[b,c,q,a]  : the entry number (p ks + k) ann + n ascending over idx[b,p,a,k,n] == q
and every case is checked five ways: (1) random operands give that evaluation BIT FOR BIT (a kernel that adds in another order, or
fuses the product into the add, fails here); (2) small-integer operands give the int64 result exactly; (3) float32 stays within
(T + 1) u sum|terms| of the float64 evaluation of the same operands, T the number of terms of the output element and u = 2^-24 (T
roundings of the products and T - 1 of the sums, first order, the + 1 for the second-order terms; for float64 the reference IS the
evaluation of (1)); (4) a second call gives the same bits; (5) the Python operators and the autograd wrappers reach the ordered
regimes under torch.use_deterministic_algorithms(True) and today's regimes without it.  Every output buffer the entries write is
pre-filled with NaN: an element they skip shows.  All indices are inside their range.  One more float32 case runs the inter operator on
a batch that mixes clouds the on-chip kernel keeps, one it leaves to the product pipeline and an irregular one (MIXED below)."""
import contextlib
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = {'f32': np.float32, 'f64': np.float64}
U32 = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _nan(dev, shape, width):
    return torch.full(shape, float('nan'), dtype=torch.float32 if width == 'f32' else torch.float64, device=dev)


@contextlib.contextmanager
def deterministic(on, warn_only=False):
    """torch.use_deterministic_algorithms(on) for the block; the previous setting AND its warn_only state come back afterwards."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on, warn_only=warn_only)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.are_deterministic_algorithms_enabled() == was and torch.is_deterministic_algorithms_warn_only_enabled() == warn


@contextlib.contextmanager
def recorded_regimes():
    """(entry, regime) of every C entry reached through vgtk._hip.call inside the block; the regime is what eap_last_kernel says right
    after the entry, on the thread that made the call (autograd runs the backward on a thread of its own)"""
    from vgtk import _hip
    seen, real = [], _hip.call

    def spy(name, *args, **kw):
        _hip.abi.eap_last_kernel()                                            # (clear)
        r = real(name, *args, **kw)
        seen.append((name, _hip.abi.eap_last_kernel().decode()))
        return r
    _hip.call = spy
    try:
        yield seen
    finally:
        _hip.call = real


# ---- the sequential evaluations ----------------------------------------------------------------------------------------------
# One function per operator, written over whole arrays of independent outputs but ONE TERM PER STEP along the summation order; the
# arithmetic is NumPy's at the dtype of the operands (float32: every product and every sum rounded to float32; int64: exact).
def seq_gather(idx, g, n):
    b, c, m = g.shape
    out = np.zeros((b, c, n), g.dtype)
    for j in range(m):
        out[np.arange(b), :, idx[:, j]] += g[:, :, j]
    return out


def seq_intra(idx, w, g, na_in):
    b, c, ks, np_, na_out = g.shape
    out = np.zeros((b, c, np_, na_in), g.dtype)
    for a in range(na_out):
        for k in range(ks):
            for n in range(idx.shape[1]):
                out[:, :, :, idx[a, n]] += g[:, :, k, :, a] * w[a, k, n]
    return out


def seq_inter(idx, w, g, nq):
    b, np_, na, ks, ann = idx.shape
    c = g.shape[1]
    out = np.zeros((b, c, nq, na), g.dtype)
    B, A = np.arange(b)[:, None], np.arange(na)[None, :]
    for p in range(np_):
        for k in range(ks):
            for n in range(ann):
                term = g[:, :, k, p, :] * w[:, p, :, k, n][:, None, :]          # [b, c, na], rounded at the operand width
                out[B, :, idx[:, p, :, k, n], A] += term.transpose(0, 2, 1)     # (one target per (cloud, anchor): no repeats)
    return out


def expectations(seq, idx, w, g, n, width):
    """-> dict of what the checks compare with, for float operands (w may be None: the gather has no weights)"""
    ops = lambda f: seq(idx, *( [f(w)] if w is not None else []), f(g), n)
    out = {'ordered': ops(lambda x: x)}
    if width == 'f32':
        out['f64'] = ops(lambda x: x.astype(np.float64))
        out['abs'] = ops(lambda x: np.abs(x.astype(np.float64)))
        out['terms'] = ops(lambda x: np.ones(x.shape, np.int64))
    return out


def check_float(name, got, want, width):
    got = got.cpu().numpy()
    assert not np.isnan(got).any(), f'{name}: the entry left output elements unwritten'
    differ = got != want['ordered']
    print(f'ORDERED {name} {width} elements off the documented order: {int(differ.sum())} of {got.size}')
    assert not differ.any(), f'{name}: not the documented order ({int(differ.sum())} of {got.size} elements differ in their bits)'
    if width == 'f32':
        bound = (want['terms'] + 1) * U32 * want['abs']
        err = np.abs(got.astype(np.float64) - want['f64'])
        print(f'ORDERED {name} f32 worst error / bound: {float((err / np.maximum(bound, 1e-300)).max()):.3g}')
        assert (err <= bound).all(), name


def int_operands(rng, shape, lo, hi, dtype):
    return rng.integers(lo, hi + 1, shape).astype(dtype)


# ---- gather ------------------------------------------------------------------------------------------------------------------
GATHER_CASES = {'n37': (2, 5, 37, 150), 'n1': (2, 5, 1, 150)}


@functools.lru_cache(maxsize=None)
def gather_case(case, width):
    b, c, n, m = GATHER_CASES[case]
    rng = np.random.default_rng(37 + n)
    idx = np.zeros((b, m), np.int32)
    if n > 1:
        # cloud 0: rows 5 and 31 .. 36 are never named, row 3 is named 70 times (more than a wavefront); cloud 1 names row 36 alone, m times
        pool = np.array([q for q in range(31) if q != 5], np.int32)
        idx[0] = rng.choice(pool, m)
        idx[0, rng.choice(m, 70, replace=False)] = 3
        idx[1] = 36
        assert (idx[0] == 3).sum() > 64 and not np.isin(idx[0], [5] + list(range(31, 37))).any()
    g = rng.standard_normal((b, c, m)).astype(WIDTHS[width])
    gi = int_operands(rng, (b, c, m), -9, 9, WIDTHS[width])
    return idx, g, gi, expectations(seq_gather, idx, None, g, n, width), seq_gather(idx, gi.astype(np.int64), n)


def run_gather(dev, width, idx, g, n):
    from vgtk import _hip
    d_idx, d_g = _dev(dev, idx, g)
    b, c, m = g.shape
    lists = _hip.inv_lists(d_idx.view(b, m, 1), n)
    out = _nan(dev, (b, c, n), width)
    _hip.abi.eap_last_kernel()
    _hip.call('eap_gather_points_bwd_ordered_' + width, out, b, c, n, m, d_g, *lists, out)
    assert _hip.abi.eap_last_kernel().decode() == 'gather_points_bwd_ordered'
    return out


@pytest.mark.parametrize('width', list(WIDTHS))
@pytest.mark.parametrize('case', list(GATHER_CASES))
def test_gather_ordered(dev, case, width):
    n = GATHER_CASES[case][2]
    idx, g, gi, want, exact = gather_case(case, width)
    out = run_gather(dev, width, idx, g, n)
    check_float(f'gather {case}', out, want, width)
    assert torch.equal(out, run_gather(dev, width, idx, g, n)), 'a second call gave other bits'
    got = run_gather(dev, width, idx, gi, n).cpu().numpy()
    assert np.array_equal(got.astype(np.int64), exact) and np.array_equal(got, exact.astype(got.dtype))
    # the Python operator, asked for the ordered kernel, is this entry
    import vgtk.cuda.gathering as G
    d_idx, d_g = _dev(dev, idx, g)
    assert torch.equal(G.gather_points_backward(d_g, d_idx, n, ordered=True), out)


# ---- intra -------------------------------------------------------------------------------------------------------------------
# (na_in, na_out, ann, ks, b, c, np): the small table with 35 points (a block serves 32 points: a full block and a second with 3)
INTRA_CASES = {'7x5': (7, 5, 3, 2, 2, 3, 35), '60x60': (60, 60, 12, 24, 2, 3, 5)}


@functools.lru_cache(maxsize=None)
def intra_case(case, width):
    na_in, na_out, ann, ks, b, c, np_ = INTRA_CASES[case]
    rng = np.random.default_rng(na_in)
    if case == '7x5':
        # input anchor 6 is never named; input anchor 2 is named by every output anchor (the first entry of every row of the table)
        idx = rng.integers(0, 6, (na_out, ann)).astype(np.int32)
        idx[:, 0] = 2
        assert not (idx == 6).any() and (idx == 2).any(axis=1).all()
    else:
        idx = rng.integers(0, na_in, (na_out, ann)).astype(np.int32)
    dt = WIDTHS[width]
    w, g = rng.standard_normal((na_out, ks, ann)).astype(dt), rng.standard_normal((b, c, ks, np_, na_out)).astype(dt)
    wi, gi = int_operands(rng, w.shape, -3, 3, dt), int_operands(rng, g.shape, -4, 4, dt)
    return idx, w, g, wi, gi, expectations(seq_intra, idx, w, g, na_in, width), seq_intra(idx, wi.astype(np.int64), gi.astype(np.int64), na_in)


def run_intra(dev, width, idx, w, g, na_in):
    from vgtk import _hip
    d_idx, d_w, d_g = _dev(dev, idx, w, g)
    b, c, ks, np_, na_out = g.shape
    out = _nan(dev, (b, c, np_, na_in), width)
    _hip.abi.eap_last_kernel()
    _hip.call('eap_intra_zpconv_bwd_ordered_' + width, out, b, np_, na_in, na_out, ks, idx.shape[1], c, d_idx, d_w, d_g, out)
    assert _hip.abi.eap_last_kernel().decode() == 'intra_zpconv_bwd_ordered'
    return out


@pytest.mark.parametrize('width', list(WIDTHS))
@pytest.mark.parametrize('case', list(INTRA_CASES))
def test_intra_ordered(dev, case, width):
    na_in = INTRA_CASES[case][0]
    idx, w, g, wi, gi, want, exact = intra_case(case, width)
    out = run_intra(dev, width, idx, w, g, na_in)
    check_float(f'intra {case}', out, want, width)
    assert torch.equal(out, run_intra(dev, width, idx, w, g, na_in)), 'a second call gave other bits'
    got = run_intra(dev, width, idx, wi, gi, na_in).cpu().numpy()
    assert np.array_equal(got.astype(np.int64), exact) and np.array_equal(got, exact.astype(got.dtype))
    import vgtk.cuda.zpconv as Z
    d_idx, d_w, d_g = _dev(dev, idx, w, g)
    assert torch.equal(Z.intra_zpconv_backward(d_idx, d_w, d_g, na_in, ordered=True), out)


# ---- inter -------------------------------------------------------------------------------------------------------------------
# (b, np, nq, na, ks, ann, c, one list per point)
INTER_CASES = {'irregular': (2, 9, 11, 4, 3, 5, 5, False), 'shared': (2, 9, 11, 4, 3, 5, 5, True), 'strides': (2, 8, 9, 60, 24, 64, 3, False)}


@functools.lru_cache(maxsize=None)
def inter_case(case, width):
    b, np_, nq, na, ks, ann, c, shared = INTER_CASES[case]
    rng = np.random.default_rng(nq + na + shared)
    # (the last support row is never named: it must come back as zeros)
    if shared:
        idx = np.broadcast_to(rng.integers(0, nq - 1, (b, np_, 1, 1, ann)), (b, np_, na, ks, ann)).astype(np.int32)
    else:
        idx = rng.integers(0, nq - 1, (b, np_, na, ks, ann)).astype(np.int32)
    dt = WIDTHS[width]
    w, g = rng.standard_normal(idx.shape).astype(dt), rng.standard_normal((b, c, ks, np_, na)).astype(dt)
    wi, gi = int_operands(rng, w.shape, -3, 3, dt), int_operands(rng, g.shape, -4, 4, dt)
    return idx, w, g, wi, gi, expectations(seq_inter, idx, w, g, nq, width), seq_inter(idx, wi.astype(np.int64), gi.astype(np.int64), nq)


def run_inter(dev, width, idx, w, g, nq):
    from vgtk import _hip
    d_idx, d_w, d_g = _dev(dev, idx, w, g)
    b, np_, na, ks, ann = idx.shape
    c = g.shape[1]
    ws = torch.empty((int(_hip.abi.eap_inter_zpconv_bwd_ordered_workspace(b, np_, nq, na, ks, ann)) + 3) // 4, dtype=torch.int32, device=dev)
    out = _nan(dev, (b, c, nq, na), width)
    _hip.abi.eap_last_kernel()
    _hip.call('eap_inter_zpconv_bwd_ordered_' + width, out, b, np_, nq, na, ks, ann, c, d_idx, d_w, d_g, out, ws)
    assert _hip.abi.eap_last_kernel().decode() == 'zpconv_bwd_ordered'
    return out


@pytest.mark.parametrize('width', list(WIDTHS))
@pytest.mark.parametrize('case', list(INTER_CASES))
def test_inter_ordered(dev, case, width, monkeypatch):
    nq = INTER_CASES[case][2]
    idx, w, g, wi, gi, want, exact = inter_case(case, width)
    if case == 'strides':
        assert want['ordered'].shape == (2, 3, 9, 60) and np.bincount(idx[0, :, 0].ravel()).max() > 64      # a list longer than a wavefront
    out = run_inter(dev, width, idx, w, g, nq)
    assert (out[:, :, nq - 1] == 0).all(), 'the row nothing names is not zero'
    check_float(f'inter {case}', out, want, width)
    assert torch.equal(out, run_inter(dev, width, idx, w, g, nq)), 'a second call gave other bits'
    got = run_inter(dev, width, idx, wi, gi, nq).cpu().numpy()
    assert np.array_equal(got.astype(np.int64), exact) and np.array_equal(got, exact.astype(got.dtype))
    # the Python operator, asked for the ordered kernel: these sizes are outside the float32 on-chip kernel and product pipeline, so
    # every cloud reaches this entry at either width -- in one call, and in one-cloud slices when the scratch bound is a cloud's worth
    import vgtk.cuda.zpconv as Z
    from vgtk import _hip
    d_idx, d_w, d_g = _dev(dev, idx, w, g)
    default_bound = Z.BWD_WORKSPACE_BYTES
    for bound in (default_bound, int(_hip.abi.eap_inter_zpconv_bwd_ordered_workspace(1, *idx.shape[1:2], nq, *idx.shape[2:]))):
        monkeypatch.setattr(Z, 'BWD_WORKSPACE_BYTES', bound)
        with recorded_regimes() as seen:
            assert torch.equal(Z.inter_zpconv_backward(d_idx, d_w, d_g, nq, ordered=True), out)
        entries = [name for name, _ in seen if name.startswith('eap_inter_zpconv_bwd')]
        assert entries == ['eap_inter_zpconv_bwd_ordered_' + width] * (1 if bound == default_bound else idx.shape[0]), entries


# ---- inter, float32, where the atomics-free paths of the default route keep their clouds ---------------------------------------
# (b, np, nq, na, ks, ann, c): the sizes the on-chip kernel takes (ks = 24, ann = 64, na % 4 == 0, c % 32 == 0) and the product pipeline
# with them.  One list per point in clouds 0, 1 and 3; cloud 0 and cloud 3 name 200 support rows (the on-chip kernel serves them), cloud 1
# names 291, one more than the on-chip kernel holds (it leaves the cloud to the product pipeline); cloud 2 is cloud-0-like with ONE entry of
# its 5-D index changed: no longer one list per point, nothing but the ordered kernel serves it without atomics.  So the shared clouds
# come in two runs ([0, 2) and [3, 4)) around the irregular one.
MIXED = (4, 11, 300, 4, 24, 64, 32)


@functools.lru_cache(maxsize=None)
def mixed_case():
    import zpconv_common as ZC
    b, np_, nq, na, ks, ann, c = MIXED
    lists = np.concatenate([ZC.lists_with_rows(1, np_, nq, R, seed) for seed, R in enumerate((200, ZC.HOT_RCAP + 1, 200, 200))])
    idx = ZC.deviate(ZC.broadcast5d(lists, na, ks), (2, np_ - 1, na - 1, ks - 1, ann - 1), nq)
    shared = [bool((idx[i] == idx[i, :, :1, :1, :]).all()) for i in range(b)]
    assert shared == [True, True, False, True]
    rng = np.random.default_rng(291)
    w, g = rng.standard_normal(idx.shape).astype(np.float32), rng.standard_normal((b, c, ks, np_, na)).astype(np.float32)
    wi, gi = int_operands(rng, w.shape, -3, 3, np.float32), int_operands(rng, g.shape, -4, 4, np.float32)
    want = {'f64': ZC.inter_backward(idx, w, g, nq), 'abs': ZC.inter_backward(idx, w, g, nq, absolute=True), 'terms': ZC.inter_backward_T(idx, nq),
            'ordered2': seq_inter(idx[2:3], w[2:3], g[2:3], nq)[0], 'exact': ZC.inter_backward(idx, wi, gi, nq, acc=np.int64)}
    return idx, w, g, wi, gi, want


@pytest.fixture
def _fresh_verdicts():
    import vgtk.cuda.zpconv as Z
    Z._check_pending_verdicts(block=True)
    before = dict(Z._HOT_VERDICTS)
    yield before
    Z._check_pending_verdicts(block=True)


@pytest.mark.parametrize('how', ['ordered=True', 'flag'])
def test_inter_ordered_float32_keeps_the_atomics_free_paths(dev, how, _fresh_verdicts):
    """float32, ordered: the on-chip kernel keeps clouds 0 and 3, the product pipeline cloud 1, the ordered kernel takes cloud 2 -- no scatter
    regime anywhere -- asked for by the keyword and by torch's flag.  Cloud 2 is the documented order bit for bit; every cloud is the int64
    result on integer operands and within 2 T u sum|terms| of float64 on random ones (the bound tests/test_gpu_zpconv_regimes.py holds the
    on-chip kernel and the product pipeline to: they sum partial sums, T roundings of the products and at most T of the sums); a second call
    gives the same bits; the remembered verdicts of the default route are left as they were."""
    import vgtk.cuda.zpconv as Z
    b, np_, nq, na, ks, ann, c = MIXED
    idx, w, g, wi, gi, want = mixed_case()
    d_idx, d_w, d_g, d_wi, d_gi = _dev(dev, idx, w, g, wi, gi)

    def run(weights, grad):
        with deterministic(how == 'flag'), recorded_regimes() as seen:
            out = Z.inter_zpconv_backward(d_idx, weights, grad, nq, ordered=True if how == 'ordered=True' else None)
            torch.cuda.synchronize()
        return out, [(name, regime) for name, regime in seen if name.startswith('eap_inter_zpconv_bwd')]

    out, seen = run(d_w, d_g)
    # run [0, 2): on-chip (leaves cloud 1), pipeline for cloud 1; run [3, 4): on-chip; then cloud 2 to the ordered kernel
    assert seen == [('eap_inter_zpconv_bwd_hot_f32', 'zp_hot_kernel'), ('eap_inter_zpconv_bwd_ws_f32', 'zpconv_bwd_products'),
                    ('eap_inter_zpconv_bwd_hot_f32', 'zp_hot_kernel'), ('eap_inter_zpconv_bwd_ordered_f32', 'zpconv_bwd_ordered')], seen
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got[2], want['ordered2']), 'the irregular cloud is not in the documented order'
    bound = 2.0 * want['terms'] * U32 * want['abs']
    err = np.abs(got.astype(np.float64) - want['f64'])
    print(f'ORDERED inter mixed f32 ({how}) worst error / bound: {float((err / np.maximum(bound, 1e-300)).max()):.3g}')
    assert (err <= bound).all()
    again, seen2 = run(d_w, d_g)
    assert torch.equal(out, again) and seen2 == seen, 'a second call gave other bits or another route'
    exact, _ = run(d_wi, d_gi)
    assert np.array_equal(exact.cpu().numpy().astype(np.int64), want['exact'])
    assert dict(Z._HOT_VERDICTS) == _fresh_verdicts


# ---- routing -----------------------------------------------------------------------------------------------------------------
def _backward_regimes(dev, width, flag):
    """forward and backward of the three autograd wrappers on the small cases -> {wrapper: [(entry, regime)] of its backward}"""
    import vgtk.spconv.functional as F
    tdt = torch.float32 if width == 'f32' else torch.float64
    out = {}
    with deterministic(flag):
        # Gathering: points [b,c,n], idx [b,m]
        idx, g = gather_case('n37', width)[:2]
        pts = torch.randn(2, 5, 37, dtype=tdt, device=dev, requires_grad=True)
        y = F.Gathering.apply(pts, _dev(dev, idx)[0])
        with recorded_regimes() as seen:
            y.backward(_dev(dev, g.astype(np.float32))[0])
        out['gather'] = list(seen)
        assert pts.grad is not None and pts.grad.dtype == tdt
        # IntraZPConvGrouping: idx [na_out,ann], w [na_out,ks,ann], feats [b,c,np,na_in]
        idx, w, g = intra_case('7x5', width)[:3]
        d_idx, d_w, d_g = _dev(dev, idx, w, g)
        feats = torch.randn(2, 3, 35, 7, dtype=tdt, device=dev, requires_grad=True)
        y = F.IntraZPConvGrouping.apply(d_idx, d_w, feats)
        with recorded_regimes() as seen:
            y.backward(d_g)
        out['intra'] = list(seen)
        intra_grad = feats.grad.clone()
        # InterZPConvGrouping: idx, w [b,np,na,ks,ann], feats [b,c,nq,na]
        idx, w, g = inter_case('irregular', width)[:3]
        d_idx, d_w, d_g = _dev(dev, idx, w, g)
        feats = torch.randn(2, 5, 11, 4, dtype=tdt, device=dev, requires_grad=True)
        y = F.InterZPConvGrouping.apply(d_idx, d_w, feats)
        with recorded_regimes() as seen:
            y.backward(d_g)
        out['inter'] = list(seen)
        torch.cuda.synchronize()
    return out, intra_grad, feats.grad.clone()


@pytest.mark.parametrize('width', list(WIDTHS))
def test_wrappers_follow_torchs_flag(dev, width):
    on, intra_on, inter_on = _backward_regimes(dev, width, True)
    assert on['gather'][-1] == ('eap_gather_points_bwd_ordered_f32', 'gather_points_bwd_ordered')        # (the gather's output is float32 at either width)
    assert on['intra'] == [('eap_intra_zpconv_bwd_ordered_' + width, 'intra_zpconv_bwd_ordered')]
    assert on['inter'][-1] == ('eap_inter_zpconv_bwd_ordered_' + width, 'zpconv_bwd_ordered')
    assert not any('scatter' in regime or name.endswith('_bwd_' + width) for seen in on.values() for name, regime in seen), on
    # under the flag the wrappers give the documented order
    assert np.array_equal(intra_on.cpu().numpy(), intra_case('7x5', width)[5]['ordered'])
    assert np.array_equal(inter_on.cpu().numpy(), inter_case('irregular', width)[5]['ordered'])
    off, _, _ = _backward_regimes(dev, width, False)
    assert off['gather'] == [('eap_gather_points_bwd_f32', '')]
    assert off['intra'] == [('eap_intra_zpconv_bwd_' + width, 'intra_zpconv')]
    assert off['inter'][-1][1] == 'zpconv_bwd_scatter' and not any('ordered' in name for name, _ in off['inter']), off


def test_no_ordered_kernel_follows_torchs_contract(dev):
    """more than 16384 target rows: the list builders cannot serve the call -- raise under the flag (or when ordered=True was asked
    for), warn and scatter under warn_only, scatter quietly without the flag"""
    import vgtk.cuda.gathering as G
    n, idx = 16385, torch.tensor([[3, 16384, 3, 0]], dtype=torch.int32, device=dev)
    g = torch.tensor([[[1.0, 2.0, 4.0, 8.0]]], device=dev)
    want = torch.zeros(1, 1, n, device=dev)
    want[0, 0, 0], want[0, 0, 3], want[0, 0, 16384] = 8.0, 5.0, 2.0
    with deterministic(False):
        assert torch.equal(G.gather_points_backward(g, idx, n), want)
        with pytest.raises(RuntimeError, match='gather_points_backward does not have a deterministic implementation'):
            G.gather_points_backward(g, idx, n, ordered=True)
    with deterministic(True):
        with pytest.raises(RuntimeError, match='gather_points_backward does not have a deterministic implementation'):
            G.gather_points_backward(g, idx, n)
        assert torch.equal(G.gather_points_backward(g, idx, n, ordered=False), want)
    with deterministic(True, warn_only=True), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        assert torch.equal(G.gather_points_backward(g, idx, n), want)
    assert any('gather_points_backward does not have a deterministic implementation' in str(x.message) for x in seen)
