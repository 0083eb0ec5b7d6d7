"""GPU: chamfer distance in float64 and the ordered (atomic-free) backward at both widths (csrc/chamfer.hip,
eap_chamfer_fwd_f64 / eap_chamfer_bwd_ordered_f32 / eap_chamfer_bwd_ordered_f64).

Float64 expectations are NumPy restatements computed here on the CPU: the forward is ((dx*dx + dy*dy) + dz*dz) elementwise with
the first arg-min; the backward is, with v1[i] = (g1[i]*2) * (x1[i] - x2[idx1[i]]) and v2[j] = (g2[j]*2) * (x2[j] - x1[idx2[j]]),
    gxyz1[i] = ((0 + v1[i]) + sum over j ascending with idx2[j] == i of (-v2[j]))
    gxyz2[j] = ((0 + sum over i ascending with idx1[i] == j of (-v1[i])) + v2[j])
(np.add.at is unbuffered and adds in index order).  In float32 the same sums are what the serial CPU oracle computes, so the ordered
float32 backward is compared with the oracle bit for bit.  Everything here is exact (assert_array_equal / torch.equal) except where
a tolerance is written next to the assert with its reason."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import native  # noqa: E402  (checker only)

T = torch.from_numpy


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@contextlib.contextmanager
def deterministic(on):
    """torch.use_deterministic_algorithms(on) for the block; the previous setting AND its warn_only state come back afterwards."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.are_deterministic_algorithms_enabled() == was and torch.is_deterministic_algorithms_warn_only_enabled() == warn


@contextlib.contextmanager
def recorded_calls():
    """the names of the C entries reached through vgtk._hip.call inside the block"""
    from vgtk import _hip
    names, real = [], _hip.call

    def spy(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    _hip.call = spy
    try:
        yield names
    finally:
        _hip.call = real


# ---- the NumPy restatements --------------------------------------------------------------------------------------------------
def np_forward(x1, x2):
    """-> dist1, dist2, idx1, idx2 at the width of x1: one rounding per operation, first minimum"""
    def one(a, c):
        dx, dy, dz = (c[:, None, :, k] - a[:, :, None, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz                                 # [b, n, m]
        idx = d.argmin(axis=2)                                            # (first occurrence)
        return np.take_along_axis(d, idx[..., None], 2)[..., 0], idx.astype(np.int32)
    d1, i1 = one(x1, x2)
    d2, i2 = one(x2, x1)
    assert d1.dtype == x1.dtype
    return d1, d2, i1, i2


def np_backward(x1, x2, i1, i2, g1, g2):
    """the two ordered sums of the module docstring, at the width of x1; an index outside its cloud contributes nothing"""
    gx1, gx2 = np.zeros_like(x1), np.zeros_like(x2)
    for b in range(x1.shape[0]):
        ok1 = (i1[b] >= 0) & (i1[b] < x2.shape[1])
        ok2 = (i2[b] >= 0) & (i2[b] < x1.shape[1])
        v1 = np.zeros_like(x1[b]); v2 = np.zeros_like(x2[b])
        v1[ok1] = (g1[b][ok1] * 2)[:, None] * (x1[b][ok1] - x2[b][i1[b][ok1]])
        v2[ok2] = (g2[b][ok2] * 2)[:, None] * (x2[b][ok2] - x1[b][i2[b][ok2]])
        gx1[b] = gx1[b] + v1
        np.add.at(gx1[b], i2[b][ok2], -v2[ok2])
        np.add.at(gx2[b], i1[b][ok1], -v1[ok1])
        gx2[b] = gx2[b] + v2
    assert gx1.dtype == x1.dtype
    return gx1, gx2


# ---- the cases (float64 arrays; the float32 runs use their roundings), built once --------------------------------------------
CASES = ['300x1100', '1100x300', '1x1', 'many_to_one']


@functools.lru_cache(maxsize=None)
def case(name):
    """-> x1, x2, g1, g2 (float64, read-only)"""
    rng = np.random.default_rng(2913)
    if name == 'many_to_one':
        # every point of cloud 1 picks point 7 of cloud 2 (1100 contributions from two tiles), most of cloud 2 receives none
        x1 = rng.standard_normal((2, 1100, 3))
        x2 = 40 + 0.01 * rng.standard_normal((2, 300, 3))
        x2[:, 7] = 0.0
    else:
        n, m = (int(v) for v in name.split('x'))
        b = 1 if n == 1 else 2
        x1, x2 = rng.standard_normal((b, n, 3)), rng.standard_normal((b, m, 3))
    out = (x1, x2, rng.standard_normal(x1.shape[:2]), rng.standard_normal(x2.shape[:2]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, width):
    """-> (x1, x2, g1, g2) at `width`, the forward's (d1, d2, i1, i2) and the ordered backward's (gx1, gx2): float64 from the NumPy
    restatements, float32 from the CPU oracle"""
    dt = np.float64 if width == 'f64' else np.float32
    ins = tuple(np.ascontiguousarray(a.astype(dt)) for a in case(name))
    x1, x2, g1, g2 = ins
    if width == 'f64':
        fwd = np_forward(x1, x2)
        bwd = np_backward(x1, x2, fwd[2], fwd[3], g1, g2)
    else:
        fwd = native.chamfer_forward(x1, x2)
        bwd = native.chamfer_backward(x1, x2, fwd[2], fwd[3], g1, g2)
    return ins, fwd, bwd


def test_numpy_restatement_is_the_oracle_in_float32():
    """the formulas this file states for float64 are, evaluated in float32, the serial oracle bit for bit (no GPU involved)"""
    for name in CASES:
        (x1, x2, g1, g2), fwd, bwd = expected(name, 'f32')
        for got, want in zip(np_forward(x1, x2), fwd):
            np.testing.assert_array_equal(got, want)
        for got, want in zip(np_backward(x1, x2, fwd[2], fwd[3], g1, g2), bwd):
            np.testing.assert_array_equal(got, want)
    (x1, x2, _, _), fwd, _ = expected('many_to_one', 'f32')
    assert (fwd[2] == 7).all() and len(np.unique(fwd[3])) > 1


# ---- 1. forward, float64, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['300x1100', '1100x300', '1x1'])
def test_forward_f64_exact(dev, name):
    import chamfer
    (x1, x2, _, _), want, _ = expected(name, 'f64')
    got = chamfer.forward(T(x1).to(dev), T(x2).to(dev))
    assert [t.dtype for t in got] == [torch.float64, torch.float64, torch.int32, torch.int32]
    for g, w in zip(got, want):
        assert tuple(g.shape) == w.shape
        np.testing.assert_array_equal(g.cpu().numpy(), w)


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------
def test_ties_f64(dev):
    """the hand-derived known answers of tests/test_oracle_native.py in float64, and a tie across THIS kernel's 1024-point tile"""
    import chamfer
    import test_oracle_native as K

    def in_f64(fn):
        def run(*args):
            conv = [T(np.ascontiguousarray(a.astype(np.float64) if a.dtype.kind == 'f' else a)).to(dev) for a in args]
            return [o.cpu().numpy() for o in fn(*conv)]
        return run

    K.known_chamfer(in_f64(chamfer.forward), in_f64(chamfer.backward))
    for dt in (np.float64, np.float32):
        big = np.full((1, 1100, 3), 50.0, dt)
        big[0, 5] = [2, 0, 0]
        big[0, 1030] = [-2, 0, 0]
        d1, _, i1, _ = chamfer.forward(T(np.zeros((1, 1, 3), dt)).to(dev), T(big).to(dev))
        assert i1.item() == 5 and d1.item() == 4.0


# ---- 3. / 4. the ordered backward, exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('width', ['f32', 'f64'])
def test_ordered_backward_exact(dev, name, width):
    """called directly and through ChamferFunction (float32: under torch.use_deterministic_algorithms(True)); float32 against the CPU
    oracle, float64 against the NumPy restatement"""
    import chamfer
    from extensions.chamfer_dist import ChamferFunction
    (x1, x2, g1, g2), fwd, want = expected(name, width)
    t1, t2, tg1, tg2 = (T(a).to(dev) for a in (x1, x2, g1, g2))
    with recorded_calls() as names:
        got = chamfer.backward(t1, t2, T(fwd[2]).to(dev), T(fwd[3]).to(dev), tg1, tg2, ordered=True)
    assert names == ['eap_chamfer_bwd_ordered_' + width]
    for g, w in zip(got, want):
        assert g.dtype == t1.dtype and torch.equal(g.cpu(), T(w))
    with deterministic(width == 'f32'), recorded_calls() as names:
        a1, a2 = t1.clone().requires_grad_(True), t2.clone().requires_grad_(True)
        d1, d2 = ChamferFunction.apply(a1, a2)
        torch.autograd.backward([d1, d2], [tg1, tg2])
    assert names == ['eap_chamfer_fwd_' + width, 'eap_chamfer_bwd_ordered_' + width]
    np.testing.assert_array_equal(d1.detach().cpu().numpy(), fwd[0])
    assert torch.equal(a1.grad.cpu(), T(want[0])) and torch.equal(a2.grad.cpu(), T(want[1]))


@pytest.mark.parametrize('width', ['f32', 'f64'])
def test_ordered_backward_ignores_indices_outside_the_cloud(dev, width):
    """an index outside [0, m) contributes nothing (and is not dereferenced): the NumPy restatement with those entries left out"""
    import chamfer
    (x1, x2, g1, g2), fwd, _ = expected('300x1100', width)
    i1, i2 = fwd[2].copy(), fwd[3].copy()
    i1[0, 3], i1[1, 299], i2[0, 0], i2[1, 1050] = -1, x2.shape[1], x1.shape[1], -7
    want = np_backward(x1, x2, i1, i2, g1, g2)
    got = chamfer.backward(*(T(a).to(dev) for a in (x1, x2, i1, i2, g1, g2)), ordered=True)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


# ---- 5. run to run ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', ['f32', 'f64'])
def test_backward_is_bit_identical_run_to_run(dev, width):
    from extensions.chamfer_dist import ChamferFunction
    (x1, x2, g1, g2), _, _ = expected('many_to_one', width)
    runs = []
    with deterministic(width == 'f32'):
        for _ in range(2):
            a1, a2 = T(x1).to(dev).requires_grad_(True), T(x2).to(dev).requires_grad_(True)
            torch.autograd.backward(list(ChamferFunction.apply(a1, a2)), [T(g1).to(dev), T(g2).to(dev)])
            runs.append((a1.grad, a2.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- 6. the default is untouched --------------------------------------------------------------------------------------------
def test_default_float32_backward_is_still_the_scatter(dev):
    from extensions.chamfer_dist import ChamferFunction
    (x1, x2, g1, g2), _, want = expected('many_to_one', 'f32')
    with deterministic(False), recorded_calls() as names:
        a1, a2 = T(x1).to(dev).requires_grad_(True), T(x2).to(dev).requires_grad_(True)
        torch.autograd.backward(list(ChamferFunction.apply(a1, a2)), [T(g1).to(dev), T(g2).to(dev)])
    assert names == ['eap_chamfer_fwd_f32', 'eap_chamfer_bwd_f32']
    e1, e2 = rel_err(a1.grad.cpu().numpy(), want[0]), rel_err(a2.grad.cpu().numpy(), want[1])
    print(f'scatter backward against the oracle: {e1:.3e}, {e2:.3e}')
    assert e1 < 1e-5 and e2 < 1e-5            # the bar of tests/test_gpu_parity.py::test_chamfer


# ---- 7. the reference's own test --------------------------------------------------------------------------------------------
def test_reference_gradcheck(dev):
    """extensions/chamfer_dist/test.py of the reference: gradcheck of ChamferFunction.apply on [4,64,3] / [4,128,3] in double, default
    tolerances (its reentrancy check has nondet_tol = 0: the backward must be bit-identical run to run).  Chamfer is piecewise
    differentiable only: the clouds must keep every nearest neighbour through gradcheck's 1e-6 perturbations, asserted first."""
    from extensions.chamfer_dist import ChamferFunction
    g = torch.Generator().manual_seed(2913)
    x = torch.randn(4, 64, 3, dtype=torch.float64, generator=g)
    y = torch.randn(4, 128, 3, dtype=torch.float64, generator=g)
    d = (x[:, :, None] - y[:, None]).square().sum(-1)
    for dim in (2, 1):
        two = d.topk(2, dim=dim, largest=False).values
        gap = (two.select(dim, 1) - two.select(dim, 0)).min().item()
        print(f'smallest gap between nearest and second nearest (direction {3 - dim}): {gap:.3e}')
        assert gap >= 1e-4
    x, y = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(ChamferFunction.apply, (x, y))


# ---- 8. above the function --------------------------------------------------------------------------------------------------
def test_chamfer_distance_f64(dev):
    from extensions.chamfer_dist import ChamferDistance
    (x1, x2, _, _), (d1, d2, _, _), _ = expected('300x1100', 'f64')
    loss = ChamferDistance()(T(x1).to(dev), T(x2).to(dev))
    want = d1.mean() + d2.mean()
    assert loss.dtype == torch.float64
    assert abs(loss.item() - want) <= 1e-12 * abs(want)      # two means of positive terms: a few hundred roundings of 1.1e-16 at worst
    raw = ChamferDistance()(T(x1).to(dev), T(x2).to(dev), return_raw=True)
    np.testing.assert_array_equal(raw[0].cpu().numpy(), d1)
    # ignore_zeros: one pair, zero-padded rows are dropped first
    p1, p2 = x1[:1, :50].copy(), x2[:1, :70].copy()
    p1[0, 40:] = 0.0
    p2[0, 50:] = 0.0
    e1, e2, _, _ = np_forward(p1[:, :40], p2[:, :50])
    want = e1.mean() + e2.mean()
    loss = ChamferDistance(ignore_zeros=True)(T(p1).to(dev), T(p2).to(dev))
    assert loss.dtype == torch.float64 and abs(loss.item() - want) <= 1e-12 * abs(want)
    padded = ChamferDistance()(T(p1).to(dev), T(p2).to(dev)).item()
    assert abs(padded - want) > 1e-3 * abs(want)             # (the padding does change the plain distance: the flag was exercised)


def test_orbit_reconstruction_distances_f64(dev):
    """B = 1, S = 2, A = 4, M = 16, N = 40 in float64 against the reference's materialised [B,S,A,M,N] expression (oracle/orbit_ref.py) in
    float64 torch on the CPU, as tests/test_gpu_parity.py states it for float32.  Outputs: 1e-12 relative per element (each is a sum of
    three squares, or a mean of 16 such minima: positive terms, a few tens of roundings of 1.1e-16; the 99999 constants are exact).
    Gradient: 1e-10 of its largest magnitude (its elements are signed sums and may cancel)."""
    from extensions.chamfer_dist import orbit_reconstruction_distances
    from oracle import orbit_ref
    b, s, a, m, n = 1, 2, 4, 16, 40
    gen = torch.Generator().manual_seed(9)
    recon = torch.randn(b, s, a, m, 3, dtype=torch.float64, generator=gen) * 0.3
    ori = torch.randn(b, 3, n, dtype=torch.float64, generator=gen) * 0.3
    slot = torch.randint(0, s, (b, n), generator=gen)
    assert 0 < slot.sum().item() < n                                   # both slots hold points
    labels = torch.nn.functional.one_hot(slot, s).double()           # [B,N,S]
    rc = recon.clone().requires_grad_(True)
    want = orbit_ref.orbit_reconstruction_distances(rc, ori, labels)
    rg = recon.clone().to(dev).requires_grad_(True)
    got = orbit_reconstruction_distances(rg, ori.to(dev), labels.to(dev))
    assert any((v.detach() > 9e4).any() for v in want)                 # the masked constant is among the outputs
    for u, v in zip(got, want):
        assert u.shape == v.shape and u.dtype == torch.float64
        np.testing.assert_allclose(u.detach().cpu().numpy(), v.detach().numpy(), rtol=1e-12, atol=0)
    wts = [torch.randn(v.shape, dtype=torch.float64, generator=gen) for v in want]
    finite = [torch.where(v.detach() < 9e4, w, torch.zeros_like(w)) for v, w in zip(want, wts)]   # constants carry no gradient
    sum((v * w).sum() for v, w in zip(want, finite)).backward()
    sum((u * w.to(dev)).sum() for u, w in zip(got, finite)).backward()
    assert rg.grad.dtype == torch.float64
    err = rel_err(rg.grad.cpu().numpy(), rc.grad.numpy())
    print(f'orbit gradient, float64: {err:.3e}')
    assert err <= 1e-10


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import chamfer
    from extensions.chamfer_dist import ChamferFunction
    x32 = torch.zeros(1, 4, 3, device=dev)
    x64 = torch.zeros(1, 5, 3, device=dev, dtype=torch.float64)
    for pair in ((x32, x64), (x64, x32), (x32.half(), x32.half()), (x32.bfloat16(), x32.bfloat16()), (x64.cpu(), x64.cpu()), (x32, x32.cpu())):
        with pytest.raises(RuntimeError):
            chamfer.forward(*pair)
        with pytest.raises(RuntimeError):
            ChamferFunction.apply(*pair)
    i4 = torch.zeros(1, 4, dtype=torch.int32, device=dev)
    i5 = torch.zeros(1, 5, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):                                  # gradients in another width than the clouds
        chamfer.backward(x64[:, :4], x64, i4, i5, x32[..., 0], x64[..., 0].contiguous())
    with pytest.raises(RuntimeError):                                  # float64 has no scatter
        chamfer.backward(x64[:, :4].contiguous(), x64, i4, i5, x64[:, :4, 0].contiguous(), x64[..., 0].contiguous(), ordered=False)
