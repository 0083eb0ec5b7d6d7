"""CPU: the host logic and the arithmetic of the conv + BatchNorm + leaky_relu node (vgtk/so3conv/functional.py TrainEpilogue; kernels
csrc/bn_act.hip bn_act_bwd_reduce_fromy_kernel, csrc/so3_dense.hip dense_split_kernel<true> / dense_untranspose_kernel) against torch's own
BatchNorm2d + leaky_relu and its autograd (`feat = self.norm(x.feats); feat = self.relu(feat)`, SPConvNets/utils/base_so3poseconv.py:L214-221):
  * TrainEpilogue.moments: scale / shift from pivoted sums, running statistics as nn.BatchNorm2d updates them;
  * the backward FROM THE OUTPUT: pre-activation and xhat recovered from y' (also with a negative gamma), gx = k1 g - k2 - k3 xhat, the row
    bound |k1| max|g| + |k2| + |k3| max|xhat| really bounds |gx|;
  * the same backward in FLOAT32, as the two kernels evaluate it, against float64 PER CHANNEL as r = |beta / gamma| and m = |mean| invstd of
    the conv output grow: the derivation of the 8u bound (test_float32_recovery_per_channel) that the GPU tests of
    tests/test_gpu_conv_norm_conditioning.py hold the kernels and the node to, and of the limit R = 128 past which a layer keeps the
    separate norm module.
The GPU tests compare the kernels with the separate modules; this file pins the formulas those kernels implement."""
import pytest
import torch
import torch.nn.functional as F


def _case(seed=3, b=3, c=5, p=7, a=4):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, p, a, generator=gen, dtype=torch.float64) * 2.0 + torch.randn(1, c, 1, 1, generator=gen, dtype=torch.float64)
    gamma = torch.rand(c, generator=gen, dtype=torch.float64) + 0.5
    gamma[1] = -0.8
    beta = torch.randn(c, generator=gen, dtype=torch.float64) * 0.3
    return x, gamma, beta


def test_moments_give_the_batchnorm_affine_map_and_running_statistics():
    import vgtk.so3conv as sptk
    from vgtk.so3conv.functional import TrainEpilogue
    x, gamma, beta = _case()
    b, c = x.shape[:2]
    norm = sptk.BatchNormLeakyReLU(c, negative_slope=0.01)
    ref = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        for m in (norm, ref):
            m.weight.copy_(gamma.float()); m.bias.copy_(beta.float())
            m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 1.5)
        ref.running_mean.copy_(norm.running_mean); ref.running_var.copy_(norm.running_var)
    pivot = x[0, :, 0, 0].clone()
    d = x - pivot[None, :, None, None]
    ep = TrainEpilogue(norm)
    scale, shift, slope = ep.moments(d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), pivot, b * x.shape[2] * x.shape[3])
    ref.train()
    want = F.leaky_relu(ref(x.float()), 0.01)
    got = F.leaky_relu(x.float() * scale[None, :, None, None] + shift[None, :, None, None], slope)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)
    assert torch.allclose(norm.running_mean, ref.running_mean, rtol=1e-6, atol=1e-6) and torch.allclose(norm.running_var, ref.running_var, rtol=1e-6, atol=1e-6)
    k1, beta_s, inv_gamma, total = ep.saved
    assert total == b * x.shape[2] * x.shape[3] and torch.allclose(beta_s.double(), beta, atol=1e-6)
    assert torch.allclose(inv_gamma.double() * gamma, torch.ones(c, dtype=torch.float64), atol=1e-6)


@pytest.mark.parametrize('slope', [0.01, 0.2])
def test_backward_from_the_output_equals_autograd(slope):
    x, gamma, beta = _case(seed=9)
    x = x.requires_grad_(True)
    g_ = gamma.clone().requires_grad_(True)
    b_ = beta.clone().requires_grad_(True)
    y = F.leaky_relu(F.batch_norm(x, None, None, g_, b_, True, 0.0, 1e-5), slope)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    gx_ref, gg_ref, gb_ref = torch.autograd.grad(y, [x, g_, b_], gy)
    # what the node does, from y' alone
    with torch.no_grad():
        yv = y.detach()
        n = x.numel() // x.shape[1]
        mean = x.mean((0, 2, 3)); var = x.var((0, 2, 3), unbiased=False)
        invstd = torch.rsqrt(var + 1e-5)
        k1 = gamma * invstd
        bc = lambda t: t[None, :, None, None]
        pos = yv > 0
        pre = torch.where(pos, yv, yv / slope)
        xhat = (pre - bc(beta)) / bc(gamma)
        g = torch.where(pos, gy, gy * slope)
        sg, sgx = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
        k2, k3 = k1 * sg / n, k1 * sgx / n
        gx = bc(k1) * g - bc(k2) - bc(k3) * xhat
        assert torch.allclose(xhat, (x.detach() - bc(mean)) * bc(invstd), atol=1e-9)           # the pre-activation IS recoverable (negative gamma too)
        assert torch.allclose(gx, gx_ref, atol=1e-10) and torch.allclose(sgx, gg_ref, atol=1e-9) and torch.allclose(sg, gb_ref, atol=1e-9)
        # the row bound of the stored-operand split (per cloud, channel, anchor over the points)
        gmax, xmax = g.abs().amax(2), xhat.abs().amax(2)                                   # [b,c,a]
        bound = k1.abs()[None, :, None] * gmax + k2.abs()[None, :, None] + k3.abs()[None, :, None] * xmax
        assert bool((gx.abs().amax(2) <= bound * (1 + 1e-12)).all())


# ---- the float32 recovery, per channel -------------------------------------------------------------------------------------------------
# In float32 the recovery xhat = ((y' > 0 ? y' : y' / slope) - beta) / gamma subtracts two numbers of size |beta| to get one of size
# |gamma xhat|: the absolute error of the recovered xhat grows with r = |beta / gamma|, and -- through the rounded shift = beta - mean scale
# -- with m = |mean| invstd of the conv output.  With u = 2^-24 (half an ulp of 1) the roundings on the path from the conv output x to the
# recovered xhat, each relative to the value it rounds, expressed in units of xhat (that is, divided by |gamma|):
#   1  scale = fl(gamma invstd):         u |x scale| / |gamma| = u |xhat + mean invstd|          <= u (|xhat| + m)
#   2  shift = fl(beta - mean scale):    u |shift| / |gamma|                                     <= u (r + m)
#   3  the fma's one rounding:           u |gamma xhat + beta| / |gamma|                         <= u (|xhat| + r)
#   4  y' = fl(pre slope) (pre < 0)      u |pre slope| / (slope |gamma|)                         <= u (|xhat| + r)
#   5  inv_slope = fl(1 / slope)         u |pre| / |gamma|                                       <= u (|xhat| + r)
#   6  fl(y' inv_slope)                  the same
#   7  fl(pre - beta)                    u |gamma xhat| / |gamma| = u |xhat|  (exact where pre and beta are within a factor 2: Sterbenz)
#   8  inv_gamma = fl(1 / gamma)         u |xhat|
#   9  fl((pre - beta) inv_gamma)        u |xhat|
# Nine, of which 7 is exact or nearly so wherever r matters: |xhat_rec - xhat| <= 8u (|xhat| + r + m).  The sums and gx follow by the
# triangle inequality (bounds()).  The float32 ACCUMULATION of the two sums is not among the nine: its error is no function of r or m, and
# the kernel's blocks hand float32 partials of at most 64 terms per thread to a float64 sum; the test shows that it stays inside the same
# constant at these sizes.
U = 2.0 ** -24
R_LIMIT = 128.0            # vgtk.so3conv.functional.NORM_IN_NODE_MAX_RATIO: past it a layer keeps the separate norm module
# (gamma, beta) per channel: r = 0, 0.3, 2, 0.43, 8, 64, 64, 128, 500, 500 (negative gamma), 3e4; the last entry is the channel whose conv
# output has |mean| invstd ~ 30 (MEANS below)
TABLE = [(1.0, 0.0), (1.0, 0.3), (0.5, 1.0), (-0.7, 0.3), (1.0, 8.0), (1.0, 64.0), (0.01, 0.64), (1.0, 128.0), (1e-3, 0.5), (-1e-3, 0.5),
         (1e-5, 0.3), (1.0, 0.3)]
MEANS = [0.3, -0.2, 0.1, 0.4, -0.3, 0.2, -0.1, 0.3, 0.2, -0.4, 0.1, 30.0]      # mean of the conv output per channel (its deviation is ~1)
SLOPES = [0.01, 0.2, 1.0]


def table(c, device='cpu'):
    """-> gamma, beta, mean float64 [c]: TABLE and MEANS, repeated up to c channels"""
    g = torch.tensor([TABLE[i % len(TABLE)][0] for i in range(c)], dtype=torch.float64, device=device)
    b = torch.tensor([TABLE[i % len(TABLE)][1] for i in range(c)], dtype=torch.float64, device=device)
    m = torch.tensor([MEANS[i % len(MEANS)] for i in range(c)], dtype=torch.float64, device=device)
    return g, b, m


def _ch(t):
    return t[None, :, None]


def emulate_forward(x, gamma, beta, slope, eps=1e-5):
    """What the node's forward stores, in float32 as the kernels form it.  x float32 [b,c,n] = the conv output; gamma, beta float64 [c] (the
    float32 parameters as doubles).  Moments in float64 (TrainEpilogue.moments), scale and shift rounded to float32, one fma per element
    (formed in float64 and rounded), float32 product with the slope.
    -> dict: yact float32 = y'; scale, shift, beta, inv_gamma float32 [c]; mean, invstd, xhat float64 (the true ones of this x)"""
    xd = x.double()
    mean, var = xd.mean((0, 2)), xd.var((0, 2), unbiased=False)
    invstd = torch.rsqrt(var + eps)
    scale = (gamma * invstd).float()
    shift = (beta - mean * (gamma * invstd)).float()
    pre = (xd * _ch(scale.double()) + _ch(shift.double())).float()
    yact = torch.where(pre > 0, pre, pre * torch.tensor(slope, dtype=torch.float32, device=x.device))
    inv_gamma = torch.where(gamma == 0, torch.zeros_like(gamma), 1.0 / gamma).float()
    return {'yact': yact, 'scale': scale, 'shift': shift, 'beta': beta.float(), 'inv_gamma': inv_gamma, 'mean': mean, 'invstd': invstd,
            'xhat': (xd - _ch(mean)) * _ch(invstd), 'count': x.shape[0] * x.shape[2]}


def emulate_backward(fw, gy, slope):
    """The node's backward from y' in float32: bn_act_bwd_reduce_fromy_kernel's recovery and sums, the host's k2 / k3 (float64 arithmetic on
    the sums, rounded to float32), dense_split_kernel<true>'s gx = fma(g, k1, -k2) - xhat k3.
    -> dict: pos bool, g, xhat, gx float32 [b,c,n]; sg, sgx float64 [c]; k1, k2, k3 float32 [c]"""
    yact, be, ig, k1 = fw['yact'], fw['beta'], fw['inv_gamma'], fw['scale']
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=yact.device)
    inv_slope = f32(1.0) / f32(slope)                                  # float32(1 / slope), as the entry forms it
    pos = yact > 0
    g = torch.where(pos, gy, gy * f32(slope))
    xhat = (torch.where(pos, yact, yact * inv_slope) - _ch(be)) * _ch(ig)
    sg = g.sum((0, 2), dtype=torch.float32).double()
    sgx = (g * xhat).sum((0, 2), dtype=torch.float32).double()
    k2 = (k1.double() * sg / fw['count']).float()
    k3 = (k1.double() * sgx / fw['count']).float()
    gx = ((g.double() * _ch(k1.double()) - _ch(k2.double())).float() - xhat * _ch(k3))
    return {'pos': pos, 'g': g, 'xhat': xhat, 'gx': gx, 'sg': sg, 'sgx': sgx, 'k1': k1, 'k2': k2, 'k3': k3}


def float64_reference(x, gamma, beta, gy, slope, eps=1e-5, pos=None):
    """float64 autograd of leaky_relu(batch_norm(x)) for x [b,c,n] -> dict: y, pre, gx [b,c,n]; dgamma, dbeta, k1, k2, k3 [c]; g [b,c,n].
    pos bool [b,c,n]: the side of the kink every element is on, where a float32 forward has decided that already (an element whose
    pre-activation is within that forward's rounding of 0 has two right answers; the caller checks that pos differs from pre > 0 only there)"""
    xd = x.double().requires_grad_(True)
    g_, b_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    pre = F.batch_norm(xd, None, None, g_, b_, True, 0.0, eps)
    side = (pre.detach() > 0) if pos is None else pos
    y = pre * torch.where(side, 1.0, slope).to(pre.dtype)                  # leaky_relu, the decisions given
    gx, dgamma, dbeta = torch.autograd.grad(y, [xd, g_, b_], gy.double())
    n = x.shape[0] * x.shape[2]
    k1 = gamma * torch.rsqrt(xd.detach().var((0, 2), unbiased=False) + eps)
    return {'y': y.detach(), 'pre': pre.detach(), 'gx': gx, 'dgamma': dgamma, 'dbeta': dbeta, 'k1': k1, 'k2': k1 * dbeta / n, 'k3': k1 * dgamma / n,
            'g': torch.where(side, gy.double(), gy.double() * slope)}


def bounds(ref, xhat, gamma, beta, mean, invstd, count, r_cap=None):
    """The per-channel bounds of the header, from float64 quantities only.  r_cap: r_c is taken as min(r_c, r_cap) (the GPU tests of the
    node cap it at R_LIMIT: a channel beyond it must not be in the node); 0 for a path that does not recover xhat from y'.
    -> dict: room [c] = r_c + m_c; xhat [b,c,n] (elementwise); dgamma, dbeta [c]; gx [b,c,n]"""
    r = torch.where(gamma == 0, torch.zeros_like(gamma), beta.abs() / gamma.abs().clamp(min=1e-300))
    if r_cap is not None:
        r = r.clamp(max=r_cap)
    room = r + mean.abs() * invstd
    ex = 8 * U * (xhat.abs() + _ch(room))
    ga = ref['g'].abs()
    dgamma = (ga * ex).sum((0, 2))
    dbeta = 8 * U * ga.sum((0, 2))
    k1, k2, k3 = ref['k1'].abs(), ref['k2'].abs(), ref['k3'].abs()
    gx = 8 * U * (_ch(k1) * ga + _ch(k2)) + _ch(k3) * ex + _ch(k1 * (dgamma + dbeta) / count)
    return {'room': room, 'xhat': ex, 'dgamma': dgamma, 'dbeta': dbeta, 'gx': gx}


def ratio(err, bound):
    """largest error / bound per channel: err, bound [c] or [b,c,...] -> [c]"""
    q = err / bound.clamp(min=1e-300)
    return q if q.dim() == 1 else q.transpose(0, 1).flatten(1).amax(1)


def conv_output(seed, b, c, n, device='cpu'):
    """a float32 conv output [b,c,n] with the channel means of MEANS and a deviation near 1, and the gradient dL/dy' (uncorrelated)"""
    gen = torch.Generator(device=device).manual_seed(seed)
    _, _, mean = table(c, device)
    x = (torch.randn(b, c, n, generator=gen, dtype=torch.float64, device=device) * (0.8 + 0.4 * torch.rand(1, c, 1, generator=gen, dtype=torch.float64, device=device))
         + _ch(mean)).float()
    gy = torch.randn(b, c, n, generator=gen, dtype=torch.float64, device=device).float()
    return x, gy


def test_the_guard_flags_a_channel_past_the_limit_only():
    """vgtk.so3conv.functional._norm_ill, the word _ListHead sends to the host: gamma != 0 and |beta| > 128 |gamma|"""
    import vgtk.so3conv.functional as L
    assert L.NORM_IN_NODE_MAX_RATIO == R_LIMIT
    f = lambda pairs: int(L._norm_ill(torch.tensor([p[0] for p in pairs], dtype=torch.float32), torch.tensor([p[1] for p in pairs], dtype=torch.float32)))
    within = [p for p in TABLE if abs(p[1]) <= R_LIMIT * abs(p[0])]
    assert len(within) == len(TABLE) - 3 and (1.0, 128.0) in within
    assert f(within) == 0 and f([(1.0, 0.0)] * 4) == 0                      # the limit itself and the default initialisation: in the node
    assert f(TABLE) == 1
    for beyond in ((1e-3, 0.5), (-1e-3, 0.5), (1e-5, 0.3), (1.0, -128.00002), (-1.0, 128.00002)):
        assert f(within + [beyond]) == 1, beyond
    assert f(within + [(0.0, 0.5)]) == 0                                    # gamma = 0 has its own treatment and does not count
    assert f(within + [(0.0, 0.5), (1e-3, 0.5)]) == 1


@pytest.mark.parametrize('slope', SLOPES)
def test_float32_recovery_per_channel(slope):
    """The float32 emulation of the two kernels against float64 autograd, channel by channel, over TABLE: 7680 elements per channel."""
    b, c, n = 2, len(TABLE), 64 * 60
    x, gy = conv_output(11, b, c, n)
    gamma, beta, _ = table(c)
    gamma, beta = gamma.float().double(), beta.float().double()                  # the parameters are float32 numbers
    fw = emulate_forward(x, gamma, beta, slope)
    bw = emulate_backward(fw, gy, slope)
    ref = float64_reference(x, gamma, beta, gy, slope)
    bd = bounds(ref, fw['xhat'], gamma, beta, fw['mean'], fw['invstd'], fw['count'])
    assert 25 < float(bd['room'][11]) < 40                                       # the channel with |mean| invstd ~ 30
    # the float32 forward takes every element to the side of the kink that float64 does (else g itself differs: not a rounding of the recovery)
    assert torch.equal(bw['pos'], ref['y'] > 0)
    if slope != 1.0:
        assert bool((bw['pos'].any(2).any(0) & (~bw['pos']).any(2).any(0))[:4].all())      # both branches in the channels with small r
    rx = ratio((bw['xhat'].double() - fw['xhat']).abs(), bd['xhat'])
    rg = ratio((bw['sgx'] - ref['dgamma']).abs(), bd['dgamma'])
    rb = ratio((bw['sg'] - ref['dbeta']).abs(), bd['dbeta'])
    rgx = ratio((bw['gx'].double() - ref['gx']).abs(), bd['gx'])
    for i in range(c):
        print(f'slope {slope} channel {i} gamma {float(gamma[i]):g} beta {float(beta[i]):g} r + m {float(bd["room"][i]):.3g}: error / bound  '
              f'xhat {float(rx[i]):.3f}  dgamma {float(rg[i]):.3f}  dbeta {float(rb[i]):.3f}  gx {float(rgx[i]):.3f};  '
              f'dgamma off by {float((bw["sgx"][i] - ref["dgamma"][i]).abs() / ref["dgamma"][i].abs()):.1e} of itself')
    assert float(rx.max()) <= 1.0 and float(rg.max()) <= 1.0 and float(rb.max()) <= 1.0 and float(rgx.max()) <= 1.0, (rx, rg, rb, rgx)
