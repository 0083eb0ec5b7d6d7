"""GPU: the 'narrow input' regime of the inter conv node (vgtk/so3conv/functional.py _forward_narrow / _backward_narrow, csrc/narrow_conv.hip):
a conv with C*K <= 32 contraction indices whose input needs no gradient, followed by a training-mode BatchNorm + leaky_relu, as one
node that keeps the grouped input X and never writes the conv output -- against the same modules with FUSE_CONV_NORM = False (conv,
then the BatchNormLeakyReLU module as passes of their own) and against a float64 evaluation of W X -> BatchNorm -> leaky_relu on the
host.  Bars as in tests/test_gpu_dense.py::test_conv_norm_node_against_separate_modules: y' 1e-5, dW 5e-5, d gamma / d beta 2e-5 (of
the largest magnitude of the reference), running statistics 1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NA, NN = 2, 60, 16
RADIUS, SIGMA = 0.3, 0.03


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a HIP device'
    return torch.device('cuda:0')


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.RandomState(seed).randn(3, 3))
    q *= np.sign(np.linalg.det(q))
    return torch.from_numpy(q.astype(np.float32))


def _inputs(dev, P, O, ck, rotated, seed):
    import synth_clouds
    xyz = torch.from_numpy(synth_clouds.laptop_batch(seed, B, P)[0]).to(dev)
    pose = torch.eye(4, device=dev).repeat(B, P, 1, 1)
    if rotated:                                                  # one rotation per cloud
        for b in range(B):
            pose[b, :, :3, :3] = _rotation(seed + b).to(dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    feats = torch.rand(B, 1, P, NA, device=dev, generator=gen) + 0.5
    W = torch.randn(O, ck, device=dev, generator=gen) * 0.3
    gamma = torch.rand(O, device=dev, generator=gen) + 0.5
    gamma[3] = -0.7                                              # a negative scale
    gamma[5] = 0.0                                               # a constant channel
    beta = torch.randn(O, device=dev, generator=gen) * 0.3
    gy = torch.randn(B, O, P, NA, device=dev, generator=gen)
    return xyz, pose, feats, W, gamma, beta, gy


def _modules(dev, O, kernel_size, slope, W, gamma, beta, radius=RADIUS, sigma=SIGMA, nn=NN):
    import vgtk.so3conv as sptk
    torch.manual_seed(2913)
    conv = sptk.InterSO3PoseConv(1, O, kernel_size, 1, radius, sigma, nn, kanchor=NA, permute_modes=1).to(dev)
    norm = sptk.BatchNormLeakyReLU(O, negative_slope=slope).to(dev)
    with torch.no_grad():
        conv.basic_conv.W.copy_(W); norm.weight.copy_(gamma); norm.bias.copy_(beta)
    return conv, norm


def _step(conv, norm, xyz, pose, feats, gy):
    """one training step -> (y', dW, d gamma, d beta), backward log, forward log, entry names"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    L.BACKWARD_LOG, L.FORWARD_LOG, _hip.KERNEL_TIMES = [], [], []
    try:
        y = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
        grads = torch.autograd.grad(y, [conv.basic_conv.W, norm.weight, norm.bias], gy)
        torch.cuda.synchronize()
        names = [k[0] for k in _hip.KERNEL_TIMES]
    finally:
        blog, flog, L.BACKWARD_LOG, L.FORWARD_LOG, _hip.KERNEL_TIMES = L.BACKWARD_LOG, L.FORWARD_LOG, None, None, None
    return (y.detach(),) + grads, blog, flog, names


def _float64(conv, xyz, pose, feats, W, gamma, beta, gy, slope, eps, momentum):
    """W X -> BatchNorm (batch statistics) -> leaky_relu in float64 on the host, X = the grouped input as the node sees it"""
    import vgtk.so3conv.functional as L
    x = L._inter_group(xyz, pose, feats, NN, conv.anchors, conv.kernels, conv.radius, conv.sigma, True)[2]      # [b,1,k,p,a]
    x = x.reshape(B, -1, x.shape[3] * x.shape[4]).double().cpu()
    W64, g64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (W, gamma, beta))
    y = torch.einsum('ok,bkn->bon', W64, x)
    mean, var = y.mean((0, 2)), y.var((0, 2), unbiased=False)
    out = torch.nn.functional.leaky_relu((y - mean[None, :, None]) * torch.rsqrt(var + eps)[None, :, None] * g64[None, :, None] + b64[None, :, None], slope)
    grads = torch.autograd.grad(out, [W64, g64, b64], gy.double().cpu().reshape(out.shape))
    count = y.shape[0] * y.shape[2]
    rm = momentum * mean.detach()
    rv = (1 - momentum) * 1.0 + momentum * var.detach() * count / (count - 1)
    return (out.detach().view(gy.shape),) + grads + (rm, rv)


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max() / b.detach().double().abs().max())


CASES = [      # P, O, kernel size (1: 24 points, 2: 30), slope, one rotation per cloud
    (64, 64, 1, 0.01, False),
    (52, 64, 1, 0.2, True),           # n = 3120: tails in every pass
    (64, 32, 2, 0.01, True),
    (52, 32, 2, 0.2, False),
    (52, 64, 2, 0.01, False),
]


@pytest.mark.parametrize('P,O,kernel_size,slope,rotated', CASES)
def test_node_against_separate_modules_and_float64(dev, monkeypatch, P, O, kernel_size, slope, rotated):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    ck = {1: 24, 2: 30}[kernel_size]
    xyz, pose, feats, W, gamma, beta, gy = _inputs(dev, P, O, ck, rotated, 7 + P + O)
    out = {}
    for fused in (False, True):
        monkeypatch.setattr(L, 'FUSE_CONV_NORM', fused)
        conv, norm = _modules(dev, O, kernel_size, slope, W, gamma, beta)
        assert conv.basic_conv.W.shape == (O, ck)
        res, blog, flog, names = _step(conv, norm, xyz, pose, feats, gy)
        assert len(blog) == 1 and (blog[0]['regime'] == 'narrow input') == fused and (blog[0].get('norm') == 'in the node') == fused, blog
        assert (flog[0].get('regime') == 'narrow input') == fused, flog
        assert 'eap_inv_lists_rows' not in names                       # neither path builds lists for a layer whose input needs no gradient
        assert ('eap_narrow_conv_bwd_dw_f32' in names) == fused and ('eap_bn_act_bwd_apply_f32' in names) == (not fused), names
        out[fused] = res + (norm.running_mean.clone(), norm.running_var.clone(), int(norm.num_batches_tracked))
        with torch.no_grad():                                          # training mode, gradients off: the same forward, bit for bit
            y_ng = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
        assert torch.equal(y_ng, res[0])
        assert int(norm.num_batches_tracked) == 2
    ref = _float64(conv, xyz, pose, feats, W, gamma, beta, gy, slope, norm.eps, norm.momentum)
    a = out[True]
    for name, b_ in (('separate modules', out[False]), ('float64', ref)):
        errs = [_rel(a[i], b_[i]) for i in range(6)]
        print(f'P={P} O={O} ck={ck} against {name}: y\' {errs[0]:.2e} dW {errs[1]:.2e} dgamma {errs[2]:.2e} dbeta {errs[3]:.2e} '
              f'running mean {errs[4]:.2e} var {errs[5]:.2e}')
        assert errs[0] <= 1e-5 and errs[1] <= 5e-5 and errs[2] <= 2e-5 and errs[3] <= 2e-5 and errs[4] <= 1e-6 and errs[5] <= 1e-6, (name, errs)
    assert a[6] == out[False][6] == 1
    assert float(a[2][5]) == float(a[2][5]) and torch.isfinite(a[1]).all()      # the gamma = 0 channel: finite everywhere


def test_node_per_channel_over_the_conditioning_table(dev, monkeypatch):
    """The first case with the (gamma, beta) table of tests/test_fused_norm_host.py over the channels -- |beta / gamma| up to 3e4 -- channel by
    channel against float64.  This regime recomputes xhat from X and never from y', so it must meet the bounds of that file with r = 0: the
    narrow-input node is free of the effect the dense node is guarded against (tests/test_gpu_conv_norm_conditioning.py), and its layer
    stays in the node whatever beta / gamma is.  What the recomputed conv output adds -- a 24-term float32 dot product, 24u sum |W||X| at
    the most -- is charged to the kink only; the sums' bounds stay 8u."""
    import test_fused_norm_host as H
    import vgtk.so3conv.functional as L
    P, O, kernel_size, slope, rotated = CASES[0]
    xyz, pose, feats, W, _, _, gy = _inputs(dev, P, O, 24, rotated, 7 + P + O)
    pairs = torch.tensor([H.TABLE[i % 11] for i in range(O)], dtype=torch.float32, device=dev)
    gamma, beta = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    monkeypatch.setattr(L, 'FUSE_CONV_NORM', True)
    conv, norm = _modules(dev, O, kernel_size, slope, W, gamma, beta)
    res, blog, flog, _ = _step(conv, norm, xyz, pose, feats, gy)
    assert len(blog) == 1 and blog[0]['regime'] == 'narrow input' and blog[0].get('norm') == 'in the node', blog
    x = L._inter_group(xyz, pose, feats, NN, conv.anchors, conv.kernels, conv.radius, conv.sigma, True)[2]
    x = x.reshape(B, -1, x.shape[3] * x.shape[4]).double().cpu()                                          # [b,ck,n]
    W64, g64, b64 = W.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    y = torch.einsum('ok,bkn->bon', W64, x)
    mean, var = y.mean((0, 2)), y.var((0, 2), unbiased=False)
    invstd = torch.rsqrt(var + norm.eps)
    xhat = (y - mean[None, :, None]) * invstd[None, :, None]
    count = y.shape[0] * y.shape[2]
    yrun = res[0].flatten(2).cpu()
    ref = H.float64_reference(y, g64, b64, gy.flatten(2).cpu(), slope, eps=norm.eps, pos=yrun > 0)
    differ = (yrun > 0) != (ref['pre'] > 0)
    kink = (4 * H.U * (g64.abs()[None, :, None] * (xhat.abs() + (mean.abs() * invstd)[None, :, None]) + b64.abs()[None, :, None])
            + 24 * H.U * (g64.abs() * invstd)[None, :, None] * torch.einsum('ok,bkn->bon', W64.abs(), x.abs()))
    assert bool((ref['pre'].abs()[differ] <= kink[differ]).all()), int(differ.sum())
    bd = H.bounds(ref, xhat, g64, b64, mean, invstd, count, r_cap=0.0)
    ry = H.ratio((yrun.double() - ref['y']).abs(), (1e-5 * ref['y'].abs().amax((0, 2)))[None, :, None].expand_as(ref['y']))
    rg = H.ratio((res[2].double().cpu() - ref['dgamma']).abs(), bd['dgamma'])
    rb = H.ratio((res[3].double().cpu() - ref['dbeta']).abs(), bd['dbeta'])
    dW64 = torch.einsum('bon,bkn->ok', ref['gx'], x)
    dWb = torch.einsum('bon,bkn->ok', bd['gx'], x.abs())
    rW = ((res[1].double().cpu() - dW64).abs() / (5e-5 * float(dW64.abs().max()) + dWb)).amax(1)
    print(f'narrow input over the table ({int(differ.sum())} elements at the kink): largest error / bound per channel  y\' {float(ry.max()):.3f}  '
          f'dgamma {float(rg.max()):.3f}  dbeta {float(rb.max()):.3f}  dW {float(rW.max()):.3f}')
    assert float(ry.max()) <= 1.0 and float(rg.max()) <= 1.0 and float(rb.max()) <= 1.0 and float(rW.max()) <= 1.0


def test_two_identical_steps_are_bit_equal(dev):
    xyz, pose, feats, W, gamma, beta, gy = _inputs(dev, 52, 64, 24, True, 19)
    res = []
    for _ in range(2):
        conv, norm = _modules(dev, 64, 1, 0.01, W, gamma, beta)
        r, blog, _, _ = _step(conv, norm, xyz, pose, feats, gy)
        assert blog[0]['regime'] == 'narrow input'
        res.append(r)
    for a, b_ in zip(*res):
        assert torch.equal(a, b_)


def test_features_that_need_a_gradient_fall_back(dev):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    xyz, pose, feats, W, gamma, beta, gy = _inputs(dev, 64, 64, 24, False, 23)
    conv, norm = _modules(dev, 64, 1, 0.01, W, gamma, beta)
    ref, blog0, _, _ = _step(conv, norm, xyz, pose, feats, gy)
    assert blog0[0]['regime'] == 'narrow input'
    conv, norm = _modules(dev, 64, 1, 0.01, W, gamma, beta)
    f = feats.clone().requires_grad_(True)
    L.BACKWARD_LOG, L.FORWARD_LOG = [], []
    try:
        y = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, f, None, pose))[3].feats
        gF, gW = torch.autograd.grad(y, [f, conv.basic_conv.W], gy)
    finally:
        blog, flog, L.BACKWARD_LOG, L.FORWARD_LOG = L.BACKWARD_LOG, L.FORWARD_LOG, None, None
    assert len(blog) == 1 and blog[0]['regime'] in ('inverse lists', 'textbook dX') and 'norm' not in blog[0], blog
    assert 'regime' not in flog[0]
    assert gF is not None and torch.isfinite(gF).all()
    assert _rel(y, ref[0]) <= 1e-5 and _rel(gW, ref[1]) <= 5e-5


def test_first_layer_of_the_bench_takes_the_regime_without_lists(dev, monkeypatch):
    """the benchmark's first layer (1 -> 64, 64 neighbours, the 4096-point plan's radius, features of ones, identity poses) at P = 64"""
    import synth_clouds
    import vgtk.so3conv.functional as L
    c, o, radius, sigma = synth_clouds.backbone_layers(4096)[0]
    assert (c, o) == (1, 64)
    P = 64
    xyz = torch.from_numpy(synth_clouds.laptop_batch(0, B, P)[0]).to(dev)
    pose = torch.eye(4, device=dev).repeat(B, P, 1, 1)
    feats = torch.ones(B, 1, P, NA, device=dev)
    gen = torch.Generator(device=dev).manual_seed(29)
    gy = torch.randn(B, o, P, NA, device=dev, generator=gen)
    W = torch.randn(o, 24, device=dev, generator=gen) * 0.3
    for fused in (True, False):
        monkeypatch.setattr(L, 'FUSE_CONV_NORM', fused)
        conv, norm = _modules(dev, o, 1, 0.01, W, torch.ones(o, device=dev), torch.zeros(o, device=dev), radius, sigma, 64)
        res, blog, flog, names = _step(conv, norm, xyz, pose, feats, gy)
        assert [r['regime'] for r in blog] == ['narrow input' if fused else 'textbook dX'], blog
        assert 'eap_inv_lists_rows' not in names and 'eap_inv_lists_fill' not in names, names
        if fused:
            assert flog[0]['regime'] == 'narrow input'
            assert [n for n in names if n.startswith('eap_narrow_conv')] == ['eap_narrow_conv_stats_f32', 'eap_narrow_conv_bnact_fwd_f32',
                                                                           'eap_narrow_conv_bwd_reduce_f32', 'eap_narrow_conv_bwd_dw_f32']
            assert not any(n.startswith('eap_bn_') or n.startswith('eap_gemm') for n in names), names
        assert all(torch.isfinite(t).all() for t in res)
