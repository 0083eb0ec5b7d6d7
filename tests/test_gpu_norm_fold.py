"""GPU: the entries of csrc/norm_fold.hip against the tensor expressions they replace (vgtk/so3conv/blocks.py batch_moments,
update_running_stats, affine_from_moments; the glue of _backward_dense / _backward_narrow; _hip.so3_dense_gplanes; _hip.DenseGeometry), on
the same partial sums.  Only the order of the float64 sum over the partials differs, so the bars are those of the number formats:
  * float32 outputs that are a product or a quotient (scale, k2, k3, inv_gamma, d gamma, d beta, running variance): 1 float32 ulp, 2^-23 |ref|;
  * float32 outputs formed by a difference (shift = beta - mean scale, running mean): 2^-22 x (the sum of the magnitudes of their terms);
  * mean (float64): parts x 2^-52 x (|pivot| + sum |ps| / count);
    invstd (float64): parts x 2^-52 x (invstd + invstd^3 / 2 x T), T = sum |pq| / count + 2 |m| sum |ps| / count + m^2 the magnitudes of the
    terms of var = s2 / count - m^2 (d invstd = - invstd^3 / 2 d var), the first summand for the rounding of rsqrt itself;
  * the bounds (bound, colmax, words, the operand's bound) feed a power-of-two scale: within 4 x 2^-23 of the expression's value and never
    more than 2^-22 below it;
  * integer outputs and copies: bit-exact.
Then one dense and one narrow-input conv + norm step with the switch on and off at the layer bars of tests/test_gpu_dense.py and
tests/test_gpu_narrow_input_node.py, and the launch sequence of the dense node."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
B, NA = 2, 60


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'the gpu-marked tests need a HIP device'
    return torch.device('cuda:0')


def _within(name, got, ref, rel, terms=None):
    """|got - ref| <= rel x (terms or |ref|), element by element, in float64"""
    got, ref = got.double(), ref.double()
    room = rel * (ref.abs() if terms is None else terms.double())
    bad = (got - ref).abs() > room
    assert not bool(bad.any()), (name, float(((got - ref).abs() / room.clamp_min(1e-300)).max()))


def _upper_bound(name, got, ref):
    _within(name, got, ref, 4 * ULP)
    assert bool((got.double() >= ref.double() * (1 - 2.0 ** -22)).all()), name


@pytest.mark.parametrize('o', [32, 96])
@pytest.mark.parametrize('parts', [1, 7, 480])
@pytest.mark.parametrize('running,stride', [(True, 1), (False, 5), (True, 3)])
def test_train_fold_against_the_block_helpers(dev, o, parts, running, stride):
    from vgtk import _hip
    from vgtk.so3conv.blocks import affine_from_moments, batch_moments, update_running_stats
    gen = torch.Generator(device=dev).manual_seed(100 * o + parts + stride)
    count = 50 * parts + 3
    ps = torch.randn(o, parts, device=dev, generator=gen) * 5
    pq = (torch.rand(o, parts, device=dev, generator=gen) + 0.5) * 60
    ps[4], pq[4] = 0.0, 0.0                                         # a constant channel: var = 0
    ps[6], pq[6] = 3.0, 1e-3                                        # ... and one whose raw variance is negative: clamped to 0
    store = torch.randn(o, stride, device=dev, generator=gen) * 2
    pivot = store[:, 0]
    assert pivot.stride(0) == stride
    gamma = torch.rand(o, device=dev, generator=gen) + 0.5
    gamma[3], gamma[5] = -0.7, 0.0
    beta = torch.randn(o, device=dev, generator=gen) * 0.3
    eps, momentum = 1e-5, 0.1
    rm0 = torch.randn(o, device=dev, generator=gen)
    rv0 = torch.rand(o, device=dev, generator=gen) + 0.5
    # the tensor expressions (TrainEpilogue.moments)
    s1, s2 = ps.sum(1, dtype=torch.float64), pq.sum(1, dtype=torch.float64)
    mean, var, total = batch_moments(s1, s2, pivot.double(), count)
    rm_ref, rv_ref = rm0.clone(), rv0.clone()
    update_running_stats(rm_ref, rv_ref, mean, var, total, momentum)
    g64 = gamma.double()
    scale, shift, invstd = affine_from_moments(mean, var, g64, beta, eps)
    inv_gamma = torch.where(g64 == 0, torch.zeros_like(g64), 1.0 / g64).float()
    assert float(var[4]) == 0.0 and float(var[6]) == 0.0
    out = []
    for _ in range(2):
        rm, rv = (rm0.clone(), rv0.clone()) if running else (None, None)
        out.append(_hip.norm_fold_train(ps, pq, pivot, count, gamma, beta, eps, momentum, rm, rv) + ((rm, rv) if running else ()))
    for a, b_ in zip(*out):
        assert torch.equal(a, b_)                                   # the same bits on every run
    scale_n, shift_n, mean_n, invstd_n, beta_n, inv_gamma_n = out[0][:6]
    assert mean_n.dtype == invstd_n.dtype == torch.float64 and scale_n.dtype == torch.float32
    _within('scale', scale_n, scale, ULP)
    _within('inv_gamma', inv_gamma_n, inv_gamma, ULP)
    assert float(inv_gamma_n[5]) == 0.0 and float(scale_n[5]) == 0.0 and torch.equal(beta_n, beta)
    _within('shift', shift_n, shift, 2 * ULP, beta.double().abs() + (mean * g64 * invstd).abs())
    m = s1 / count
    abs1, abs2 = ps.double().abs().sum(1) / count, pq.double().abs().sum(1) / count
    _within('mean', mean_n, mean, parts * 2.0 ** -52, pivot.double().abs() + abs1)
    _within('invstd', invstd_n, invstd, parts * 2.0 ** -52, invstd + 0.5 * invstd ** 3 * (abs2 + 2 * m.abs() * abs1 + m * m))
    if running:
        _within('running_var', out[0][7], rv_ref, ULP)
        _within('running_mean', out[0][6], rm_ref, 2 * ULP, (1 - momentum) * rm0.double().abs() + momentum * mean.abs())


@pytest.mark.parametrize('o', [32, 96])
@pytest.mark.parametrize('parts', [1, 7, 480])
def test_backward_fold_against_the_node_expressions(dev, o, parts):
    from vgtk import _hip
    gen = torch.Generator(device=dev).manual_seed(7 * o + parts)
    count = 50 * parts + 3
    pg = torch.randn(o, parts, device=dev, generator=gen) + 0.3
    pgx = torch.randn(o, parts, device=dev, generator=gen) * 2 - 0.4
    k1 = torch.randn(o, device=dev, generator=gen)
    k1[5] = 0.0
    beta = torch.randn(o, device=dev, generator=gen)
    inv_gamma = torch.randn(o, device=dev, generator=gen)
    gmax = torch.rand(B, o, NA, device=dev, generator=gen) * 3
    xmax = torch.rand(B, o, NA, device=dev, generator=gen) * 4
    # _backward_dense
    tg, tgx = pg.sum(1, dtype=torch.float64), pgx.sum(1, dtype=torch.float64)
    k2 = (k1.double() * tg / count).float()
    k3 = (k1.double() * tgx / count).float()
    bound = (k1.abs()[None, :, None] * gmax + k2.abs()[None, :, None] + k3.abs()[None, :, None] * xmax).contiguous()
    dense = [_hip.norm_fold_bwd(pg, pgx, k1, count, beta, inv_gamma, gmax, xmax) for _ in range(2)]
    narrow = [_hip.norm_fold_bwd(pg, pgx, k1, count) for _ in range(2)]
    for pair in (dense, narrow):
        for a, b_ in zip(*pair):
            assert torch.equal(a, b_)
    for a, b_ in zip(dense[0][:4], narrow[0]):                      # the narrow node's four are the dense node's first four
        assert torch.equal(a, b_)
    dgamma_n, dbeta_n, k2_n, k3_n, coef_n, bound_n, colmax_n = dense[0]
    _within('dgamma', dgamma_n, tgx.float(), ULP)
    _within('dbeta', dbeta_n, tg.float(), ULP)
    _within('k2', k2_n, k2, ULP)
    _within('k3', k3_n, k3, ULP)
    assert coef_n.shape == (5, o) and torch.equal(coef_n[0], k1) and torch.equal(coef_n[1], k2_n) and torch.equal(coef_n[2], k3_n)
    assert torch.equal(coef_n[3], beta) and torch.equal(coef_n[4], inv_gamma)
    _upper_bound('bound', bound_n, bound)
    _upper_bound('colmax', colmax_n, bound.amax(1))
    assert torch.equal(colmax_n, bound_n.amax(1))                   # ... and exactly the maximum of the bound it goes with


@pytest.mark.parametrize('rp', [16, 48])
def test_zbound_against_the_node_expression(dev, rp):
    from vgtk import _hip
    gen = torch.Generator(device=dev).manual_seed(rp)
    p, ra = 37, NA * rp
    ldz = _hip.dense_pitch(ra)
    assert ldz > ra and ldz % 4 == 0
    colmax = torch.rand(B, NA, device=dev, generator=gen) * 5
    cnt = torch.randint(0, p + 1, (B, rp + 11), device=dev, generator=gen, dtype=torch.int32)       # (rows rp + 11 apart: a row stride of its own)
    cnt[0, 1], cnt[1, 2], cnt[0, 6], cnt[1, 0] = -2, -1, p + 9, 2 * p                                  # negative entries, entries above p
    assert int(cnt[:, :rp].min()) < 0 and int(cnt[:, :rp].max()) > p
    n_rows = torch.tensor([rp - 3, rp // 2], dtype=torch.int32, device=dev)
    # _backward_dense
    live = torch.arange(rp, device=dev)[None, :] < n_rows[:, None]
    cntf = torch.where(live, cnt[:, :rp], torch.zeros_like(cnt[:, :rp])).clamp(min=0, max=p).to(torch.float32)
    cols = colmax[:, :, None] * cntf[:, None, :]
    ref = torch.zeros(B, ldz // 4, dtype=torch.float32, device=dev)
    ref[:, :ra // 4] = cols.view(B, NA, rp // 4, 4).amax(3).view(B, ra // 4)
    words = [_hip.so3_dense_zbound(colmax, cnt, n_rows, rp, p, ldz) for _ in range(2)]
    assert torch.equal(words[0], words[1]) and words[0].shape == (B, ldz // 4)
    _upper_bound('words', words[0], ref)
    assert float(words[0][:, ra // 4:].abs().max()) == 0.0 and float(ref.max()) > 0.0


@pytest.mark.parametrize('o,c,rp', [(32, 64, 16), (96, 128, 48)])
def test_operand_bound_against_the_expression(dev, o, c, rp):
    from vgtk import _hip
    ks = 24
    gen = torch.Generator(device=dev).manual_seed(o + rp)
    W3 = torch.randn(o * ks, c, device=dev, generator=gen) * torch.exp(torch.randn(o * ks, 1, device=dev, generator=gen))
    fc4 = torch.randn(B, c, rp, NA, device=dev, generator=gen) * torch.exp(2 * torch.randn(B, 1, 1, NA, device=dev, generator=gen))
    # _hip.so3_dense_gplanes
    wsum = W3.abs().sum(1).view(o, ks).amax(1)
    fm = fc4.abs().amax((1, 2))
    ref = (fm[:, :, None] * (wsum * 1.0001)[None, None, :]).contiguous()
    got = [_hip.so3_dense_gplanes_bound(W3, fc4, ks) for _ in range(2)]
    assert torch.equal(got[0], got[1]) and got[0].shape == (B, NA, o)
    _upper_bound('operand bound', got[0], ref)
    # (the bound it is: no |G| of the operand above it, float64)
    G = torch.einsum('okc,bcra->bokra', W3.view(o, ks, c).double(), fc4.double()).abs().amax((2, 3))      # [b,o,a]
    assert bool((got[0].double() >= G.transpose(1, 2)).all())


@pytest.mark.parametrize('words', [16, 32])
@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_point_order_is_bit_exact(dev, words, where):
    from vgtk import _hip
    p = 101                                                         # not a multiple of 32
    gen = torch.Generator(device=dev).manual_seed(words + len(where))
    order = torch.stack([torch.randperm(p, device=dev, generator=gen) for _ in range(B)])
    j = {'first': 0, 'middle': 57, 'last': p - 1}[where]
    at = int((order[0] == 0).nonzero()[0, 0])
    order[0, at], order[0, j] = order[0, j].clone(), 0              # cloud 0's point 0 in column j
    assert order.dtype == torch.int64 and sorted(order[0].tolist()) == list(range(p))
    memb = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, p, words), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    q_xyz = torch.randn(B, 3, p, device=dev, generator=gen)
    # _hip.DenseGeometry
    xyz_ref = q_xyz.gather(2, order[:, None, :].expand(B, 3, p)).contiguous()
    memb_ref = memb.gather(1, order[:, :, None].expand(B, p, words)).contiguous()
    pivot_ref = (order[0] == 0).to(torch.int32).argmax().to(torch.int32).view(1)
    got = [_hip.so3_dense_point_order(order, memb, q_xyz) for _ in range(2)]
    for a, b_ in zip(*got):
        assert torch.equal(a, b_)
    order32, memb_n, xyz_n, pivot_n = got[0]
    assert order32.dtype == torch.int32 and torch.equal(order32, order.to(torch.int32))
    assert torch.equal(memb_n, memb_ref) and torch.equal(xyz_n, xyz_ref)
    assert pivot_n.dtype == torch.int32 and torch.equal(pivot_n, pivot_ref) and int(pivot_n) == j


def _rel(a, b_):
    return float((a.detach().double() - b_.detach().double()).abs().max() / b_.detach().double().abs().max())


def test_dense_node_with_the_switch_on_and_off(dev, monkeypatch):
    """tests/test_gpu_dense.py::test_conv_norm_node_against_separate_modules at its smallest shape, node against node"""
    import synth_clouds
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    P, c, o, KS, NN = 512, 64, 128, 24, 64                       # (c = 64: the smallest width whose forward operand is made by one kernel)
    _, _, radius, sigma = synth_clouds.backbone_layers(4096)[2]
    xyz = torch.from_numpy(synth_clouds.laptop_batch(71, B, P)[0]).to(dev)
    pose = torch.eye(4, device=dev).repeat(B, P, 1, 1)
    gen = torch.Generator(device=dev).manual_seed(41)
    feats0 = torch.randn(B, c, P, NA, device=dev, generator=gen)
    W0 = torch.randn(o, c * KS, device=dev, generator=gen) * 0.05
    gamma0 = torch.rand(o, device=dev, generator=gen) + 0.5
    gamma0[3], gamma0[5] = -0.7, 0.0
    beta0 = torch.randn(o, device=dev, generator=gen) * 0.3
    gy = torch.randn(B, o, P, NA, device=dev, generator=gen)
    out, names = {}, {}
    for native in (False, True):
        monkeypatch.setattr(_hip, 'NATIVE_NORM_GLUE', native)
        torch.manual_seed(2913)
        conv = sptk.InterSO3PoseConv(c, o, 1, 1, radius, sigma, NN, kanchor=NA, permute_modes=1).to(dev)
        norm = sptk.BatchNormLeakyReLU(o, negative_slope=0.01).to(dev)
        with torch.no_grad():
            conv.basic_conv.W.copy_(W0); norm.weight.copy_(gamma0); norm.bias.copy_(beta0)
        feats = feats0.clone().requires_grad_(True)
        L.BACKWARD_LOG, _hip.KERNEL_TIMES = [], []
        try:
            y = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
            grads = torch.autograd.grad(y, [feats, conv.basic_conv.W, norm.weight, norm.bias], gy)
            torch.cuda.synchronize()
            names[native] = [k[0] for k in _hip.KERNEL_TIMES]
        finally:
            log, L.BACKWARD_LOG, _hip.KERNEL_TIMES = L.BACKWARD_LOG, None, None
        assert log[0]['regime'] == 'dense rows' and log[0].get('norm') == 'in the node', log
        out[native] = (y.detach(),) + grads + (norm.running_mean.clone(), norm.running_var.clone())
    a, b_ = out[True], out[False]
    errs = [_rel(a[i], b_[i]) for i in range(7)]
    print('dense node, switch on against off: y\' %.2e dF %.2e dW %.2e dgamma %.2e dbeta %.2e running mean %.2e var %.2e' % tuple(errs))
    assert errs[0] < 1e-5 and errs[1] < 2e-5 and errs[2] < 5e-5 and errs[3] < 2e-5 and errs[4] < 2e-5 and errs[5] < 1e-5 and errs[6] < 1e-5, errs
    assert all(torch.isfinite(t).all() for t in a)
    # the launch sequence of the node: every new entry, in the order of the sites, between the kernels they serve
    new = ['eap_so3_dense_point_order', 'eap_so3_dense_gplanes_bound_f32', 'eap_norm_fold_train_f32', 'eap_norm_fold_bwd_f32', 'eap_so3_dense_zbound_f32']
    seq = names[True]
    assert [n for n in seq if n in new] == new, seq
    assert seq.index('eap_so3_dense_gplanes_bound_f32') < seq.index('eap_so3_dense_gplanes_f32')
    assert seq.index('eap_bn_stats_f32') < seq.index('eap_norm_fold_train_f32') < seq.index('eap_so3_dense_untranspose_bnact_f32')
    assert seq.index('eap_bn_act_bwd_reduce_fromy_f32') < seq.index('eap_norm_fold_bwd_f32') < seq.index('eap_so3_dense_split_bn_f32')
    assert not any(n in new for n in names[False]) and [n for n in seq if n not in new] == names[False]


def test_narrow_node_with_the_switch_on_and_off(dev, monkeypatch):
    """tests/test_gpu_narrow_input_node.py at its first case (P = 64, O = 64, 24 contraction indices), node against node"""
    import synth_clouds
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    from vgtk import _hip
    P, O, NN = 64, 64, 16
    xyz = torch.from_numpy(synth_clouds.laptop_batch(135, B, P)[0]).to(dev)
    pose = torch.eye(4, device=dev).repeat(B, P, 1, 1)
    gen = torch.Generator(device=dev).manual_seed(135)
    feats = torch.rand(B, 1, P, NA, device=dev, generator=gen) + 0.5
    W = torch.randn(O, 24, device=dev, generator=gen) * 0.3
    gamma = torch.rand(O, device=dev, generator=gen) + 0.5
    gamma[3], gamma[5] = -0.7, 0.0
    beta = torch.randn(O, device=dev, generator=gen) * 0.3
    gy = torch.randn(B, O, P, NA, device=dev, generator=gen)
    out, names = {}, {}
    for native in (False, True):
        monkeypatch.setattr(_hip, 'NATIVE_NORM_GLUE', native)
        torch.manual_seed(2913)
        conv = sptk.InterSO3PoseConv(1, O, 1, 1, 0.3, 0.03, NN, kanchor=NA, permute_modes=1).to(dev)
        norm = sptk.BatchNormLeakyReLU(O, negative_slope=0.01).to(dev)
        with torch.no_grad():
            conv.basic_conv.W.copy_(W); norm.weight.copy_(gamma); norm.bias.copy_(beta)
        _hip.KERNEL_TIMES = []
        try:
            y = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
            grads = torch.autograd.grad(y, [conv.basic_conv.W, norm.weight, norm.bias], gy)
            torch.cuda.synchronize()
            names[native] = [k[0] for k in _hip.KERNEL_TIMES]
        finally:
            _hip.KERNEL_TIMES = None
        out[native] = (y.detach(),) + grads + (norm.running_mean.clone(), norm.running_var.clone())
    a, b_ = out[True], out[False]
    errs = [_rel(a[i], b_[i]) for i in range(6)]
    print('narrow node, switch on against off: y\' %.2e dW %.2e dgamma %.2e dbeta %.2e running mean %.2e var %.2e' % tuple(errs))
    assert errs[0] <= 1e-5 and errs[1] <= 5e-5 and errs[2] <= 2e-5 and errs[3] <= 2e-5 and errs[4] <= 1e-6 and errs[5] <= 1e-6, errs
    assert [n for n in names[True] if n.startswith(('eap_narrow_conv', 'eap_norm_fold'))] == [
        'eap_narrow_conv_stats_f32', 'eap_norm_fold_train_f32', 'eap_narrow_conv_bnact_fwd_f32', 'eap_narrow_conv_bwd_reduce_f32',
        'eap_norm_fold_bwd_f32', 'eap_narrow_conv_bwd_dw_f32']
    assert not any(n.startswith('eap_norm_fold') for n in names[False])
