"""GPU: the conv + BatchNorm + leaky_relu node's backward FROM THE OUTPUT, per channel, as |beta / gamma| grows.

The node (vgtk/so3conv/functional.py TrainEpilogue) keeps y' and recovers xhat = ((y' > 0 ? y' : y' / slope) - beta) / gamma in float32, in
bn_act_bwd_reduce_fromy_kernel (csrc/bn_act.hip) and in dense_split_kernel<true> (csrc/so3_dense.hip).  The absolute error of the recovered
xhat grows with r = |beta / gamma| and with m = |mean| invstd of the conv output; the other node tests keep r below 2 and normalise the
parameter gradients by the largest entry over ALL channels, so neither would notice.  Here every channel is held to its own bound.

DERIVED (tests/test_fused_norm_host.py, which also emulates the arithmetic on the CPU):
  * 8u with u = 2^-24: nine roundings between the conv output and the recovered xhat, one of them exact where it matters ->
        |xhat_rec - xhat| <= 8u (|xhat| + r + m),   |d gamma - d gamma_64| <= 8u sum |g| (|xhat| + r + m),   |d beta - d beta_64| <= 8u sum |g|,
        |gx - gx_64| <= 8u (|k1| |g| + |k2| + |k3| (|xhat| + r + m)) + |k1| (the two sums' bounds) / count;
  * R = 128 (vgtk.so3conv.functional.NORM_IN_NODE_MAX_RATIO): the typical loss 2u (max |xhat| + 128) ~ 1.6e-5 reaches the 2e-5 the suite
    grants d gamma / d beta anywhere, so a layer with a channel past it keeps the separate norm module.  The node tests below cap r at R in
    their bounds and demand the log entry without 'norm'.  MEASURED with the guard switched off: the capped worst-case bounds alone would
    let r = 3e4 through (0.05 of the bound -- float32 errors of 61440 terms average out, the bound adds them up), the 2e-5 whole-tensor
    bar kept beside them does not (8e-4);
  * 2^-21 of the row bound: the stored-operand split's own error (tests/test_gpu_dense_passes.py);
  * 0.25 in the decision count: one wrong side of the kink moves a block's sum of g by 1 - slope >= 0.8, the float32 sum of at most 16320
    ones and slopes (64 terms per thread, then a tree over 256 threads) is off by less than 72 u 16320 < 0.1.
No bar here is a measured number.  The largest error / bound ratio of every quantity is printed by each test; the margins found
on an MI355X are on record in profiles/conv_norm_conditioning.txt.  The bars of the whole-layer tests (y' 1e-5, dF 2e-5, dW 5e-5, running
statistics 1e-5 of the largest magnitude) are those of tests/test_gpu_dense.py::test_conv_norm_node_against_separate_modules.

Inputs of the kernel tests are made on the host by the emulation (so they are the same numbers everywhere): a conv output with the channel
means of the table, y' exactly as a forward would have stored it."""
import pytest
import torch

import test_fused_norm_host as H

pytestmark = pytest.mark.gpu

B, C = 2, 16
NN, NA, KS = 64, 60, 24
U, R = H.U, H.R_LIMIT


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _case(dev, seed, b, c, n, slope):
    """-> everything of one (shape, slope) on the device: the emulated forward and backward, the float64 reference and the bounds"""
    x, gy = H.conv_output(seed, b, c, n)
    x, gy = x.to(dev), gy.to(dev)
    gamma, beta, _ = H.table(c, dev)
    gamma, beta = gamma.float().double(), beta.float().double()
    fw = H.emulate_forward(x, gamma, beta, slope)
    bw = H.emulate_backward(fw, gy, slope)
    ref = H.float64_reference(x, gamma, beta, gy, slope)
    bd = H.bounds(ref, fw['xhat'], gamma, beta, fw['mean'], fw['invstd'], fw['count'])
    # (every element on the side of the kink that float64 takes: otherwise g itself differs, which is no rounding of the recovery)
    assert torch.equal(fw['yact'] > 0, ref['y'] > 0)
    return gy, fw, bw, ref, bd


@pytest.mark.parametrize('pts', [1, 272, 300])
@pytest.mark.parametrize('na', [60, 20, 12])
def test_reduction_from_the_output_per_channel(dev, na, pts):
    """eap_bn_act_bwd_reduce_fromy_f32 alone.  At na = 60 a block covers 272 points: pts = 1 is one partly filled block, 272 exactly one
    full block, 300 two blocks with a tail (at na = 20 / 12 a block covers 816 / 1360 points: a partly filled block each time)."""
    from vgtk import _hip
    n = pts * na
    worst = {}
    for slope in H.SLOPES:
        gy, fw, bw, ref, bd = _case(dev, 100 * na + pts, B, C, n, slope)
        shape = (B, C, pts, na)
        gy4, y4 = gy.view(shape).contiguous(), fw['yact'].view(shape).contiguous()
        runs = [_hip.bn_act_bwd_reduce_fromy(gy4, y4, fw['beta'], fw['inv_gamma'], slope, partials=part) for part in (False, True, False, True)]
        for first, again in ((runs[0], runs[2]), (runs[1], runs[3])):
            assert all(torch.equal(p, q) for p, q in zip(first, again))                    # both runs of each call bit-equal
        sg, sgx, gmax, xmax = runs[0]
        pg, pgx = runs[1][0], runs[1][1]
        nblk = int(_hip.abi.eap_bn_act_fromy_blocks(n, na))
        assert pg.shape == (C, B * nblk) and nblk == (2 if (na, pts) == (60, 300) else 1)
        assert torch.equal(pg.sum(1, dtype=torch.float64), sg) and torch.equal(pgx.sum(1, dtype=torch.float64), sgx)
        assert torch.equal(runs[1][2], gmax) and torch.equal(runs[1][3], xmax)
        # the sums, per channel
        rg, rb = H.ratio((sgx - ref['dgamma']).abs(), bd['dgamma']), H.ratio((sg - ref['dbeta']).abs(), bd['dbeta'])
        # the row maxima: |g| exactly, |xhat| within the recovery's bound
        assert torch.equal(gmax, bw['g'].abs().view(shape).amax(2))
        tmax = fw['xhat'].abs().view(shape).amax(2)                                         # [b,c,na] float64
        room = 8 * U * (tmax + bd['room'][None, :, None])
        rx = H.ratio((xmax.double() - tmax).abs(), room)
        # every decision: with dL/dy' = 1 a block's sum of g counts the elements on either side of the kink
        ones = torch.ones_like(gy4)
        cnt = _hip.bn_act_bwd_reduce_fromy(ones, y4, fw['beta'], fw['inv_gamma'], slope, partials=True)[0].view(C, B, nblk)
        per_blk = 16320 // na                                                               # points per block: 16 x 255 float4
        pos = (y4 > 0).double()
        want = torch.zeros(C, B, nblk, dtype=torch.float64, device=dev)
        for k in range(nblk):
            seg = pos[:, :, k * per_blk:(k + 1) * per_blk]
            want[:, :, k] = (seg.sum((2, 3)) + slope * (1 - seg).sum((2, 3))).transpose(0, 1)
        rd = H.ratio((cnt.double() - want).abs().flatten(1).amax(1), torch.full((C,), 0.25, dtype=torch.float64, device=dev))
        for name, r_ in (('dgamma', rg), ('dbeta', rb), ('xmax', rx), ('decisions', rd)):
            worst[name] = max(worst.get(name, 0.0), float(r_.max()))
            assert float(r_.max()) <= 1.0, (name, slope, r_)
    print(f'na={na} pts={pts}: largest error / bound  ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('l', [8, 48])
@pytest.mark.parametrize('na', [60, 20, 12])
def test_split_behind_the_norm_per_channel(dev, na, l):
    """eap_so3_dense_split_bn_f32 alone: the planes' reconstruction of gx = k1 g - k2 - k3 xhat against float64, every element within the
    split's own 2^-21 of the row bound plus the gx bound of its channel.  48 source columns; l = 8 through a column map with absent entries,
    l = 48 without a map (as test_split_behind_a_batchnorm).  The entry takes rows in multiples of 32: the table's channels appear twice,
    on other data."""
    from test_gpu_dense_passes import _planes_to_rows
    from vgtk import _hip
    from vgtk._hip import _ptr, _F32
    m, l_src = 32, 48
    worst = 0.0
    for slope in H.SLOPES:
        gy, fw, bw, ref, bd = _case(dev, 7 + 100 * na + l, B, m, l_src * na, slope)
        shape = (B, m, l_src, na)
        gy4, y4 = gy.view(shape).contiguous(), fw['yact'].view(shape).contiguous()
        coef = torch.stack([bw['k1'], bw['k2'], bw['k3'], fw['beta'], fw['inv_gamma']]).contiguous()
        # the row bound as the node forms it (vgtk/so3conv/functional.py _backward_dense), from the emulation's maxima
        gmax, xmax = bw['g'].abs().view(shape).amax(2), bw['xhat'].abs().view(shape).amax(2)
        bound = (bw['k1'].abs()[None, :, None] * gmax + bw['k2'].abs()[None, :, None] + bw['k3'].abs()[None, :, None] * xmax).contiguous()
        assert bool((bw['gx'].abs().view(shape).amax(2) <= bound * (1 + 8 * U)).all())
        bound = (bound * (1 + 2.0 ** -20)).clamp(min=2.0 ** -100)
        colmap = None
        if l != l_src:
            gen = torch.Generator().manual_seed(na + l)
            colmap = torch.stack([torch.randperm(l_src, generator=gen)[:l] for _ in range(B)]).int()
            colmap[:, 2::5] = -1
            colmap = colmap.to(dev).contiguous()
        gx64, room = ref['gx'].view(shape), bd['gx'].view(shape)
        if colmap is not None:
            take = colmap.clamp(min=0).long()
            live = (colmap >= 0).double()[:, None, :, None]
            gx64 = torch.stack([gx64[i][:, take[i]] for i in range(B)]) * live
            room = torch.stack([room[i][:, take[i]] for i in range(B)]) * live
        lp = (l + 31) // 32 * 32
        outs = []
        for _ in range(2):
            scale = torch.empty(2, B, na, m, device=dev)
            planes = torch.full((B * na * m * lp,), 0x3c003c00, dtype=torch.int32, device=dev)          # (fp16 ones: nothing may stay)
            _hip.call('eap_so3_dense_split_bn_f32', gy4, B, m, l, l_src, na, _ptr(bound.view(torch.int32)), _ptr(colmap), _ptr(gy4), _ptr(y4), _ptr(coef),
                      _F32(slope), _ptr(scale), _ptr(planes))
            outs.append((scale, planes))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])           # both runs bit-equal
        scale, planes = outs[0]
        v, mag = _planes_to_rows(planes, scale, B, m, l, na)                                         # [b,a,row,k]
        rec = (v / scale[0].double()[:, :, :, None])[:, :, :, :l].permute(0, 2, 3, 1)                # [b,row,k,a]
        r_ = H.ratio((rec - gx64).abs(), 2.0 ** -21 * bound.double()[:, :, None, :] + room)
        worst = max(worst, float(r_.max()))
        assert float(r_.max()) <= 1.0, (slope, r_)
        absent = torch.zeros(B, lp, dtype=torch.bool, device=dev)
        absent[:, l:] = True
        if colmap is not None:
            absent[:, :l] = colmap < 0
        assert int(absent.sum()) > 0 or l == lp
        assert float((mag * absent[:, None, None, :]).max()) == 0.0                                  # exact zeros in both planes
    print(f'na={na} l={l}: largest reconstruction error / bound {worst:.3f}')


# ---- the whole node -------------------------------------------------------------------------------------------------------------------

def _within_limit(pair):
    """the table entry, or (1, 128) -- exactly at the limit -- in place of one beyond it"""
    return pair if abs(pair[1]) <= R * abs(pair[0]) else (1.0, 128.0)


def _params(o, dev, which):
    """gamma, beta float32 [o]: 'full' = the table repeated over o (three entries beyond R: the guard acts); 'within' = the same with every
    entry beyond R replaced by (1, 128) (the node is taken); 'one beyond' = 'within' with channel 8 at (1e-3, 0.5); 'zero gamma' = 'within'
    with channel 8 at gamma = 0, beta = 0.5 (r is not defined: the documented gamma = 0 treatment, no switch)"""
    pairs = [H.TABLE[i % 11] for i in range(o)]                   # (the 12th entry of H.TABLE is the mean channel: the same pair as the 2nd)
    if which != 'full':
        pairs = [_within_limit(p) for p in pairs]
    if which == 'one beyond':
        pairs[8] = (1e-3, 0.5)
    if which == 'zero gamma':
        pairs[8] = (0.0, 0.5)
    t = torch.tensor(pairs, dtype=torch.float32, device=dev)
    return t[:, 0].contiguous(), t[:, 1].contiguous()


def _layer(dev, c, o, P=512):
    import synth_clouds
    _, _, radius, sigma = synth_clouds.backbone_layers(4096)[2]
    xyz = torch.from_numpy(synth_clouds.laptop_batch(71, B, P)[0]).to(dev)
    pose = torch.eye(4, device=dev).repeat(B, P, 1, 1)
    gen = torch.Generator(device=dev).manual_seed(41)
    feats0 = torch.randn(B, c, P, NA, device=dev, generator=gen)
    W0 = torch.randn(o, c * KS, device=dev, generator=gen) * 0.05
    gy = torch.randn(B, o, P, NA, device=dev, generator=gen)
    return xyz, pose, feats0, W0, gy, radius, sigma


def _conv(dev, c, o, radius, sigma, W):
    import vgtk.so3conv as sptk
    torch.manual_seed(2913)
    conv = sptk.InterSO3PoseConv(c, o, 1, 1, radius, sigma, NN, kanchor=NA, permute_modes=1).to(dev)
    with torch.no_grad():
        conv.basic_conv.W.copy_(W)
    return conv


def _node_step(dev, monkeypatch, fused, c, o, radius, sigma, xyz, pose, feats0, W, gamma, beta, gy, slope=0.01, seen=None):
    """one training step of conv_norm_act -> (y', dF, dW, d gamma, d beta, running mean, running var, batches tracked), in the node?
    seen: a list that takes what the norm MODULE was given, where it ran as a pass of its own (the conv output of that run)"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    monkeypatch.setattr(L, 'FUSE_CONV_NORM', fused)
    conv = _conv(dev, c, o, radius, sigma, W)
    norm = sptk.BatchNormLeakyReLU(o, negative_slope=slope).to(dev)
    with torch.no_grad():
        norm.weight.copy_(gamma); norm.bias.copy_(beta)
    if seen is not None:
        norm.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    feats = feats0.clone().requires_grad_(True)
    L.BACKWARD_LOG = []
    try:
        y = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
        grads = torch.autograd.grad(y, [feats, conv.basic_conv.W, norm.weight, norm.bias], gy)
    finally:
        log, L.BACKWARD_LOG = L.BACKWARD_LOG, None
    assert len(log) == 1 and log[0]['regime'] == 'dense rows', log
    return (y.detach(),) + grads + (norm.running_mean.clone(), norm.running_var.clone(), int(norm.num_batches_tracked)), log[0].get('norm') == 'in the node'


def _propagated(dev, monkeypatch, c, o, radius, sigma, xyz, pose, feats0, W, gx_room):
    """the gx bound carried through the conv's backward: dF takes it |W|-weighted, dW sum |X|-weighted.  The grouping's interpolation
    weights are not negative, so the conv's own backward (separate modules) on |W|, |F| and the bound as the upstream gradient gives both"""
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    monkeypatch.setattr(L, 'FUSE_CONV_NORM', False)
    conv = _conv(dev, c, o, radius, sigma, W.abs())
    feats = feats0.abs().requires_grad_(True)
    y = conv(zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
    dF, dW = torch.autograd.grad(y, [feats, conv.basic_conv.W], gx_room.float().to(dev).view(y.shape))
    return dF.double() * (1 + 1e-4), dW.double() * (1 + 1e-4)          # (its own float32 rounding: far below 1e-4 of sums of non-negative terms)


@pytest.mark.parametrize('which', ['within', 'full', 'one beyond', 'zero gamma'])
def test_node_per_channel_over_the_table(dev, monkeypatch, which):
    """conv_norm_act at (c, o) = (32, 128), B = 2, P = 512 with the (gamma, beta) table over the channels, fused and with FUSE_CONV_NORM =
    False, against float64 BatchNorm + leaky_relu (and their autograd) of the separate-modules run's conv output.  r is capped at R = 128
    in the fused run's bounds and is 0 in the separate run's.  In 'full' and 'one beyond' the guard must keep the norm out of the node (the
    log says so, and the run then meets the r-free bounds); 'one beyond' against 'within' -- the same channel at (1e-3, 0.5) and at
    (1, 128) -- is the limit from both sides; a gamma = 0 channel alone does not switch regimes."""
    c, o, slope = 32, 128, 0.01
    xyz, pose, feats0, W0, gy, radius, sigma = _layer(dev, c, o)
    gamma, beta = _params(o, dev, which)
    g64, b64 = gamma.double().cpu(), beta.double().cpu()
    out, in_node, seen = {}, {}, []
    for fused in (False, True):
        out[fused], in_node[fused] = _node_step(dev, monkeypatch, fused, c, o, radius, sigma, xyz, pose, feats0, W0, gamma, beta, gy, slope,
                                                seen=seen)
    assert not in_node[False]
    assert in_node[True] == (which in ('within', 'zero gamma')), (which, in_node)
    assert len(seen) == (1 if in_node[True] else 2) and all(torch.equal(t, seen[0]) for t in seen)
    xd = seen[0].flatten(2).double().cpu()                          # the separate-modules run's conv output
    mean, var = xd.mean((0, 2)), xd.var((0, 2), unbiased=False)
    invstd = torch.rsqrt(var + 1e-5)
    xhat = (xd - mean[None, :, None]) * invstd[None, :, None]
    count = xd.shape[0] * xd.shape[2]
    gy64 = gy.flatten(2).cpu()
    live = g64 != 0                                                  # (gamma = 0: d gamma is reported as 0 by the node, documented; not judged here)
    sep = out[False]
    for fused in (False, True):
        res = out[fused]
        # the side of the kink as this run's forward decided it; it may differ from float64's only within the forward's rounding of 0
        yrun = res[0].flatten(2).cpu()
        ref = H.float64_reference(xd, g64, b64, gy64, slope, pos=yrun > 0)
        differ = (yrun > 0) != (ref['pre'] > 0)
        fwd_room = 4 * U * (g64.abs()[None, :, None] * (xhat.abs() + (mean.abs() * invstd)[None, :, None]) + b64.abs()[None, :, None])
        assert bool((ref['pre'].abs()[differ] <= fwd_room[differ]).all()), int(differ.sum())
        # r-free where the norm ran as the separate module (it normalises the stored conv output), capped at R in the node
        bd = H.bounds(ref, xhat, g64, b64, mean, invstd, count, r_cap=R if in_node[fused] else 0.0)
        ry = H.ratio((yrun.double() - ref['y']).abs(), (1e-5 * ref['y'].abs().amax((0, 2)))[None, :, None].expand_as(ref['y']))
        rg = H.ratio((res[3].double().cpu() - ref['dgamma']).abs(), bd['dgamma'])
        rb = H.ratio((res[4].double().cpu() - ref['dbeta']).abs(), bd['dbeta'])
        if in_node[fused] and not bool(live.all()):
            assert bool((res[3].cpu()[~live] == 0).all())
            rg = torch.where(live, rg, torch.zeros_like(rg))
        line = (f'{which} fused={fused} in the node={in_node[fused]} ({int(differ.sum())} elements at the kink): largest error / bound per channel  '
                f'y\' {float(ry.max()):.3f}  dgamma {float(rg.max()):.3f}  dbeta {float(rb.max()):.3f}')
        ok = float(ry.max()) <= 1.0 and float(rg.max()) <= 1.0 and float(rb.max()) <= 1.0
        if fused:
            # dF and dW against the separate run: today's bars plus the gx bound carried through the conv's backward
            dFb, dWb = _propagated(dev, monkeypatch, c, o, radius, sigma, xyz, pose, feats0, W0, bd['gx'])
            rF = float(((res[1].double() - sep[1].double()).abs() / (2e-5 * float(sep[1].abs().max()) + dFb)).max())
            rW = ((res[2].double() - sep[2].double()).abs() / (5e-5 * float(sep[2].abs().max()) + dWb)).amax(1)      # [o]
            line += f'  dF {rF:.3f}  dW (per output channel) {float(rW.max()):.3f}'
            ok = ok and rF <= 1.0 and float(rW.max()) <= 1.0
        print(line)
        assert ok, line
    # y', the running statistics and the batch counter as test_conv_norm_node_against_separate_modules has them
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    a = out[True]
    assert rel(a[0], sep[0]) < 1e-5 and rel(a[5], sep[5]) < 1e-5 and rel(a[6], sep[6]) < 1e-5 and a[7] == sep[7] == 1
    # ... and its whole-tensor bars for the gradients.  The worst-case bounds above are wide enough for r = 3e4 to slip through them capped
    # at R (0.05 of the bound, measured with the guard switched off: profiles/conv_norm_conditioning.txt); this bar is not -- d gamma of the
    # full table in the node is 8e-4 of the largest entry off, 40 times the bar -- so the guard is held by numbers too, not by the log alone
    keep = live.to(dev)                                              # (a gamma = 0 channel's d gamma is reported as 0 by the node)
    whole = (rel(a[1], sep[1]), rel(a[2], sep[2]), rel(a[3][keep], sep[3][keep]), rel(a[4], sep[4]))
    print(f'{which}: against the separate modules, of the largest entry  dF {whole[0]:.2e}  dW {whole[1]:.2e}  dgamma {whole[2]:.2e}  dbeta {whole[3]:.2e}')
    assert whole[0] < 2e-5 and whole[1] < 5e-5 and whole[2] < 2e-5 and whole[3] < 2e-5, whole
    if not in_node[True]:                                            # the guard's run IS the separate-modules run
        assert torch.equal(a[0], sep[0]) and torch.equal(a[5], sep[5]) and torch.equal(a[6], sep[6])
