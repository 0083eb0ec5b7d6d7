"""GPU: the per-slot shape-code head, vgtk.so3conv.InvOutBlockOursWithMask / PointnetSO3ConvOurs (SPConvNets/utils/base_so3conv.py:L1013-1205):
the fused BatchNorm + leaky_relu + point-mean kernels (csrc/heads.hip, eap_bn_act_cloud_mean_*) against float64 with derived bounds, the
module against the fixture the reference class produced (tests/golden/inv_slot_head.npz), and the batched per-cloud / per-slot forms
against the loops they replace."""
import copy

import numpy as np
import pytest
import torch

from inv_slot_common import (BAR_DFEATS, BAR_DPARAM, BAR_OUT, BAR_RUNNING, check_param_grads, inputs_of, make_head, pack_members, rel_err,
                             state_of)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


# ---- kernels against float64 -----------------------------------------------------------------------------------------------------

def _kernel_case(shape, slope, soft, seed):
    """float32 operands on the host and the float64 quantities every bound is evaluated from (the SAME float32 coefficients, widened);
    None when a pre-activation is within rounding of zero (a flipped ReLU must not hide in a tolerance): the caller takes the next seed"""
    b, c, n, na = shape
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    u = lambda *s: torch.rand(*s, generator=gen)
    t = dict(x=r(b, c, n, na) * 1.7 + 0.4, scale=(0.5 + u(b, c)) * torch.where(u(b, c) > 0.25, 1.0, -1.0), shift=r(b, c) * 0.5,
             mean=r(b, c) * 0.3, invstd=0.5 + 1.5 * u(b, c), k2=r(b, c) * 0.1, k3=r(b, c) * 0.1, g=r(b, c, na))
    if soft:
        t['w'] = u(b, n) + 0.05
    else:
        t['w'] = (u(b, n) > 0.4).float()
        t['w'][:, 0] = 1.0
    t['inv_den'] = 1.0 / t['w'].sum(1)
    t['stat_mask'] = (u(b, n) > 0.3).float()
    d = {k: v.double() for k, v in t.items()}
    bc = lambda k: d[k].view(b, c, 1, 1)
    pre = d['x'] * bc('scale') + bc('shift')
    if bool((pre.abs() < 2.0 ** -20 * ((d['x'] * bc('scale')).abs() + bc('shift').abs())).any()):
        return None
    w, den = d['w'].view(b, 1, n, 1), d['inv_den'].view(b, 1, 1, 1)
    slope = float(np.float32(slope))                                          # as the kernel receives it
    act = torch.where(pre > 0, pre, slope * pre)
    gg = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope)) * w * den * d['g'].view(b, c, 1, na)
    xh = (d['x'] - bc('mean')) * bc('invstd')
    ref = dict(fwd=d['inv_den'].view(b, 1, 1) * (w * act).sum(2), fwd_abs=d['inv_den'].view(b, 1, 1) * (w * act).abs().sum(2),
               sg=gg.sum((2, 3)), sg_abs=gg.abs().sum((2, 3)), sgx=(gg * xh).sum((2, 3)), sgx_abs=(gg * xh).abs().sum((2, 3)))
    for tag, m in (('masked', d['stat_mask'].view(b, 1, n, 1)), ('null', 1.0)):
        ref['gx_' + tag] = bc('scale') * gg - m * (bc('k2') + xh * bc('k3'))
        ref['gx_abs_' + tag] = (bc('scale') * gg).abs() + m * (bc('k2').abs() + (xh * bc('k3')).abs())
    return t, ref


@pytest.mark.parametrize('soft', [False, True], ids=['member01', 'soft'])
@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('shape', [(3, 8, 40, 60), (2, 5, 700, 60), (4, 16, 33, 12), (1, 3, 1, 4)])
def test_kernels_against_float64(dev, shape, slope, soft):
    """The three entries against float64 torch on the same float32 coefficients.  L = the longest fp32 accumulation chain of the kernels'
    mapping (csrc/heads.hip): a lane takes every 16th point into 4 alternating accumulators, ceil(n / 64) terms each; the forward then
    folds the 4 (a tree, 2), the 16 (wave, point group) rows through LDS (16) and scales by inv_den (1); the reduction adds the 4 anchors
    of a lane as a tree (2), folds the 4 accumulators (2) and the 16 lanes of a point group (4 shuffles), and its 16 partials are summed
    in float64.  The constant 20 in the bounds pays for the roundings inside one term (the pre-activation, the slope, the weight, xhat).
    Bounds: forward (L + 20) u inv_den sum_p |w act|; reduction (L + 20) u sum |terms|; apply 8 u (|scale gg| + |k2| + |xhat k3|) with
    u = 2^-24 (at most 5 roundings on the first term, 2 and 4 on the others)."""
    from vgtk import _hip
    b, c, n, na = shape
    seed = 100
    while True:
        case = _kernel_case(shape, slope, soft, seed)
        if case is not None:
            break
        seed += 1
    t, ref = case
    t = {k: v.to(dev).contiguous() for k, v in t.items()}
    L_fwd = -(-n // 64) + 2 + 16 + 1
    L_red = -(-n // 64) + 2 + 2 + 4

    def run():
        out = _hip.bn_act_cloud_mean_fwd(t['x'], t['scale'], t['shift'], t['w'], t['inv_den'], slope)
        sg, sgx = _hip.bn_act_cloud_mean_bwd_reduce(t['g'], t['x'], t['scale'], t['shift'], t['mean'], t['invstd'], t['w'], t['inv_den'], slope)
        gxs = [_hip.bn_act_cloud_mean_bwd_apply(t['g'], t['x'], t['scale'], t['shift'], t['mean'], t['invstd'], t['k2'], t['k3'], t['w'],
                                                t['inv_den'], m, slope) for m in (t['stat_mask'], None)]
        return [out, sg, sgx] + gxs

    first, second = run(), run()
    for a_, b_ in zip(first, second):
        assert torch.equal(a_, b_), 'two runs must be bit-identical'
    out, sg, sgx, gx_masked, gx_null = (v.double().cpu() for v in first)
    tiny = 1e-300
    worst = lambda got, want, bound: float(((got - want).abs() / (bound + tiny)).max())
    figures = {'fwd': worst(out, ref['fwd'], (L_fwd + 20) * U * ref['fwd_abs']),
               'reduce g': worst(sg, ref['sg'], (L_red + 20) * U * ref['sg_abs']),
               'reduce g xhat': worst(sgx, ref['sgx'], (L_red + 20) * U * ref['sgx_abs']),
               'apply, stat_mask': worst(gx_masked, ref['gx_masked'], 8 * U * ref['gx_abs_masked']),
               'apply, null': worst(gx_null, ref['gx_null'], 8 * U * ref['gx_abs_null'])}
    print('error / bound:', {k: round(v, 3) for k, v in figures.items()})
    for k, v in figures.items():
        assert v <= 1.0, (k, v)
    if not soft:       # a point of weight 0 adds nothing forward and takes only the statistics' correction backward
        out_pts = (t['w'] == 0).view(b, 1, n, 1).expand(b, c, n, na).cpu()
        zero_stat = out_pts & (t['stat_mask'] == 0).view(b, 1, n, 1).cpu()
        assert float(gx_masked[zero_stat].abs().max() if zero_stat.any() else 0.0) == 0.0


# ---- the fused node against the two existing passes --------------------------------------------------------------------------------

@pytest.mark.parametrize('per_cloud', [True, False], ids=['per_cloud', 'whole_batch'])
@pytest.mark.parametrize('training', [True, False])
def test_fused_node_equals_the_unfused_composition(dev, training, per_cloud):
    """_NormActPointMean against what the package had: per cloud _subset_batchnorm_act + slot_masked_mean (csrc/bn_act.hip eap_bn_act_cloud_*
    and csrc/heads.hip eap_slot_masked_mean_*), whole batch _BNAct + slot_masked_mean: output, every gradient, running statistics."""
    import vgtk.so3conv.heads as H
    from vgtk.so3conv.blocks import _BNAct
    torch.manual_seed(17)
    B, C, P, A = 3, 8, 45, 60
    y0 = torch.randn(B, C, P, A, device=dev) * 1.7 + 0.4
    bias0 = torch.randn(C, device=dev)
    member = torch.rand(B, P, device=dev) > 0.4
    member[:, 0] = True
    member[1] = False; member[1, 7] = True                                    # a 1-point subset
    mask = member.float()
    probe = torch.randn(B, C, A, device=dev)
    res = []
    for fused in (False, True):
        bn = torch.nn.BatchNorm2d(C).to(dev).train(training)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
            bn.running_mean.copy_(torch.linspace(-0.2, 0.6, C)); bn.running_var.copy_(torch.linspace(0.7, 2.0, C))
        y, bias = y0.clone().requires_grad_(True), bias0.clone().requires_grad_(True)
        if fused:
            out = H._norm_act_point_mean(y, bias, mask, 1.0 / mask.sum(1), mask if per_cloud else None, bn, 0.0)
        else:
            if per_cloud:
                z = H._subset_batchnorm_act(y, bias, mask, bn, 0.0)
            else:
                if training:
                    bn.num_batches_tracked.add_(1)
                z = _BNAct.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, bn.momentum, bn.eps, 0.0, False, None, bias)
            out = H.slot_masked_mean(z, mask.view(B, 1, P))[:, 0]
        (out * probe).sum().backward()
        res.append(dict(out=out.detach(), dy=y.grad, dbias=bias.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean.clone(),
                        running_var=bn.running_var.clone(), batches=bn.num_batches_tracked.clone()))
    bars = dict(out=BAR_OUT, dy=BAR_DFEATS, dbias=BAR_DPARAM, dgamma=BAR_DPARAM, dbeta=BAR_DPARAM, running_mean=BAR_RUNNING, running_var=BAR_RUNNING)
    for k, bar in bars.items():
        want, got = res[0][k].cpu().numpy(), res[1][k].cpu().numpy()
        if k == 'dbias' and training:
            assert np.abs(want).max() == 0.0 and np.abs(got).max() == 0.0
            continue
        assert rel_err(got, want) < bar, (k, rel_err(got, want))
    assert int(res[0]['batches']) == int(res[1]['batches']) == ((B if per_cloud else 1) if training else 0)


def test_anchor_counts_the_kernels_do_not_take_run_as_tensor_ops(dev):
    import vgtk.so3conv.heads as H
    torch.manual_seed(2)
    B, C, P = 2, 4, 9
    mask = (torch.rand(B, P, device=dev) > 0.3).float()
    mask[:, 0] = 1.0
    for A in (1, 3):
        y = torch.randn(B, C, P, A, device=dev)
        bn = torch.nn.BatchNorm2d(C).to(dev)
        ref = copy.deepcopy(bn)
        got = H._norm_act_point_mean(y, None, mask, 1.0 / mask.sum(1), None, bn, 0.0)
        want = (torch.relu(ref(y)) * mask.view(B, 1, P, 1)).sum(2) / mask.sum(1).view(B, 1, 1)
        assert rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy()) < BAR_OUT


def test_pointnet_forward_equals_the_concatenated_form(dev):
    """PointnetSO3ConvOurs.forward (contraction of the feature half + rank-3 coordinate term) against the reference's statements
    (base_so3conv.py:L1181-1205) written with torch's convolution on the concatenation"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    torch.manual_seed(4)
    b, c, n, A = 2, 16, 20, 60
    feats, xyz = torch.randn(b, c, n, A, device=dev), torch.randn(b, 3, n, device=dev) * 0.3
    for abs_pos in (False, True):
        for raw in (True, False):
            net = sptk.PointnetSO3ConvOurs(c, 24, A, return_raw=raw, use_abs_pos=abs_pos).to(dev)
            got = net(zptk.SphericalPointCloud(xyz, feats, None))
            centred = xyz if abs_pos else xyz - xyz.mean(2, keepdim=True)
            want = net.embed(torch.cat([feats, torch.einsum('aji,bjn->bina', net.anchors, centred)], 1))
            want = want if raw else want.max(2)[0]
            assert got.shape == want.shape and rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy()) < BAR_OUT


# ---- the module against the reference's fixture --------------------------------------------------------------------------------------

def _functional(res, g):
    return sum((gi * r).sum() for gi, r in zip(g, res))


@pytest.mark.parametrize('batched', [False, True], ids=['per_cloud_loop', 'over_subsets'])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('tag', ['rel', 'abs'])
def test_module_matches_reference_golden(dev, golden, tag, training, batched):
    """InvOutBlockOursWithMask called as the model calls it (once per cloud, batch 1, mask=None, on the gathered subset: 21, 4 and 1
    points), and inv_head_over_subsets on the three clouds at once, against the reference class's outputs, running statistics and
    gradients.  Bars: those of the same comparisons in tests/test_gpu_lists_and_modules.py; tests/test_inv_slot_head_host.py holds the
    collapsed form itself to a quarter of them."""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    G = golden('inv_slot_head.npz')
    mode = 'train' if training else 'eval'
    head = make_head(tag)
    head.load_state_dict(state_of(G, tag))
    head = head.to(dev).train(training)
    xyz, feats, member, g = (v.to(dev) if torch.is_tensor(v) else tuple(e.to(dev) for e in v) for v in inputs_of(G))
    feats.requires_grad_(True)
    if batched:
        res = sptk.inv_head_over_subsets(head, feats, xyz, member)
    else:
        outs = []
        for i in range(member.shape[0]):
            sel = member[i].nonzero().squeeze(1)
            outs.append(head(zptk.SphericalPointCloud(xyz[i:i + 1][:, :, sel].contiguous(), feats[i:i + 1][:, :, sel].contiguous(), None), None))
        res = tuple(torch.cat([o[k] for o in outs], 0) for k in range(3))
    for name, got in zip(('pooled', 'code', 'logits'), res):
        ref = np.asarray(G[f'{tag}_{mode}_{name}'])
        assert got.shape == ref.shape, name
        assert rel_err(got.detach().cpu().numpy(), ref) < BAR_OUT, (name, rel_err(got.detach().cpu().numpy(), ref))
    if training:
        for k, v in head.state_dict().items():
            if 'running' in k:
                assert rel_err(v.cpu().numpy(), np.asarray(G[f'{tag}_after_{k}'])) < BAR_RUNNING, k
            if 'num_batches' in k:
                assert int(v) == 3, k
    names = [n for n, _ in head.named_parameters()]
    grads = torch.autograd.grad(_functional(res, g), [feats] + list(head.parameters()), allow_unused=True)
    assert rel_err(pack_members(grads[0], member).cpu().numpy(), np.asarray(G[f'{tag}_{mode}_grad_feats'])) < BAR_DFEATS
    assert float(grads[0].permute(0, 2, 1, 3)[~member].abs().max()) == 0.0, 'points outside the subset must receive no gradient'
    check_param_grads(dict(zip(names, grads[1:])), G, tag, training, BAR_DPARAM)
    if training:                  # the fused node's own absorbed gradient is exactly zero
        lin_bias = grads[1 + names.index('linear.0.bias')]
        assert lin_bias is None or float(lin_bias.abs().max()) == 0.0


# ---- the batched forms against the loops they replace ---------------------------------------------------------------------------------

def _loop_over_clouds(head, feats, xyz, member):
    import vgtk.spconv as zptk
    outs = []
    for i in range(member.shape[0]):
        sel = member[i].nonzero().squeeze(1)
        outs.append(head(zptk.SphericalPointCloud(xyz[i:i + 1][:, :, sel].contiguous(), feats[i:i + 1][:, :, sel].contiguous(), None), None))
    return tuple(torch.cat([o[k] for o in outs], 0) for k in range(len(outs[0])))


def _compare_heads(ref_head, fast_head, ref_res, fast_res, f_ref, f_fast, probes, training, member=None):
    for k, (want, got) in enumerate(zip(ref_res, fast_res)):
        assert got.shape == want.shape, k
        assert rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy()) < BAR_OUT, (training, k)
    for (k, v), (_, w) in zip(ref_head.state_dict().items(), fast_head.state_dict().items()):
        if 'running' in k:
            assert rel_err(w.cpu().numpy(), v.cpu().numpy()) < BAR_RUNNING, k
        if 'num_batches' in k:
            assert int(v) == int(w), k
    _functional(ref_res, probes).backward()
    _functional(fast_res, probes).backward()
    assert rel_err(f_fast.grad.cpu().numpy(), f_ref.grad.cpu().numpy()) < BAR_DFEATS, training
    if member is not None:
        assert (f_fast.grad.permute(0, 2, 1, 3)[~member] == 0).all(), 'points outside the subset must receive no gradient'
    top = max(float(p_.grad.abs().max()) for p_ in ref_head.parameters() if p_.grad is not None)
    for (k, v), (_, w) in zip(ref_head.named_parameters(), fast_head.named_parameters()):
        got = np.zeros(tuple(v.shape), np.float32) if w.grad is None else w.grad.cpu().numpy()
        want = np.zeros(tuple(v.shape), np.float32) if v.grad is None else v.grad.cpu().numpy()
        if training and k.endswith('.bias') and (k.startswith('linear.') or k == 'pointnet.embed.bias'):
            # in front of a training-mode norm: absorbed by the batch mean, zero or rounding noise on both sides
            assert np.abs(want).max() < 1e-4 * top and np.abs(got).max() < 1e-4 * top, k
            continue
        assert rel_err(got, want) < BAR_DPARAM, (training, k, rel_err(got, want))


@pytest.mark.parametrize('A,abs_pos', [(60, False), (12, False), (60, True), (20, True)], ids=['60-rel', '12-rel', '60-abs', '20-abs'])
def test_inv_head_over_subsets_equals_the_per_cloud_loop(dev, A, abs_pos):
    """vgtk.so3conv.inv_head_over_subsets against the model's loop: the module called once per cloud, batch 1, mask=None, on the gathered
    subset (...pn_38_multi_stage.py:L706-830), with a 4-point and a 1-point subset: outputs, running statistics of both kinds of norm,
    gradients; training and eval mode.  Absolute coordinates need an anchor set to rotate them into (60, or the 20-anchor subset); 12
    anchors, which no anchor set has, run with centred coordinates, whose mean is zero."""
    import vgtk.so3conv as sptk
    torch.manual_seed(3)
    B, C, N = 3, 16, 40
    params = {'dim_in': C, 'mlp': [32, 24], 'fc': [24], 'k': 24, 'kanchor': A, 'temperature': 3.0}
    head = sptk.InvOutBlockOursWithMask(params, norm=1, pooling_method='attention', use_pointnet=True, use_abs_pos=abs_pos,
                                        return_point_pooling_feature=True).to(dev)
    feats = torch.randn(B, C, N, A, device=dev)
    xyz = torch.randn(B, 3, N, device=dev) * 0.3
    member = torch.rand(B, N, device=dev) > 0.5
    member[:, 0] = True
    member[1, 4:] = False; member[1, :4] = True                    # a 4-point subset
    member[2] = False; member[2, 11] = True                        # a 1-point subset
    probes = (torch.randn(B, 24, A, device=dev), torch.randn(B, 24, device=dev), torch.randn(B, A, device=dev))
    for training in (True, False):
        ref_head, fast_head = copy.deepcopy(head).train(training), copy.deepcopy(head).train(training)
        f_ref, f_fast = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
        ref_res = _loop_over_clouds(ref_head, f_ref, xyz, member)
        fast_res = sptk.inv_head_over_subsets(fast_head, f_fast, xyz, member)
        _compare_heads(ref_head, fast_head, ref_res, fast_res, f_ref, f_fast, probes, training, member)


def test_inv_heads_over_slot_groups_equals_the_masked_form(dev):
    """three slots on 64-point clouds: slot 0 small (gathered), slot 1 absent from cloud 1 (falls back to the whole cloud there, so the masked
    form on the full clouds), slot 2 a two-head sequence on one gather"""
    import vgtk.so3conv as sptk
    torch.manual_seed(6)
    B, C, N, A = 2, 16, 64, 60
    params = {'dim_in': C, 'mlp': [24], 'fc': [24], 'k': 24, 'kanchor': A, 'temperature': 3.0}
    mk = lambda abs_pos: sptk.InvOutBlockOursWithMask(params, norm=1, pooling_method='attention', use_pointnet=True, use_abs_pos=abs_pos,
                                                      return_point_pooling_feature=True).to(dev)
    heads = [mk(False), mk(False), [mk(False), mk(True)]]
    labels = torch.full((B, N), 2, device=dev, dtype=torch.long)     # slot 2: points 32 .. 63 of both clouds
    labels[:, :32] = 0
    labels[0, 9:32] = 1                                             # slot 1: 23 points of cloud 0, none of cloud 1
    feats = torch.randn(B, C, N, A, device=dev)
    xyz = torch.randn(B, 3, N, device=dev) * 0.3
    probes = (torch.randn(B, 24, A, device=dev), torch.randn(B, 24, device=dev), torch.randn(B, A, device=dev))
    assert (labels[1] == 1).sum() == 0
    flat = lambda hs: [h for e in hs for h in (e if isinstance(e, list) else [e])]
    ref_heads, fast_heads = copy.deepcopy(heads), copy.deepcopy(heads)
    f_ref, f_fast = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    groups = sptk.slot_point_groups(labels, 3)
    assert groups[0].shape[1] * 10 < N * 9 and groups[1].shape[1] * 10 >= N * 9 and groups[2].shape[1] * 10 < N * 9
    fast = sptk.inv_heads_over_slot_groups(fast_heads, f_fast, xyz, labels, groups=groups)
    assert isinstance(fast[2], list) and len(fast[2]) == 2
    want = []
    for s_, entry in enumerate(ref_heads):
        member = labels == s_
        member = member | (member.sum(1, keepdim=True) == 0)
        for h in (entry if isinstance(entry, list) else [entry]):
            want.append(sptk.inv_head_over_subsets(h, f_ref, xyz, member))
    got = [fast[0], fast[1]] + fast[2]
    ref_loss = sum(_functional(r, probes) for r in want)
    fast_loss = sum(_functional(r, probes) for r in got)
    ref_loss.backward(); fast_loss.backward()
    for i, (w_, g_) in enumerate(zip(want, got)):
        for k in range(3):
            assert rel_err(g_[k].detach().cpu().numpy(), w_[k].detach().cpu().numpy()) < BAR_OUT, (i, k)
    assert rel_err(f_fast.grad.cpu().numpy(), f_ref.grad.cpu().numpy()) < BAR_DFEATS
    for hr, hf in zip(flat(ref_heads), flat(fast_heads)):
        for (k, v), (_, w) in zip(hr.state_dict().items(), hf.state_dict().items()):
            if 'running' in k:
                assert rel_err(w.cpu().numpy(), v.cpu().numpy()) < BAR_RUNNING, k
        top = max(float(p_.grad.abs().max()) for p_ in hr.parameters() if p_.grad is not None)
        for (k, v), (_, w) in zip(hr.named_parameters(), hf.named_parameters()):
            if k.endswith('.bias') and (k.startswith('linear.') or k == 'pointnet.embed.bias'):
                assert float(v.grad.abs().max()) < 1e-4 * top and float(w.grad.abs().max()) < 1e-4 * top, k
                continue
            assert rel_err(w.grad.cpu().numpy(), v.grad.cpu().numpy()) < BAR_DPARAM, k


def test_whole_batch_call_with_masks_follows_the_reference_branches(dev):
    """forward(x, mask, soft_mask) on a whole batch (whole_shp_outblock / glb_outblock): the reference's statements (base_so3conv.py:L1063-1150)
    written with torch modules on the same parameters -- mask in front of and behind the stack, xyz * mask, embed on every point, the plain
    or soft-mask weighted mean, BatchNorm1d + ReLU, attention pooling"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import torch.nn.functional as F
    torch.manual_seed(9)
    B, C, N, A = 2, 16, 21, 60
    params = {'dim_in': C, 'mlp': [24, 16], 'fc': [16], 'k': 16, 'kanchor': A, 'temperature': 3.0}
    feats = torch.randn(B, C, N, A, device=dev)
    xyz = torch.randn(B, 3, N, device=dev) * 0.3
    mask = (torch.rand(B, N, device=dev) > 0.3).float()
    soft = torch.rand(B, N, device=dev)

    def reference(h, x_feats, m, s):
        x_out, x_xyz = x_feats, xyz
        if m is not None:
            x_out = x_out * m.unsqueeze(1).unsqueeze(-1)
            x_xyz = x_xyz * m.unsqueeze(1)
        for lid, linear in enumerate(h.linear):
            x_out = F.relu(h.norm[lid](linear(x_out)))
        if m is not None:
            x_out = x_out * m.unsqueeze(1).unsqueeze(-1)
        if not h.use_pointnet:
            x_out = x_out.sum(2) / s.unsqueeze(1).unsqueeze(-1).sum(2).clamp(min=1e-8) if s is not None else x_out.mean(2)
        else:
            out_feat = x_out
            centred = x_xyz if h.use_abs_pos else x_xyz - x_xyz.mean(2, keepdim=True)
            x_out = h.pointnet.embed(torch.cat([x_out, torch.einsum('aji,bjn->bina', h.pointnet.anchors, centred)], 1))
            if s is not None:
                x_out = (x_out * s.unsqueeze(1).unsqueeze(-1)).sum(2) / s.unsqueeze(1).unsqueeze(-1).sum(2).clamp(min=1e-8)
            else:
                x_out = x_out.mean(2)
            x_out = F.relu(h.norm[len(h.linear)](x_out))
        pooled = x_out.clone()
        if h.pooling_method == 'mean':
            return pooled, x_out.mean(2), out_feat.squeeze(1)
        if h.pooling_method == 'max':
            return pooled, x_out.max(2)[0], out_feat.squeeze(1)
        out_feat = h.attention_layer(x_out)
        return pooled, (x_out * F.softmax(out_feat * h.temperature, dim=2)).sum(-1), out_feat.squeeze(1)

    # (behind the pointnet stage a pooling other than 'attention' returns the per-point map in the last place, as the reference does)
    for use_pointnet, abs_pos, m, s, pooling in ((True, False, mask, None, 'attention'), (True, True, mask, soft, 'attention'),
                                                 (True, False, None, soft, 'attention'), (False, False, mask, soft, 'attention'),
                                                 (False, False, None, None, 'attention'), (True, False, mask, None, 'max'),
                                                 (True, True, None, soft, 'mean')):
        head = sptk.InvOutBlockOursWithMask(params, norm=1, pooling_method=pooling, use_pointnet=use_pointnet, use_abs_pos=abs_pos,
                                            return_point_pooling_feature=True).to(dev)
        gen = torch.Generator(device=dev).manual_seed(12)
        for training in (True, False):
            ref_head, fast_head = copy.deepcopy(head).train(training), copy.deepcopy(head).train(training)
            f_ref, f_fast = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
            ref_res = reference(ref_head, f_ref, m, s)
            fast_res = fast_head(zptk.SphericalPointCloud(xyz, f_fast, None), m, soft_mask=s)
            probes = tuple(torch.randn(r.shape, generator=gen, device=dev) for r in ref_res)
            _compare_heads(ref_head, fast_head, ref_res, fast_res, f_ref, f_fast, probes, training)
