"""GPU: the per-cloud BatchNorm and the fused BatchNorm + leaky_relu + point mean on the 240-anchor map of a `use_2d` backbone:
the eap_bn_act_cloud_mean_wide_* entries (csrc/heads.hip at Q = 64) against float64 under bounds counted from their mapping
(tests/inv_slot_wide_common.py) and against their narrow twins at 60 anchors; vgtk.so3conv.heads._NormActPointMean and _subset_batchnorm_act
at 240 anchors against the unfused composition and float64; InvOutBlockOursWithMask against the fixture the reference class produced on a
240-anchor map (tests/golden/inv_slot_head_2d.npz); pose_head_over_subsets and the per-slot forms against the loops they replace; and the
names handed to the library while all of that runs (SPConvNets/utils/base_so3conv.py:L1013-1205, SPConvNets/models/model_utils.py:L470-484)."""
import copy

import numpy as np
import pytest
import torch

import inv_slot_wide_common as W
from inv_slot_common import (BAR_DFEATS, BAR_DPARAM, BAR_OUT, BAR_RUNNING, check_param_grads, inputs_of, pack_members, rel_err, state_of)
from test_gpu_head_pooling import Carved, _twice, dev  # noqa: F401  (the guard-banded buffers and the two-run check of the pooling kernels' test)

pytestmark = pytest.mark.gpu

U = W.U
MEAN_WIDE = {'eap_bn_act_cloud_mean_wide_fwd_f32', 'eap_bn_act_cloud_mean_wide_bwd_reduce_f32', 'eap_bn_act_cloud_mean_wide_bwd_apply_f32'}
MEAN_NARROW = {n.replace('_wide', '') for n in MEAN_WIDE}
FLAT_CLOUD = {'eap_bn_stats_masked_f32', 'eap_bn_act_cloud_fwd_f32', 'eap_bn_act_cloud_bwd_reduce_f32', 'eap_bn_act_cloud_bwd_apply_f32'}


@pytest.fixture
def calls(monkeypatch):
    """the names vgtk hands to _hip.call while a test runs; the torch expressions that stand behind the kernels for other anchor counts are
    replaced by refusals (calls.torch keeps the real ones for a test that needs a comparator)"""
    import vgtk.so3conv.heads as H
    from vgtk import _hip
    class Seen(list):
        pass
    real, seen = _hip.call, Seen()
    seen.torch = {}

    def recording(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(_hip, 'call', recording)
    for name in ('_subset_batchnorm_act_torch', '_norm_act_point_mean_torch', '_slot_masked_mean_torch', '_masked_max_torch'):
        seen.torch[name] = getattr(H, name)

        def refuse(*a, _name=name, **k):
            raise AssertionError(f'{_name}: the torch expression ran where a kernel is expected')
        monkeypatch.setattr(H, name, refuse)
    return seen


def _run_entries(dev, d, b, c, n, na, slope, suffix):
    """the three entries (suffix '_wide' or '') into guard-banded buffers -> {output: Carved}"""
    from vgtk import _hip
    parts = int(getattr(_hip.abi, f'eap_bn_act_cloud_mean{suffix}_parts')(n))
    o = dict(fwd=Carved((b, c, na), torch.float32, dev), pg=Carved((b, c, parts), torch.float32, dev), pgx=Carved((b, c, parts), torch.float32, dev),
             gx_masked=Carved((b, c, n, na), torch.float32, dev), gx_null=Carved((b, c, n, na), torch.float32, dev))
    pre = f'eap_bn_act_cloud_mean{suffix}_'
    _hip.call(pre + 'fwd_f32', d['x'], b, c, n, na, slope, d['x'], d['scale'], d['shift'], d['w'], d['inv_den'], o['fwd'].t)
    _hip.call(pre + 'bwd_reduce_f32', d['x'], b, c, n, na, slope, d['g'], d['x'], d['scale'], d['shift'], d['mean'], d['invstd'], d['w'], d['inv_den'],
              o['pg'].t, o['pgx'].t)
    for key, m in (('gx_masked', d['stat_mask']), ('gx_null', None)):
        _hip.call(pre + 'bwd_apply_f32', d['x'], b, c, n, na, slope, d['g'], d['x'], d['scale'], d['shift'], d['mean'], d['invstd'], d['k2'], d['k3'],
                  d['w'], d['inv_den'], m, o[key].t)
    return o


def _named(got):
    """the entries' raw outputs -> the names of inv_slot_wide_common.bounds (the partials added in float64, as the caller adds them)"""
    return {'fwd': got['fwd'], 'reduce g': got['pg'].astype(np.float64).sum(2), 'reduce g xhat': got['pgx'].astype(np.float64).sum(2),
            'apply, stat_mask': got['gx_masked'], 'apply, null': got['gx_null']}


# ---- (a) the entries against float64 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('na,shape', W.GRID)
def test_wide_entries_against_float64(dev, na, shape):
    """The three entries against float64 on the float32 coefficients of tests/test_gpu_inv_slot_head.py's _kernel_case, slope 0 and 0.2, hard
    and soft weights, stat_mask given and null, under the bounds of tests/inv_slot_wide_common.py, whose chain lengths are counted from the
    kernels' mapping: an accumulator receives every 16th point (4 waves x 4 rows in flight), so
        L_fwd = ceil(n / 16) + 2 (accumulator tree) + 4 (wave fold) + 1 (inv_den),
        L_red = ceil(n / 16) + 2 (a lane's four anchors) + 2 (accumulator tree) + 6 (shuffle steps),
    forward (L_fwd + 20) u inv_den sum |w act|, reduce (L_red + 20) u sum |terms|, apply 8 u (|scale gg| + |k2| + |xhat k3|), u = 2^-24.
    Two runs into fresh guard-banded buffers are bit-identical and leave the canaries intact; a point of weight 0 outside stat_mask
    receives a gradient of exactly 0."""
    b, c, n = shape
    figures = {}
    for slope in W.SLOPES:
        for soft in (False, True):
            t, ref = W.kernel_case(b, c, n, na, slope, soft)
            d = {k: v.to(dev) for k, v in W.as_torch(t).items()}
            got = _twice(lambda: _run_entries(dev, d, b, c, n, na, slope, '_wide'))
            for k, v in W.ratios(_named(got), ref, n).items():
                figures[k] = max(figures.get(k, 0.0), v)
            if not soft:
                zero = np.broadcast_to(((t['w'] == 0) & (t['stat_mask'] == 0)).reshape(b, 1, n, 1), got['gx_masked'].shape)
                assert float(np.abs(got['gx_masked'][zero]).max() if zero.any() else 0.0) == 0.0
    print(f'error / bound at na = {na}, (b, c, n) = {shape}:', {k: round(v, 3) for k, v in figures.items()})
    for k, v in figures.items():
        assert v <= 1.0, (k, v)


# ---- (b) the overlap of the two domains ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(2, 3, 17), (2, 2, 131)])
def test_at_60_anchors_the_wide_and_narrow_entries_agree(dev, shape):
    """both families at 60 anchors: the summation orders differ (chains over every 16th point folded over 4 waves here, over every 64th point
    folded over 16 rows there), so each element is within the SUM of the two kernels' bounds -- the narrow ones those of
    tests/test_gpu_inv_slot_head.py: L_fwd = ceil(n / 64) + 2 + 16 + 1, L_red = ceil(n / 64) + 2 + 2 + 4"""
    b, c, n = shape
    na = 60
    for slope in W.SLOPES:
        for soft in (False, True):
            t, ref = W.kernel_case(b, c, n, na, slope, soft)
            d = {k: v.to(dev) for k, v in W.as_torch(t).items()}
            wide = _named(_twice(lambda: _run_entries(dev, d, b, c, n, na, slope, '_wide')))
            narrow = _named(_twice(lambda: _run_entries(dev, d, b, c, n, na, slope, '')))
            l_fwd, l_red = -(-n // 64) + 2 + 16 + 1, -(-n // 64) + 2 + 2 + 4
            narrow_bound = {'fwd': (l_fwd + 20) * U * ref['fwd_abs'], 'reduce g': (l_red + 20) * U * ref['sg_abs'],
                            'reduce g xhat': (l_red + 20) * U * ref['sgx_abs'], 'apply, stat_mask': 8 * U * ref['gx_abs_masked'],
                            'apply, null': 8 * U * ref['gx_abs_null']}
            for k, (_, bound) in W.bounds(ref, n).items():
                r = W.worst_ratio(wide[k], np.asarray(narrow[k], np.float64), bound + narrow_bound[k])
                assert r <= 1.0, (slope, soft, k, r)


# ---- (c) the fused node against the unfused composition ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('per_cloud', [True, False], ids=['per_cloud', 'whole_batch'])
@pytest.mark.parametrize('training', [True, False])
def test_fused_node_at_240_anchors_equals_the_unfused_composition(dev, calls, training, per_cloud):
    """tests/test_gpu_inv_slot_head.py's test_fused_node_equals_the_unfused_composition on a [3,8,45,240] map, at its bars: per cloud
    _subset_batchnorm_act + slot_masked_mean, whole batch _BNAct + slot_masked_mean; a 1-point subset; output, every gradient, running
    statistics and num_batches_tracked; the pre-norm bias's gradient exactly 0 in training mode.  The fused side has called the three _wide
    entries and no narrow one, and no torch expression ran on either side."""
    import vgtk.so3conv.heads as H
    from vgtk.so3conv.blocks import _BNAct
    torch.manual_seed(17)
    B, C, P, A = 3, 8, 45, 240
    y0 = torch.randn(B, C, P, A, device=dev) * 1.7 + 0.4
    bias0 = torch.randn(C, device=dev)
    member = torch.rand(B, P, device=dev) > 0.4
    member[:, 0] = True
    member[1] = False; member[1, 7] = True                                    # a 1-point subset
    mask = member.float()
    probe = torch.randn(B, C, A, device=dev)
    res, names = [], []
    for fused in (False, True):
        bn = torch.nn.BatchNorm2d(C).to(dev).train(training)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
            bn.running_mean.copy_(torch.linspace(-0.2, 0.6, C)); bn.running_var.copy_(torch.linspace(0.7, 2.0, C))
        y, bias = y0.clone().requires_grad_(True), bias0.clone().requires_grad_(True)
        del calls[:]
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
        names.append(set(calls))
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
    assert MEAN_WIDE <= names[1] and not (MEAN_NARROW & names[1]), names[1]
    assert {'eap_slot_masked_mean_wide_fwd_f32', 'eap_slot_masked_mean_wide_bwd_f32'} <= names[0], names[0]
    if per_cloud:
        assert (FLAT_CLOUD if training else FLAT_CLOUD - {'eap_bn_stats_masked_f32'}) <= names[0], names[0]


# ---- (d) the per-cloud norm against float64 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('training', [True, False])
def test_subset_batchnorm_act_at_240_anchors_against_float64(dev, calls, training):
    """_subset_batchnorm_act on a [3,8,37,240] map, three clouds with 21, 4 and 1 members, against _subset_batchnorm_act_torch evaluated in
    float64 on the same float32 inputs: forward, dy, dgamma, dbeta, dbias and the running statistics at the bars of the fused node's test;
    training and eval mode; slope 0.01, the pose head's regressor.  The four flat per-cloud entries of csrc/bn_act.hip ran."""
    import vgtk.so3conv.heads as H
    gen = torch.Generator().manual_seed(23)
    B, C, P, A = 3, 8, 37, 240
    slope = 0.01
    y0 = torch.randn(B, C, P, A, generator=gen) * 1.7 + 0.4
    bias0 = torch.randn(C, generator=gen)
    member = torch.zeros(B, P, dtype=torch.bool)
    for i, k in enumerate((21, 4, 1)):
        member[i, torch.randperm(P, generator=gen)[:k]] = True
    # the gradient reaches every point (members and others), as it does behind the pose head's regressor
    probe = torch.randn(B, C, P, A, generator=gen) * member.view(B, 1, P, 1) + 0.1 * torch.randn(B, C, P, A, generator=gen)
    res = []
    for dtype, device in ((torch.float64, 'cpu'), (torch.float32, dev)):
        bn = torch.nn.BatchNorm2d(C).train(training)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
            bn.running_mean.copy_(torch.linspace(-0.2, 0.6, C)); bn.running_var.copy_(torch.linspace(0.7, 2.0, C))
        bn = bn.to(device=device, dtype=dtype)
        y, bias = y0.to(device=device, dtype=dtype).requires_grad_(True), bias0.to(device=device, dtype=dtype).requires_grad_(True)
        mask = member.to(device=device, dtype=dtype)
        if dtype == torch.float64:
            out = calls.torch['_subset_batchnorm_act_torch'](y, bias, mask, bn, slope)
            if training:
                bn.num_batches_tracked.add_(B)
        else:
            del calls[:]
            out = H._subset_batchnorm_act(y, bias, mask, bn, slope)
        (out * probe.to(device=device, dtype=dtype)).sum().backward()
        res.append(dict(out=out.detach(), dy=y.grad, dbias=bias.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean.clone(),
                        running_var=bn.running_var.clone(), batches=bn.num_batches_tracked.clone()))
    bars = dict(out=BAR_OUT, dy=BAR_DFEATS, dbias=BAR_DPARAM, dgamma=BAR_DPARAM, dbeta=BAR_DPARAM, running_mean=BAR_RUNNING, running_var=BAR_RUNNING)
    top = float(res[0]['dy'].abs().max())
    for k, bar in bars.items():
        want, got = res[0][k].cpu().numpy(), res[1][k].cpu().numpy()
        if k == 'dbias' and training:              # absorbed by the cloud's mean: rounding noise in float64, exactly zero in the fused backward
            assert np.abs(got).max() == 0.0 and np.abs(want).max() < 1e-9 * top * P * A
            continue
        assert rel_err(got, want) < bar, (k, rel_err(got, want))
    assert int(res[0]['batches']) == int(res[1]['batches']) == (B if training else 0)
    assert set(calls) == (FLAT_CLOUD if training else FLAT_CLOUD - {'eap_bn_stats_masked_f32'}), set(calls)


# ---- (e) the module against the reference's fixture -------------------------------------------------------------------------------------------------

def _functional(res, g):
    return sum((gi * r).sum() for gi, r in zip(g, res))


@pytest.mark.parametrize('batched', [False, True], ids=['per_cloud_loop', 'over_subsets'])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('tag', ['rel', 'abs'])
def test_module_on_a_240_anchor_map_matches_reference_golden(dev, golden, calls, tag, training, batched):
    """InvOutBlockOursWithMask (kanchor 60) on a 240-anchor map, where the reference's PointnetSO3ConvOurs takes its tot_anchors branch
    (base_so3conv.py:L1173-1176, L1196), called as the model calls it (once per cloud, batch 1, mask=None, on the gathered subset: 21, 4 and 1
    points) and as inv_head_over_subsets on the three clouds at once, against the reference class's outputs, running statistics and gradients
    at the bars of tests/test_gpu_inv_slot_head.py's test_module_matches_reference_golden.  All three _wide mean entries ran, no narrow one
    and no torch expression."""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    G = golden('inv_slot_head_2d.npz')
    mode = 'train' if training else 'eval'
    head = W.make_head_2d(tag)
    head.load_state_dict(state_of(G, tag))
    head = head.to(dev).train(training)
    xyz, feats, member, g = (v.to(dev) if torch.is_tensor(v) else tuple(e.to(dev) for e in v) for v in inputs_of(G))
    assert feats.shape == (3, 4, 37, 240) and member.sum(1).tolist() == [21, 4, 1]
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
                assert int(v) == int(G[f'{tag}_after_{k}']) == 3, k
    names = [n for n, _ in head.named_parameters()]
    grads = torch.autograd.grad(_functional(res, g), [feats] + list(head.parameters()), allow_unused=True)
    assert rel_err(pack_members(grads[0], member).cpu().numpy(), np.asarray(G[f'{tag}_{mode}_grad_feats'])) < BAR_DFEATS
    assert float(grads[0].permute(0, 2, 1, 3)[~member].abs().max()) == 0.0, 'points outside the subset must receive no gradient'
    check_param_grads(dict(zip(names, grads[1:])), G, tag, training, BAR_DPARAM)
    if training:                  # the fused node's own absorbed gradient is exactly zero
        lin_bias = grads[1 + names.index('linear.0.bias')]
        assert lin_bias is None or float(lin_bias.abs().max()) == 0.0
    assert MEAN_WIDE <= set(calls) and not (MEAN_NARROW & set(calls)), set(calls)


# ---- (f) the pose head on point subsets --------------------------------------------------------------------------------------------------------------

def _pose_inputs(dev, pooling):
    import vgtk.so3conv as sptk
    torch.manual_seed(3)
    B, C, N, A = 3, 16, 37, 240
    head = sptk.SO3OutBlockRTWithMaskSep({'dim_in': C, 'mlp': [32, 32], 'kanchor': 60, 'temperature': 3.0}, norm=1, pooling_method=pooling,
                                         pred_axis=True, pred_pv_points=True, pred_central_points=True).to(dev)
    feats = torch.randn(B, C, N, A, device=dev)
    xyz = torch.randn(B, 3, N, device=dev) * 0.3
    member = torch.rand(B, N, device=dev) > 0.5
    member[:, 0] = True
    member[1, 4:] = False; member[1, :4] = True                    # a 4-point subset
    return head, feats, xyz, member, W.tot_anchors().to(dev)


@pytest.mark.parametrize('pooling', ['max', 'mean'])
def test_pose_head_over_subsets_on_a_240_anchor_map_equals_the_per_cloud_loop(dev, calls, pooling):
    """tests/test_gpu_lists_and_modules.py's test_pose_head_over_subsets_equals_the_per_cloud_loop on a [3,16,37,240] map with the 240
    tot_anchors, at its bars (outputs 2e-5, running statistics 1e-5, d feats 5e-5, parameter gradients 1e-4; a bias in front of a
    training-mode norm exactly zero): the head called once per cloud, batch 1, on the gathered subset with mask=None.  The batched form has
    called the four flat per-cloud entries and the wide pooling, and no torch expression ran."""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    head, feats, xyz, member, anchors = _pose_inputs(dev, pooling)
    B = feats.shape[0]
    keys = ('R', 'T', 'axis', 'pv_points', 'central_points')
    for training in (True, False):
        ref_head, fast_head = copy.deepcopy(head).train(training), copy.deepcopy(head).train(training)
        gen = torch.Generator().manual_seed(11)
        f_ref = feats.clone().requires_grad_(True)
        outs = []
        for b in range(B):
            sel = member[b].nonzero().squeeze(1)
            fx, px = f_ref[b:b + 1, :, sel].contiguous(), xyz[b:b + 1, :, sel].contiguous()
            outs.append(ref_head(zptk.SphericalPointCloud(px, fx, None), None, fx, trans_xyz=px, anchors=anchors.unsqueeze(0)))
        want = {k: torch.cat([o[k] for o in outs], 0) for k in keys}
        probes = {k: torch.randn(want[k].shape, generator=gen).to(dev) for k in keys}
        sum((want[k] * probes[k]).sum() for k in keys).backward()
        f_fast = feats.clone().requires_grad_(True)
        del calls[:]
        got = sptk.pose_head_over_subsets(fast_head, f_fast, xyz, member, anchors)
        sum((got[k] * probes[k]).sum() for k in keys).backward()
        seen = set(calls)
        for k in keys:
            assert got[k].shape == want[k].shape, k
            assert rel_err(got[k].detach().cpu().numpy(), want[k].detach().cpu().numpy()) < 2e-5, (training, k)
        for (k, v), (_, w) in zip(ref_head.state_dict().items(), fast_head.state_dict().items()):
            if 'running' in k:
                assert rel_err(w.cpu().numpy(), v.cpu().numpy()) < 1e-5, k
            if 'num_batches' in k:
                assert int(v) == int(w), k
        assert rel_err(f_fast.grad.cpu().numpy(), f_ref.grad.cpu().numpy()) < 5e-5, training
        assert (f_fast.grad.permute(0, 2, 1, 3)[~member] == 0).all(), 'points outside the subset must receive no gradient'
        top = max(float(p_.grad.abs().max()) for p_ in ref_head.parameters() if p_.grad is not None)
        for (k, v), (_, w) in zip(ref_head.named_parameters(), fast_head.named_parameters()):
            if v.grad is None:
                assert w.grad is None or w.grad.abs().max().item() == 0.0, k
                continue
            ref_g = v.grad.cpu().numpy()
            if training and k.endswith('.bias') and k.startswith(('linear.', 'trans_linear.', 'regressor_dense_layer.0.')):
                assert np.abs(ref_g).max() < 1e-4 * top and (w.grad is None or float(w.grad.abs().max()) == 0.0), k
            else:
                assert rel_err(w.grad.cpu().numpy(), ref_g) < 1e-4, (training, k)
        pool = 'eap_masked_max_wide' if pooling == 'max' else 'eap_slot_masked_mean_wide'
        assert (FLAT_CLOUD if training else FLAT_CLOUD - {'eap_bn_stats_masked_f32'}) | {pool + '_fwd_f32', pool + '_bwd_f32'} <= seen, seen


# ---- (g) the per-slot forms: library kernels only, bit-identical run to run ----------------------------------------------------------------------------

def test_the_slot_group_forms_at_240_anchors_run_library_kernels_only(dev, calls):
    """inv_heads_over_slot_groups and pose_head_over_slot_groups on 64-point clouds with 240 anchors: slot 0 small (gathered), slot 1 absent
    from cloud 1 and slot 2 large (the masked form on the full clouds).  They equal the per-subset forms on the same memberships at the
    output bars of the tests above, two runs are bit-identical, forward and backward, every family of kernels was called and no torch
    expression stood in for one."""
    import vgtk.so3conv as sptk
    torch.manual_seed(6)
    B, C, N, A = 2, 16, 64, 240
    params = {'dim_in': C, 'mlp': [24], 'fc': [24], 'k': 24, 'kanchor': 60, 'temperature': 3.0}
    inv_heads = [sptk.InvOutBlockOursWithMask(params, norm=1, pooling_method='attention', use_pointnet=True, use_abs_pos=a,
                                              return_point_pooling_feature=True).to(dev) for a in (False, True, False)]
    pose_heads = [sptk.SO3OutBlockRTWithMaskSep({'dim_in': C, 'mlp': [24], 'kanchor': 60, 'temperature': 3.0}, norm=1, pooling_method=p).to(dev)
                  for p in ('mean', 'max', 'mean')]
    labels = torch.full((B, N), 2, device=dev, dtype=torch.long)    # slot 2: 24 points of cloud 0, 44 of cloud 1
    labels[:, :20] = 0                                              # slot 0: 20 points of both clouds
    labels[0, 20:40] = 1                                            # slot 1: 20 points of cloud 0, none of cloud 1
    groups = sptk.slot_point_groups(labels, 3)
    assert groups[0].shape[1] * 10 < N * 9 and groups[1].shape[1] * 10 >= N * 9 and groups[2].shape[1] * 10 >= N * 9
    feats = torch.randn(B, C, N, A, device=dev)
    xyz = torch.randn(B, 3, N, device=dev) * 0.3
    anchors = W.tot_anchors().to(dev)

    def run():
        f = feats.clone().requires_grad_(True)
        inv = sptk.inv_heads_over_slot_groups(copy.deepcopy(inv_heads), f, xyz, labels)
        pose = sptk.pose_head_over_slot_groups(copy.deepcopy(pose_heads), f, xyz, labels, anchors)
        outs = [t for r in inv for t in r] + [o[k] for o in pose for k in ('R', 'T')]
        sum((o * o).sum() for o in outs).backward()
        return [o.detach() for o in outs] + [f.grad]

    first = run()
    seen = set(calls)
    second = run()
    for a_, b_ in zip(first, second):
        assert torch.equal(a_, b_), 'two runs must be bit-identical'
    assert MEAN_WIDE <= seen and FLAT_CLOUD <= seen and not (MEAN_NARROW & seen), seen
    assert {'eap_rows_gather_f32', 'eap_slot_masked_mean_wide_fwd_f32', 'eap_masked_max_wide_fwd_f32'} <= seen, seen
    member = [labels == s_ for s_ in range(3)]
    member = [m | (m.sum(1, keepdim=True) == 0) for m in member]
    for s_ in range(3):
        want = sptk.inv_head_over_subsets(copy.deepcopy(inv_heads[s_]), feats, xyz, member[s_])
        for k in range(3):
            assert rel_err(first[3 * s_ + k].cpu().numpy(), want[k].detach().cpu().numpy()) < BAR_OUT, (s_, k)
        want = sptk.pose_head_over_subsets(copy.deepcopy(pose_heads[s_]), feats, xyz, member[s_], anchors)
        for j, k in enumerate(('R', 'T')):
            assert rel_err(first[9 + 2 * s_ + j].cpu().numpy(), want[k].detach().cpu().numpy()) < 2e-5, (s_, k)
