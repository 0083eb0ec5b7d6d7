"""CPU: the per-slot shape-code head (vgtk.so3conv.InvOutBlockOursWithMask, SPConvNets/utils/base_so3conv.py:L1013-1205) as far as it goes
without a device: the three C-ABI entries of its fused norm + point-mean pass (include/eap_hip.h, csrc/heads.hip) on calls that return
before they launch, the class's state_dict keys, and the collapsed form of the pointnet stage -- `embed` applied to the point MEANS, then
BatchNorm1d, ReLU and the attention pooling (vgtk.so3conv.inv_head_tail, pure torch) -- against tests/golden/inv_slot_head.npz, which the
reference class produced with the embed layer on every point."""
import numpy as np
import pytest
import torch

from inv_slot_common import (BAR_DFEATS, BAR_DPARAM, BAR_OUT, BAR_RUNNING, check_param_grads, inputs_of, make_head, pack_members, rel_err,
                             state_of)

INVALID_VALUE = 1           # hipErrorInvalidValue
ENTRIES = {'eap_bn_act_cloud_mean_fwd_f32': 12, 'eap_bn_act_cloud_mean_bwd_reduce_f32': 16, 'eap_bn_act_cloud_mean_bwd_apply_f32': 18}


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def _args(count, b, c, n, na):
    """(b, c, n, na, slope, null pointers ..., null stream)"""
    return (b, c, n, na, 0.0) + (None,) * (count - 5)


def test_the_three_entries_have_the_headers_arity(hip):
    for name, count in ENTRIES.items():
        assert len(getattr(hip.abi, name).argtypes) == count, name
    assert len(hip.abi.eap_bn_act_cloud_mean_parts.argtypes) == 1
    assert hip.abi.eap_abi_version() == 1


def test_an_empty_batch_returns_before_a_pointer_is_touched(hip):
    for name, count in ENTRIES.items():
        assert getattr(hip.abi, name)(*_args(count, 0, 8, 40, 60)) == 0, name
        assert getattr(hip.abi, name)(*_args(count, 3, 0, 40, 60)) == 0, name


@pytest.mark.parametrize('na', [0, 6, 68])
def test_an_anchor_count_the_16_byte_rows_do_not_take_is_refused(hip, na):
    for name, count in ENTRIES.items():
        assert getattr(hip.abi, name)(*_args(count, 3, 8, 40, na)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert name[len('eap_'):-len('_f32')] in msg and 'multiple of 4, at most 64' in msg, msg


POINTERS = {'eap_bn_act_cloud_mean_fwd_f32': ('x', 'scale', 'shift', 'w', 'inv_den', 'out'),
            'eap_bn_act_cloud_mean_bwd_reduce_f32': ('g', 'x', 'scale', 'shift', 'mean', 'invstd', 'w', 'inv_den', 'pg', 'pgx'),
            'eap_bn_act_cloud_mean_bwd_apply_f32': ('g', 'x', 'scale', 'shift', 'mean', 'invstd', 'k2', 'k3', 'w', 'inv_den', 'stat_mask', 'gx')}


def test_a_null_required_pointer_is_refused(hip):
    """as by the _wide twins (tests/test_inv_slot_head_wide_host.py): every pointer but stat_mask, one at a time, the others non-null and
    16-byte aligned (addresses, not memory: nothing may be launched); a null stat_mask alone is no refusal (the entry then goes on to the
    alignment rule, which an operand at 0x...4 fails)"""
    for name, ptrs in POINTERS.items():
        base = {p: 0x10000 * (i + 1) for i, p in enumerate(ptrs)}
        call = lambda given: getattr(hip.abi, name)(3, 8, 40, 60, 0.0, *(given[p] for p in ptrs), None)
        for p in ptrs:
            if p == 'stat_mask':
                assert call(dict(base, stat_mask=None, gx=base['gx'] + 4)) == INVALID_VALUE
                assert 'must be 16-byte aligned' in hip.abi.eap_last_error().decode()
                continue
            assert call(dict(base, **{p: None})) == INVALID_VALUE, (name, p)
            msg = hip.abi.eap_last_error().decode()
            assert name[len('eap_'):-len('_f32')] in msg and 'a required pointer is null' in msg, (name, p, msg)


def test_the_backward_reduction_leaves_one_partial_per_wave_and_point_group(hip):
    """csrc/heads.hip bn_act_mean_bwd_reduce_kernel: a block of 4 waves, 4 point groups of 16 lanes each, one partial per group"""
    for n in (1, 33, 700, 4096):
        assert hip.abi.eap_bn_act_cloud_mean_parts(n) == 4 * 4
    assert hip.abi.eap_bn_act_cloud_mean_parts(0) == 0


@pytest.mark.parametrize('tag', ['rel', 'abs'])
def test_state_dict_keys_are_the_references(golden, tag):
    G = golden('inv_slot_head.npz')
    head = make_head(tag)
    assert list(head.state_dict().keys()) == list(state_of(G, tag).keys())
    head.load_state_dict(state_of(G, tag))
    assert isinstance(head.norm[1], torch.nn.BatchNorm1d) and head.pointnet.tot_anchors.shape == (240, 3, 3)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('tag', ['rel', 'abs'])
def test_embed_on_the_point_means_reproduces_the_reference(golden, tag, training):
    """mean_p embed([h_p ; A^T (x_p - mean x)]) = W_f mean_p h_p + W_x A^T mean_p (x_p - mean x) + bias in float32: the unary layer, its
    BatchNorm2d + ReLU and the point mean per cloud with torch on the CPU, then the package's tail for the three clouds at once.  A
    quarter of the bars the device path is held to (tests/test_gpu_inv_slot_head.py), so that it keeps three quarters for its own
    rounding."""
    import vgtk.so3conv as sptk
    G = golden('inv_slot_head.npz')
    mode = 'train' if training else 'eval'
    head = make_head(tag)
    head.load_state_dict(state_of(G, tag))
    head.train(training)
    xyz, feats, member, g = inputs_of(G)
    feats.requires_grad_(True)
    means, xyz_means = [], []
    for i in range(member.shape[0]):                                                  # cloud order: three BatchNorm2d updates
        sel = member[i].nonzero().squeeze(1)
        h = torch.relu(head.norm[0](head.linear[0](feats[i:i + 1][:, :, sel])))
        means.append(h.mean(2))
        xyz_means.append(xyz[i:i + 1][:, :, sel].mean(2))
    res = sptk.inv_head_tail(head, torch.cat(means, 0), torch.cat(xyz_means, 0) if tag == 'abs' else None, None, per_cloud=True)
    for name, got in zip(('pooled', 'code', 'logits'), res):
        ref = np.asarray(G[f'{tag}_{mode}_{name}'])
        assert got.shape == ref.shape, name
        assert rel_err(got.detach().numpy(), ref) < BAR_OUT / 4, (name, rel_err(got.detach().numpy(), ref))
    if training:
        for k, v in head.state_dict().items():
            if 'running' in k:
                assert rel_err(v.numpy(), np.asarray(G[f'{tag}_after_{k}'])) < BAR_RUNNING / 4, k
            if 'num_batches' in k:
                assert int(v) == int(G[f'{tag}_after_{k}']) == 3, k
    names = [n for n, _ in head.named_parameters()]
    grads = torch.autograd.grad(sum((gi * r).sum() for gi, r in zip(g, res)), [feats] + list(head.parameters()), allow_unused=True)
    assert rel_err(pack_members(grads[0], member).numpy(), np.asarray(G[f'{tag}_{mode}_grad_feats'])) < BAR_DFEATS / 4
    assert float(grads[0].permute(0, 2, 1, 3)[~member].abs().max()) == 0.0
    check_param_grads(dict(zip(names, grads[1:])), G, tag, training, BAR_DPARAM / 4)
