"""CPU: the wide twins of the fused BatchNorm + leaky_relu + point-mean entries (csrc/heads.hip at Q = 64, eap_bn_act_cloud_mean_wide_*: anchor
rows of up to 256 floats, the 240 of a `use_2d` map; SPConvNets/utils/base_so3conv.py:L1076-1107) as far as they go without a device: the four
C-ABI entries on calls that return before they launch (arity, empty batch, point and anchor counts, null and misaligned operands), the routing
of vgtk.so3conv.heads._norm_act_point_mean and _subset_batchnorm_act by anchor count with the library stubbed, and the bounds
tests/test_gpu_inv_slot_head_wide.py holds the kernels to (tests/inv_slot_wide_common.py): a float32 emulation of the kernels in their own
order of operations must pass them, a result with one wrong element must fail them."""
import numpy as np
import pytest
import torch

import inv_slot_wide_common as W

INVALID_VALUE = 1           # hipErrorInvalidValue

# name -> (pointer parameters in order, those moved by 16-byte words)
ENTRIES = {
    'eap_bn_act_cloud_mean_wide_fwd_f32': (('x', 'scale', 'shift', 'w', 'inv_den', 'out'), ('x', 'out')),
    'eap_bn_act_cloud_mean_wide_bwd_reduce_f32': (('g', 'x', 'scale', 'shift', 'mean', 'invstd', 'w', 'inv_den', 'pg', 'pgx'), ('g', 'x')),
    'eap_bn_act_cloud_mean_wide_bwd_apply_f32': (('g', 'x', 'scale', 'shift', 'mean', 'invstd', 'k2', 'k3', 'w', 'inv_den', 'stat_mask', 'gx'),
                                                 ('g', 'x', 'gx')),
}
ARITY = {'eap_bn_act_cloud_mean_wide_fwd_f32': 12, 'eap_bn_act_cloud_mean_wide_bwd_reduce_f32': 16, 'eap_bn_act_cloud_mean_wide_bwd_apply_f32': 18}


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def _args(name, pointers=None, b=3, c=8, n=40, na=240):
    """(b, c, n, na, slope, pointers (null unless given: {parameter: address}) ..., null stream)"""
    return (b, c, n, na, 0.0) + tuple((pointers or {}).get(p) for p in ENTRIES[name][0]) + (None,)


def _short(name):
    return name[len('eap_'):-len('_f32')]


def _addresses(name):
    """every pointer of the entry non-null and 16-byte aligned (the addresses are not memory: nothing may be launched)"""
    return {p: 0x10000 * (i + 1) for i, p in enumerate(ENTRIES[name][0])}


def test_the_four_entries_have_the_headers_arity_and_their_narrow_twins_parameters(hip):
    for name, count in ARITY.items():
        twin = getattr(hip.abi, name.replace('_wide', ''))
        assert len(getattr(hip.abi, name).argtypes) == count == len(_args(name)), name
        assert list(getattr(hip.abi, name).argtypes) == list(twin.argtypes), name
    assert list(hip.abi.eap_bn_act_cloud_mean_wide_parts.argtypes) == list(hip.abi.eap_bn_act_cloud_mean_parts.argtypes)
    assert len(hip.abi.eap_bn_act_cloud_mean_wide_parts.argtypes) == 1


def test_an_empty_batch_returns_before_a_pointer_is_touched(hip):
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, b=0)) == 0, name
        assert getattr(hip.abi, name)(*_args(name, c=0)) == 0, name
        assert getattr(hip.abi, name)(*_args(name, b=0, na=6, n=0)) == 0, name


def test_no_points_are_refused_as_by_the_narrow_twins(hip):
    for name in ENTRIES:
        for n in (0, -3):
            assert getattr(hip.abi, name)(*_args(name, _addresses(name), n=n)) == INVALID_VALUE, name
            msg = hip.abi.eap_last_error().decode()
            assert _short(name) in msg and 'no points' in msg, msg
            assert getattr(hip.abi, name.replace('_wide', ''))(*_args(name, n=n, na=60)) == INVALID_VALUE, name


@pytest.mark.parametrize('na', [0, 2, 6, 258, 260, -4])
def test_an_anchor_count_outside_the_domain_is_refused(hip, na):
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, _addresses(name), na=na)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert _short(name) in msg and 'multiple of 4, at most 256' in msg, msg


def test_a_null_required_pointer_is_refused(hip):
    """every pointer but stat_mask, one at a time; a null stat_mask alone is no refusal (the entry then goes on to the alignment rule, which an
    operand at 0x...4 fails: nothing is launched)"""
    for name, (ptrs, wide) in ENTRIES.items():
        base = _addresses(name)
        for p in ptrs:
            if p == 'stat_mask':
                assert getattr(hip.abi, name)(*_args(name, dict(base, stat_mask=None, gx=base['gx'] + 4))) == INVALID_VALUE
                assert 'must be 16-byte aligned' in hip.abi.eap_last_error().decode()
                continue
            assert getattr(hip.abi, name)(*_args(name, dict(base, **{p: None}))) == INVALID_VALUE, (name, p)
            msg = hip.abi.eap_last_error().decode()
            assert _short(name) in msg and 'null' in msg, (name, p, msg)


def test_a_16_byte_operand_off_its_boundary_is_refused(hip):
    for name, (ptrs, wide) in ENTRIES.items():
        base = _addresses(name)
        for p in wide:
            for off in (4, 8, 12):
                assert getattr(hip.abi, name)(*_args(name, dict(base, **{p: base[p] + off}))) == INVALID_VALUE, (name, p, off)
                msg = hip.abi.eap_last_error().decode()
                assert _short(name) in msg and 'must be 16-byte aligned' in msg, (name, p, msg)


def test_sizes_beyond_the_launch_limits_are_refused(hip):
    """more than 65535 clouds (grid.y); nothing is launched"""
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, _addresses(name), b=65536)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert _short(name) in msg and 'launch limits' in msg, msg


def test_the_backward_reduction_leaves_one_partial_per_wave(hip):
    """csrc/heads.hip at Q = 64 bn_act_mean_bwd_reduce_kernel<64>: a block of 4 waves, each summed by the shuffle tree to one partial -- the count
    the emulation of tests/inv_slot_wide_common.py adds in float64"""
    for n in (1, 3, 33, 700, 4096):
        assert hip.abi.eap_bn_act_cloud_mean_wide_parts(n) == W.WAVES == 4
    assert hip.abi.eap_bn_act_cloud_mean_wide_parts(0) == 0


# ---- the routing by anchor count ---------------------------------------------------------------------------------------------------------------

class _AsDevice(torch.Tensor):
    """a host tensor that answers is_cuda = True: the wrappers' device check passes and the torch expressions of the fallback run here"""
    is_cuda = property(lambda self: True)


def _as_device(t):
    return t.as_subclass(_AsDevice)


class Reached(Exception):
    pass


@pytest.fixture
def first_call(monkeypatch):
    """_hip.call replaced by a stand-in that records the entry's name and stops"""
    from vgtk import _hip

    def record(name, *a, **k):
        raise Reached(name)
    monkeypatch.setattr(_hip, 'call', record)


@pytest.fixture
def no_library(monkeypatch):
    from vgtk import _hip

    def refuse(name, *a, **k):
        raise AssertionError(f'{name}: the fallback must not reach the library')
    monkeypatch.setattr(_hip, 'call', refuse)


def _node_inputs(na, training=True):
    gen = torch.Generator().manual_seed(na)
    b, c, p = 2, 3, 5
    y = torch.randn(b, c, p, na, generator=gen)
    mask = (torch.rand(b, p, generator=gen) > 0.4).float()
    mask[:, 0] = 1.0
    bn = torch.nn.BatchNorm2d(c).train(training)
    return y, torch.randn(c, generator=gen), mask, bn


@pytest.mark.parametrize('na', [68, 240, 256])
def test_wide_anchor_counts_reach_the_library(first_call, na):
    """_norm_act_point_mean: per-cloud statistics first (eap_bn_stats_masked_f32), and in eval mode, where no statistics are taken, the wide
    forward itself; _subset_batchnorm_act: the flat per-cloud entries of csrc/bn_act.hip"""
    import vgtk.so3conv.heads as H
    y, bias, mask, bn = _node_inputs(na)
    with pytest.raises(Reached, match='eap_bn_stats_masked_f32'):
        H._norm_act_point_mean(_as_device(y), bias, mask, 1.0 / mask.sum(1), mask, bn, 0.0)
    with pytest.raises(Reached, match='eap_bn_stats_masked_f32'):
        H._subset_batchnorm_act(_as_device(y), bias, mask, bn, 0.0)
    assert int(bn.num_batches_tracked) == 2 * y.shape[0]
    bn.eval()
    with pytest.raises(Reached, match='eap_bn_act_cloud_mean_wide_fwd_f32'):
        H._norm_act_point_mean(_as_device(y), bias, mask, 1.0 / mask.sum(1), mask, bn, 0.0)
    with pytest.raises(Reached, match='eap_bn_act_cloud_fwd_f32'):
        H._subset_batchnorm_act(_as_device(y), bias, mask, bn, 0.0)


@pytest.mark.parametrize('na', [60, 68, 240, 256])
def test_the_node_picks_its_entries_by_anchor_count(monkeypatch, na):
    """_NormActPointMean's forward and backward through the three wrappers of vgtk/_hip.py (bn_act_cloud_mean_fwd / _bwd_reduce / _bwd_apply,
    which choose the family) with _hip.call replaced by a recorder that zeroes the outputs: 60 anchors call the three narrow entries, 68 to
    256 the three wide ones, the partials have the family's count, and nothing else of the library is needed in eval mode"""
    import vgtk.so3conv.heads as H
    from vgtk import _hip
    seen = []

    def record(name, ref, *a, **k):
        seen.append((name, a))
        for out in a[-2 if name.endswith('_bwd_reduce_f32') else -1:]:        # pg and pgx; out; gx
            out.zero_()
    monkeypatch.setattr(_hip, 'call', record)
    monkeypatch.setattr(H.L, '_aligned16', lambda t: t.contiguous())
    y, bias, mask, bn = _node_inputs(na, training=False)
    y.requires_grad_(True)
    out = H._norm_act_point_mean(y, bias, mask, 1.0 / mask.sum(1), mask, bn, 0.0)
    out.sum().backward()
    fam = 'eap_bn_act_cloud_mean_wide' if na > 64 else 'eap_bn_act_cloud_mean'
    assert [name for name, _ in seen] == [fam + '_fwd_f32', fam + '_bwd_reduce_f32', fam + '_bwd_apply_f32'], seen
    assert seen[1][1][-2].shape == seen[1][1][-1].shape == (y.shape[0], y.shape[1], W.WAVES if na > 64 else 16)
    assert float(y.grad.abs().max()) == 0.0


def test_60_anchors_still_reach_the_narrow_entries(first_call):
    import vgtk.so3conv.heads as H
    y, bias, mask, bn = _node_inputs(60, training=False)
    with pytest.raises(Reached, match=r'eap_bn_act_cloud_mean_fwd_f32$'):
        H._norm_act_point_mean(_as_device(y), bias, mask, 1.0 / mask.sum(1), mask, bn, 0.0)
    with pytest.raises(Reached, match=r'eap_bn_act_cloud_fwd_f32$'):
        H._subset_batchnorm_act(_as_device(y), bias, mask, bn, 0.0)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('na', [1, 3, 260])
def test_other_anchor_counts_run_the_torch_expressions(no_library, na, training):
    """kanchor = 1, 3 and counts past 256: _norm_act_point_mean is _norm_act_point_mean_torch, _subset_batchnorm_act is
    _subset_batchnorm_act_torch, bit for bit, running statistics and num_batches_tracked included"""
    import copy
    import vgtk.so3conv.heads as H
    y, bias, mask, bn = _node_inputs(na, training)
    inv_den = 1.0 / mask.sum(1)
    for stat_mask in (mask, None):
        a, b_ = copy.deepcopy(bn), copy.deepcopy(bn)
        got = H._norm_act_point_mean(_as_device(y), bias, mask, inv_den, stat_mask, a, 0.2)
        want = H._norm_act_point_mean_torch(y, bias, mask, inv_den, stat_mask, b_, 0.2)
        assert torch.equal(torch.Tensor(got), want)
        for (k, v), (_, w_) in zip(a.state_dict().items(), b_.state_dict().items()):
            assert torch.equal(v, w_), k
        assert int(a.num_batches_tracked) == ((y.shape[0] if stat_mask is not None else 1) if training else 0)
    a, b_ = copy.deepcopy(bn), copy.deepcopy(bn)
    got = H._subset_batchnorm_act(_as_device(y), bias, mask, a, 0.0)
    b_.num_batches_tracked.add_(y.shape[0] if training else 0)
    assert torch.equal(torch.Tensor(got), H._subset_batchnorm_act_torch(y, bias, mask, b_, 0.0))
    for (k, v), (_, w_) in zip(a.state_dict().items(), b_.state_dict().items()):
        assert torch.equal(v, w_), k


def test_cumulative_average_batchnorm_is_refused_at_240_anchors_too():
    import vgtk.so3conv.heads as H
    y, bias, mask, bn = _node_inputs(240)
    bn.momentum = None
    with pytest.raises(NotImplementedError, match='momentum'):
        H._norm_act_point_mean(y, bias, mask, 1.0 / mask.sum(1), mask, bn, 0.0)
    with pytest.raises(NotImplementedError, match='momentum=None'):
        H._subset_batchnorm_act(y, bias, mask, bn, 0.0)


# ---- the bounds: the emulation passes them, a wrong element fails them ---------------------------------------------------------------------

def _last_off_by_one(a):
    a = np.array(a, order='C')
    a.reshape(-1)[-1] += 1.0
    return a


@pytest.mark.parametrize('na,shape', W.GRID)
def test_the_emulation_passes_the_bounds_and_a_wrong_element_fails_them(na, shape):
    """every output of the three kernels; the mutations: the last element of an output off by 1, and the forward's fold without the last wave, wherever that wave holds a point of some weight"""
    b, c, n = shape
    for slope in W.SLOPES:
        for soft in (False, True):
            t, ref = W.kernel_case(b, c, n, na, slope, soft)
            got = W.emulate(t, slope)
            for k, v in W.ratios(got, ref, n).items():
                assert v <= 1.0, (slope, soft, k, v)
            for k, v in W.ratios({k: _last_off_by_one(v) for k, v in got.items()}, ref, n).items():
                assert v > 1.0, (slope, soft, k, v)
            if n >= W.WAVES and bool((t['w'][:, W.WAVES - 1::W.WAVES] != 0).any()):
                assert W.ratios(W.emulate(t, slope, wave_fold=False), ref, n)['fwd'] > 1.0, (slope, soft)
