"""CPU: the five entries of csrc/norm_fold.hip (the per-channel bookkeeping of the conv + norm nodes, one launch per site) are declared in
include/eap_hip.h, exported and bound through the typed ABI, and each refuses -- with hipErrorInvalidValue and a message that starts with
its name, before any device call -- a null pointer, a size that is not positive and a size beyond the launch limits.  The pointers are
made-up addresses nothing may dereference; on a machine without a GPU a device call would answer with its own error instead.  The host
side keeps the tensor expressions for tensors that are not on the device and when vgtk._hip.NATIVE_NORM_GLUE is off."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
INVALID_VALUE = 1           # hipErrorInvalidValue
A = [0x10000000 + 0x100000 * i for i in range(16)]      # 16-byte aligned addresses, never read
NAMES = ['eap_norm_fold_train_f32', 'eap_norm_fold_bwd_f32', 'eap_so3_dense_zbound_f32', 'eap_so3_dense_gplanes_bound_f32',
         'eap_so3_dense_point_order']
ONE = 0x3FF0000000000000     # the bits of 1.0


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def test_entries_are_declared_exported_and_bound(hip):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eap_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(eap_[a-z0-9_]+)\s*\(', text))
    for name in NAMES:
        assert name in declared, f'{name} is not declared in include/eap_hip.h'
        assert hasattr(hip.lib, name), f'{name} is not exported'
        assert hasattr(hip.abi, name), f'{name} is not bound'
        assert not name.startswith(('eap_bn_', 'eap_narrow_conv', 'eap_gemm'))
    assert [len(getattr(hip.abi, n).argtypes) for n in NAMES] == [20, 20, 11, 12, 11]
    assert hip._f64_bits(1.0) == ONE and hip._f64_bits(-0.0) == -2 ** 63


def _train(hip, o=64, parts=7, stride=1, count=100, ptr=None):
    p = list(A[:13]) if ptr is None else ptr
    return hip.abi.eap_norm_fold_train_f32(o, parts, stride, count, ONE, ONE, *p, None)


def _bwd(hip, o=64, parts=7, b=2, na=60, count=100, ptr=None):
    p = list(A[:14]) if ptr is None else ptr
    return hip.abi.eap_norm_fold_bwd_f32(o, parts, b, na, count, *p, None)


def _zbound(hip, b=2, na=60, rp=16, p=64, ldz=1024, stride=64, ptr=None):
    q = list(A[:4]) if ptr is None else ptr
    return hip.abi.eap_so3_dense_zbound_f32(b, na, rp, p, ldz, stride, *q, None)


def _gbound(hip, b=2, o=64, c=64, na=60, ks=24, rp=16, ptr=None):
    q = list(A[:5]) if ptr is None else ptr
    return hip.abi.eap_so3_dense_gplanes_bound_f32(b, o, c, na, ks, rp, *q, None)


def _order(hip, b=2, p=100, words=16, ptr=None):
    q = list(A[:7]) if ptr is None else ptr
    return hip.abi.eap_so3_dense_point_order(b, p, words, *q, None)


def _nulled(k, i):
    return [None if j == i else a for j, a in enumerate(A[:k])]


REFUSED = [
    # (entry prefix of the message, words in it, call)
    *[('norm_fold_train', 'null pointer', lambda h, i=i: _train(h, ptr=_nulled(13, i))) for i in (0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12)],
    ('norm_fold_train', 'null pointer', lambda h: _train(h, ptr=_nulled(13, 5))),          # running_mean without running_var
    ('norm_fold_train', 'positive', lambda h: _train(h, o=0)),
    ('norm_fold_train', 'positive', lambda h: _train(h, parts=0)),
    ('norm_fold_train', 'positive', lambda h: _train(h, count=0)),
    ('norm_fold_train', 'positive', lambda h: _train(h, stride=0)),
    ('norm_fold_train', 'outside the launch limits', lambda h: _train(h, o=1 << 27)),
    *[('norm_fold_bwd', 'null pointer', lambda h, i=i: _bwd(h, ptr=_nulled(14, i))) for i in range(14)],
    ('norm_fold_bwd', 'positive', lambda h: _bwd(h, o=0)),
    ('norm_fold_bwd', 'positive', lambda h: _bwd(h, parts=-1)),
    ('norm_fold_bwd', 'positive', lambda h: _bwd(h, count=0)),
    ('norm_fold_bwd', 'positive', lambda h: _bwd(h, b=0)),
    ('norm_fold_bwd', 'positive', lambda h: _bwd(h, na=0)),
    ('norm_fold_bwd', '65535', lambda h: _bwd(h, b=65536)),
    ('norm_fold_bwd', 'outside the launch limits', lambda h: _bwd(h, o=1 << 27)),
    *[('so3_dense_zbound', 'null pointer', lambda h, i=i: _zbound(h, ptr=_nulled(4, i))) for i in range(4)],
    *[('so3_dense_zbound', 'positive', lambda h, k=k: _zbound(h, **{k: 0})) for k in ('b', 'na', 'rp', 'p', 'ldz')],
    ('so3_dense_zbound', 'multiples of 4', lambda h: _zbound(h, rp=18)),
    ('so3_dense_zbound', 'multiples of 4', lambda h: _zbound(h, ldz=1022)),
    ('so3_dense_zbound', 'ldz >= na * rp', lambda h: _zbound(h, ldz=956)),
    ('so3_dense_zbound', 'row stride', lambda h: _zbound(h, stride=12)),
    ('so3_dense_zbound', 'outside the launch limits', lambda h: _zbound(h, b=65536)),
    *[('so3_dense_gplanes_bound', 'null pointer', lambda h, i=i: _gbound(h, ptr=_nulled(5, i))) for i in range(5)],
    *[('so3_dense_gplanes_bound', 'positive', lambda h, k=k: _gbound(h, **{k: 0})) for k in ('b', 'o', 'c', 'na', 'ks', 'rp')],
    ('so3_dense_gplanes_bound', 'na <= 128', lambda h: _gbound(h, na=129)),
    ('so3_dense_gplanes_bound', 'below 2^31', lambda h: _gbound(h, b=1 << 20, c=1 << 12)),
    *[('so3_dense_point_order', 'null pointer', lambda h, i=i: _order(h, ptr=_nulled(7, i))) for i in range(7)],
    ('so3_dense_point_order', 'positive', lambda h: _order(h, b=0)),
    ('so3_dense_point_order', 'positive', lambda h: _order(h, p=0)),
    ('so3_dense_point_order', '16 or 32', lambda h: _order(h, words=24)),
    ('so3_dense_point_order', '16-byte aligned', lambda h: _order(h, ptr=[A[0], A[1] + 4] + A[2:7])),
    ('so3_dense_point_order', '16-byte aligned', lambda h: _order(h, ptr=A[:4] + [A[4] + 8] + A[5:7])),
    ('so3_dense_point_order', 'outside the launch limits', lambda h: _order(h, b=65536)),
]


@pytest.mark.parametrize('case', range(len(REFUSED)))
def test_refused_before_any_device_call(hip, case):
    entry, words, call = REFUSED[case]
    assert call(hip) == INVALID_VALUE
    msg = hip.abi.eap_last_error().decode()
    assert msg.startswith(entry) and words in msg, msg


def test_the_tensor_expressions_remain_off_the_device_and_with_the_switch_off(hip, monkeypatch):
    import vgtk.so3conv.functional as L
    from vgtk.so3conv.blocks import BatchNormLeakyReLU
    assert hip.NATIVE_NORM_GLUE is True
    ep = L.TrainEpilogue(BatchNormLeakyReLU(8))
    host, device = torch.zeros(2, 8, 4), types.SimpleNamespace(is_cuda=True)
    assert ep.takes_partials(device) and not ep.takes_partials(host)
    assert L._native_norm_bwd(device, 64, False) and not L._native_norm_bwd(host, 64, False)
    assert not L._native_norm_bwd(device, torch.tensor(64.0), True)          # (an exchanged element count: the SyncBatchNorm path)
    # `moments` itself is the tensor expressions, on any device: sums of a [2, 8, 4] tensor around a pivot
    x = torch.arange(64, dtype=torch.float64).view(2, 8, 4) / 7.0
    pivot = x[0, :, 0].clone()
    d = x - pivot[None, :, None]
    scale, shift, _ = ep.moments(d.sum((0, 2)), (d * d).sum((0, 2)), pivot, 8)
    ref = torch.rsqrt(x.var((0, 2), unbiased=False) + ep.norm.eps)
    assert torch.allclose(scale.double(), ref, rtol=1e-6) and torch.allclose(ep.stats[0], x.mean((0, 2)), rtol=1e-12)
    monkeypatch.setattr(hip, 'NATIVE_NORM_GLUE', False)
    assert not ep.takes_partials(device) and not L._native_norm_bwd(device, 64, False)
