"""CPU: the C-ABI entries of IntraSO3Conv2D on the (60, 4) anchor axis (so3conv/modules.py:L350-373, so3conv/functional.py:L2606-2627)
without a GPU: they are declared, exported and bound with the header's arity; sizes outside their limits are refused before a pointer is
touched (null pointers throughout), empty problems return 0; the shape predicate of the split kernel, accepted baseline, every single
violation, accepted boundary values; the operator layer refuses host and float64 tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
INVALID_VALUE = 1                                         # hipErrorInvalidValue

# entry -> number of parameters in include/eap_hip.h (the stream included)
ENTRIES = {
    'eap_so3_intra_group2d_fwd_f32': 10,
    'eap_so3_intra_group2d_bwd_f32': 10,
    'eap_so3_intra_conv2d_f32': 12,
    'eap_so3_intra_conv2d_split_supported': 7,
    'eap_so3_intra_conv2d_bf16x3_f32': 12,
    'eap_so3_intra_conv2d_f16x2_f32': 14,
}


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def test_entries_are_declared_exported_and_bound(hip):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eap_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name, count in ENTRIES.items():
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert m, f'{name} is not declared'
        assert m.group(1).count(',') + 1 == count, name
        assert hasattr(lib, name), f'{name} is not exported'
        fn = getattr(hip.abi, name)
        assert len(fn.argtypes) == count and fn.restype is ctypes.c_int, name
    # the header cites the reference lines of the layer
    raw = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    assert 'so3conv/functional.py:L2606-2627' in raw and 'so3conv/modules.py:L350-373' in raw


def _calls(hip, b, o, c, p, na, nr, nt):
    """every launching entry with null pointers -> {name: return code}"""
    a = hip.abi
    return {
        'group2d_fwd': a.eap_so3_intra_group2d_fwd_f32(b, c, p, na, nr, nt, None, None, None, None),
        'group2d_bwd': a.eap_so3_intra_group2d_bwd_f32(b, c, p, na, nr, nt, None, None, None, None),
        'conv2d_f32': a.eap_so3_intra_conv2d_f32(b, o, c, p, na, nr, nt, None, None, None, None, None),
        'conv2d_bf16x3': a.eap_so3_intra_conv2d_bf16x3_f32(b, o, c, p, na, nr, nt, None, None, None, None, None),
        'conv2d_f16x2': a.eap_so3_intra_conv2d_f16x2_f32(b, o, c, p, na, nr, nt, None, None, None, None, None, None, None),
    }


@pytest.mark.parametrize('change,word', [(dict(nr=2), 'nr = 4'), (dict(na=68), '64 anchors'), (dict(nt=17), 'taps')])
def test_sizes_outside_the_limits_are_refused_before_a_pointer_is_touched(hip, change, word):
    size = dict(b=1, o=128, c=4, p=8, na=60, nr=4, nt=12)
    size.update(change)
    a = hip.abi
    for name, fn, nargs in (('group2d_fwd', a.eap_so3_intra_group2d_fwd_f32, 4), ('group2d_bwd', a.eap_so3_intra_group2d_bwd_f32, 4)):
        rc = fn(size['b'], size['c'], size['p'], size['na'], size['nr'], size['nt'], *([None] * nargs))
        assert rc == INVALID_VALUE, (name, change)
        assert word in a.eap_last_error().decode(), (name, a.eap_last_error().decode())
    for name, fn, nargs in (('conv2d_f32', a.eap_so3_intra_conv2d_f32, 5), ('conv2d_bf16x3', a.eap_so3_intra_conv2d_bf16x3_f32, 5),
                            ('conv2d_f16x2', a.eap_so3_intra_conv2d_f16x2_f32, 7)):
        rc = fn(size['b'], size['o'], size['c'], size['p'], size['na'], size['nr'], size['nt'], *([None] * nargs))
        assert rc == INVALID_VALUE, (name, change)
        assert word in a.eap_last_error().decode(), (name, a.eap_last_error().decode())
    assert a.eap_so3_intra_conv2d_split_supported(*(size[k] for k in ('b', 'o', 'c', 'p', 'na', 'nr', 'nt'))) == 0


def test_the_split_kernel_takes_twelve_taps_only(hip):
    a = hip.abi
    assert a.eap_so3_intra_conv2d_bf16x3_f32(1, 128, 4, 8, 60, 4, 16, None, None, None, None, None) == INVALID_VALUE
    assert 'nt = 12' in a.eap_last_error().decode()
    # a shape inside the limits that the tiles do not take is refused as a shape, with the predicate named
    assert a.eap_so3_intra_conv2d_bf16x3_f32(1, 64, 4, 8, 60, 4, 12, None, None, None, None, None) == INVALID_VALUE
    assert 'eap_so3_intra_conv2d_split_supported' in a.eap_last_error().decode()


def test_empty_problems_return_zero(hip):
    assert set(_calls(hip, 0, 128, 4, 8, 60, 4, 12).values()) == {0}
    assert set(_calls(hip, 1, 128, 4, 0, 60, 4, 12).values()) == {0}


BASE = dict(b=2, o=128, c=4, p=8, na=60, nr=4, nt=12)      # o = 128, p*240 = 1920 = 15 * 128, c*12 = 48 = 3 * 16
REJECTED = [dict(o=64), dict(o=192), dict(o=130), dict(p=7), dict(p=1), dict(p=9), dict(c=3), dict(c=1), dict(c=0), dict(nt=11), dict(nt=16),
            dict(nr=1), dict(nr=2), dict(nr=8), dict(na=0), dict(na=68), dict(na=-4), dict(p=(1 << 29) // 240 // 8 * 8 + 8)]
ACCEPTED = [dict(o=256), dict(o=384), dict(p=16), dict(p=24), dict(c=8), dict(c=128), dict(b=1), dict(na=64), dict(na=4, p=32),
            dict(p=(1 << 29) // 240 // 8 * 8 - 8)]


def test_split_predicate_table(hip):
    """o and p*na*nr multiples of 128 (at least 128 and 256), c*12 a multiple of 16, nt = 12, nr = 4, na <= 64, p*na*nr < 2^29"""
    def ask(**change):
        s = dict(BASE, **change)
        return int(hip.abi.eap_so3_intra_conv2d_split_supported(s['b'], s['o'], s['c'], s['p'], s['na'], s['nr'], s['nt']))

    assert ask() == 1
    for change in REJECTED:
        assert ask(**change) == 0, ('must be rejected', change)
    for change in ACCEPTED:
        assert ask(**change) == 1, ('must be accepted', change)
    # the 1-D predicate with p * 240 for the column count
    for s in ({}, dict(o=64), dict(p=7), dict(c=3), dict(o=256, p=16, c=8)):
        s = dict(BASE, **s)
        want = int(hip.abi.eap_so3_intra_conv_bf16x3_f32_supported(s['b'], s['o'], s['c'], 4 * s['p'], 60, 12))
        assert ask(**s) == want, s


def test_operator_layer_refuses_host_and_float64_tensors():
    import vgtk.so3conv.functional as L
    idx = torch.from_numpy(np.ascontiguousarray(L.get_intra_idx())).long()
    W = torch.zeros(7, 5 * 12)
    with pytest.raises(RuntimeError, match='intra_so3conv2d: float32 device tensors only'):
        L.intra_so3conv2d(torch.zeros(1, 5, 3, 240), W, idx)
    with pytest.raises(RuntimeError, match='intra_so3conv2d: float32 device tensors only'):
        L.intra_so3conv2d(torch.zeros(1, 5, 3, 240, dtype=torch.float64), W.double(), idx)


def test_host_tensors_keep_the_tensor_expression():
    """inputs the kernels do not take keep the reference's expression: same values as a restatement of the index_select form"""
    import vgtk.so3conv.functional as L
    torch.manual_seed(3)
    idx = torch.from_numpy(np.ascontiguousarray(L.get_intra_idx())).long()
    for dtype in (torch.float64, torch.float32):
        f = torch.randn(1, 2, 3, 240, dtype=dtype).requires_grad_(True)
        g = L.intra_so3conv_grouping_2D(idx, f)
        want = f.view(1, 2, 3, 60, 4)[:, :, :, idx].permute(0, 1, 4, 2, 3, 5).reshape(1, 2, 12, 3, 240)
        assert torch.equal(g, want) and g.requires_grad
