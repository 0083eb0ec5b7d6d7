"""CPU: the entries of csrc/narrow_conv.hip (the first inter conv layer with its BatchNorm + leaky_relu, conv output never written) are
declared in include/eap_hip.h and exported, and each of them refuses -- with hipErrorInvalidValue and a message that names the
condition, before any device call -- more than 32 contraction indices, an output width that is not a multiple of 32, a row length
that is not a multiple of 4 and tensors that are not 16-byte aligned.  The pointers are made-up addresses nothing may dereference;
on a machine without a GPU a device call would answer with its own error instead."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
INVALID_VALUE = 1           # hipErrorInvalidValue
P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
X, GY, Y, ODD = 0x10000000, 0x20000000, 0x30000000, 0x10000004      # three 16-byte aligned addresses, one that is not
AUX = 0x40000000                                                  # W, the per-channel vectors, partial sums: never read either
NAMES = ['eap_narrow_conv_segments', 'eap_narrow_conv_stats_f32', 'eap_narrow_conv_bnact_fwd_f32', 'eap_narrow_conv_bwd_reduce_f32',
         'eap_narrow_conv_bwd_dw_f32']


def _lib():
    so = os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so')
    assert os.path.exists(so), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(so)
    lib.eap_last_error.restype = ctypes.c_char_p
    lib.eap_narrow_conv_segments.argtypes = [I64]
    lib.eap_narrow_conv_stats_f32.argtypes = [I, I, I, I64] + [P] * 6
    lib.eap_narrow_conv_bnact_fwd_f32.argtypes = [I, I, I, I64, F] + [P] * 6
    lib.eap_narrow_conv_bwd_reduce_f32.argtypes = [I, I, I, I64, F] + [P] * 10
    lib.eap_narrow_conv_bwd_dw_f32.argtypes = [I, I, I, I64, F] + [P] * 12
    return lib


def _aux(k):
    return [AUX + 4096 * i for i in range(k)]


# entry -> a call with (o, ck, n, x, gy / y) filled in; two clouds
ENTRIES = {
    'narrow_conv_stats': lambda lib, o, ck, n, x, t: lib.eap_narrow_conv_stats_f32(2, o, ck, n, AUX, x, *_aux(4)[1:], None),
    'narrow_conv_bnact_fwd': lambda lib, o, ck, n, x, t: lib.eap_narrow_conv_bnact_fwd_f32(2, o, ck, n, 0.01, AUX, x, AUX + 4096, AUX + 8192, t, None),
    'narrow_conv_bwd_reduce': lambda lib, o, ck, n, x, t: lib.eap_narrow_conv_bwd_reduce_f32(2, o, ck, n, 0.01, t, x, *_aux(7), None),
    'narrow_conv_bwd_dw': lambda lib, o, ck, n, x, t: lib.eap_narrow_conv_bwd_dw_f32(2, o, ck, n, 0.01, t, x, *_aux(9), None),
}
REFUSED = [
    ('contraction indices', 64, 33, 3840, X, GY),
    ('contraction indices', 64, 48, 3840, X, GY),
    ('contraction indices', 64, 0, 3840, X, GY),
    ('multiple of 32 output channels', 48, 24, 3840, X, GY),
    ('multiple of 32 output channels', 16, 24, 3840, X, GY),
    ('multiple of 4', 64, 24, 3842, X, GY),
    ('multiple of 4', 32, 30, 61, X, GY),
    ('16-byte aligned', 64, 24, 3840, ODD, GY),
    ('16-byte aligned', 64, 24, 3840, X + 8, GY),
    ('16-byte aligned', 64, 24, 3840, X, ODD),
    ('16-byte aligned', 32, 30, 3120, X, GY + 12),
]


def test_entries_are_declared_and_exported():
    text = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(eap_[a-z0-9_]+)\s*\(', text))
    lib = _lib()
    for name in NAMES:
        assert name in declared, f'{name} is not declared in include/eap_hip.h'
        assert hasattr(lib, name), f'{name} is not exported'
    assert lib.eap_abi_version() == 1


def test_segments():
    lib = _lib()
    assert lib.eap_narrow_conv_segments(0) == 0 and lib.eap_narrow_conv_segments(4) == 1
    assert lib.eap_narrow_conv_segments(2048) == 1 and lib.eap_narrow_conv_segments(2052) == 2
    assert lib.eap_narrow_conv_segments(4096 * 60) == 120


# (the statistics pass takes one tensor, x: the cases that misalign the other one are not its cases)
CASES = [(e,) + r for e in sorted(ENTRIES) for r in REFUSED if not (e == 'narrow_conv_stats' and r[4] == X and r[5] != GY)]


@pytest.mark.parametrize('entry, words, o, ck, n, x, t', CASES)
def test_refused_with_the_condition_in_the_message(entry, words, o, ck, n, x, t):
    lib = _lib()
    assert ENTRIES[entry](lib, o, ck, n, x, t) == INVALID_VALUE
    msg = lib.eap_last_error().decode()
    assert msg.startswith(entry + ':') and words in msg, msg


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_empty_batches_return_at_once(entry):
    lib = _lib()
    call = ENTRIES[entry]
    # (b = 2 is fixed in ENTRIES: an empty row length is the other empty shape)
    assert call(lib, 64, 24, 0, X, GY) == 0
