"""CPU: the argument checks of the four re-ordering entries of the dense product (csrc/so3_dense.hip eap_so3_dense_untranspose*):
rows of Y are moved as 16-byte pieces through a tile of at most 64 anchors, so na % 4 != 0, na > 64 and a yt or y that is not 16-byte
aligned are refused with hipErrorInvalidValue and a message that names the condition -- before any device call: the pointers here are
made-up addresses nothing may dereference, and on a machine without a GPU a device call would answer with its own error instead."""
import ctypes
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
INVALID_VALUE = 1           # hipErrorInvalidValue
P = ctypes.c_void_p
GOOD, GOOD2, ODD = 0x10000000, 0x20000000, 0x10000004      # two 16-byte aligned addresses, one that is not
AUX = 0x30000000                                          # map / pivot / partial sums / scale / shift: never read either


def _lib():
    so = os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so')
    assert os.path.exists(so), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(so)
    lib.eap_last_error.restype = ctypes.c_char_p
    i = ctypes.c_int
    lib.eap_so3_dense_untranspose_f32.argtypes = [i, i, i, i, P, P, P, P, P]
    lib.eap_so3_dense_untranspose_map_f32.argtypes = [i, i, i, i, i, P, P, P, P]
    lib.eap_so3_dense_untranspose_map_stats_f32.argtypes = [i, i, i, i, i, P, P, P, P, P, P, P]
    lib.eap_so3_dense_untranspose_bnact_f32.argtypes = [i, i, i, i, i, P, P, P, P, ctypes.c_float, P, P]
    return lib


# entry -> a call with (na, yt, y) filled in; b = 2, o = 3, p = 64, p_dst = 80
ENTRIES = {
    'so3_dense_untranspose': lambda lib, na, yt, y: lib.eap_so3_dense_untranspose_f32(2, 3, 64, na, yt, y, None, None, None),
    'so3_dense_untranspose_stats': lambda lib, na, yt, y: lib.eap_so3_dense_untranspose_f32(2, 3, 64, na, yt, y, AUX, AUX + 4096, None),
    'so3_dense_untranspose_map': lambda lib, na, yt, y: lib.eap_so3_dense_untranspose_map_f32(2, 3, 64, na, 80, AUX, yt, y, None),
    'so3_dense_untranspose_map_stats': lambda lib, na, yt, y: lib.eap_so3_dense_untranspose_map_stats_f32(2, 3, 64, na, 80, AUX, AUX + 4096, yt, y,
                                                                                                       AUX + 8192, AUX + 12288, None),
    'so3_dense_untranspose_bnact': lambda lib, na, yt, y: lib.eap_so3_dense_untranspose_bnact_f32(2, 3, 64, na, 80, AUX, yt, AUX + 4096, AUX + 8192, 0.2, y,
                                                                                               None),
    'so3_dense_untranspose_bnact_nomap': lambda lib, na, yt, y: lib.eap_so3_dense_untranspose_bnact_f32(2, 3, 64, na, 64, None, yt, AUX + 4096, AUX + 8192,
                                                                                                     0.2, y, None),
}
REFUSED = [
    ('na % 4', 6, GOOD, GOOD2),
    ('na % 4', 62, GOOD, GOOD2),
    ('na <= 64', 68, GOOD, GOOD2),
    ('na <= 64', 128, GOOD, GOOD2),
    ('yt 16-byte aligned', 60, ODD, GOOD2),
    ('yt 16-byte aligned', 60, GOOD + 8, GOOD2),
    ('y 16-byte aligned', 60, GOOD, ODD),
    ('y 16-byte aligned', 20, GOOD, GOOD2 + 12),
]


@pytest.mark.parametrize('entry', sorted(ENTRIES))
@pytest.mark.parametrize('names, na, yt, y', REFUSED)
def test_refused_with_the_condition_in_the_message(entry, names, na, yt, y):
    lib = _lib()
    assert ENTRIES[entry](lib, na, yt, y) == INVALID_VALUE
    msg = lib.eap_last_error().decode()
    # the entry's own name leads the message (the two forms that pass optional arguments share their entry's)
    name = entry.replace('_nomap', '').replace('untranspose_stats', 'untranspose')
    assert msg.startswith(name + ':') and names in msg, msg


def test_an_empty_batch_is_no_error():
    lib = _lib()
    assert lib.eap_so3_dense_untranspose_f32(0, 3, 64, 6, ODD, ODD, None, None, None) == 0
