"""CPU: the host-only entries of the dense product (csrc/so3_dense.hip) at the wide table width -- up to 1024 referenced rows per cloud,
32 membership words per point, a 64-bit group key.  No kernel runs: shape predicates, table sizes, exported symbols."""
import ctypes
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
WIDE = ('eap_so3_dense_max_rows', 'eap_so3_dense_member_wide', 'eap_so3_dense_point_keys_wide', 'eap_so3_dense_masks_wide',
        'eap_so3_dense_steps_wide')


def _lib():
    so = os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so')
    assert os.path.exists(so), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(so)
    lib.eap_so3_dense_mask_words.restype = ctypes.c_int64
    lib.eap_so3_dense_steps_words.restype = ctypes.c_int64
    return lib


def test_rows_up_to_1024_are_supported():
    lib = _lib()
    assert lib.eap_so3_dense_supported(4096, 60, 24, 768, 128) == 1
    assert lib.eap_so3_dense_supported(4096, 60, 24, 1024, 512) == 1
    assert lib.eap_so3_dense_supported(4096, 60, 24, 1040, 128) == 0          # over the cap
    assert lib.eap_so3_dense_supported(4096, 60, 24, 1040, 512) == 0
    assert lib.eap_so3_dense_supported(4096, 60, 24, 520, 128) == 0           # not whole groups of 16
    assert lib.eap_so3_dense_supported(4096, 60, 24, 520, 512) == 0
    # what was taken before still is
    assert lib.eap_so3_dense_supported(4096, 60, 24, 512, 128) == 1 and lib.eap_so3_dense_supported(512, 60, 24, 144, 256) == 1
    assert lib.eap_so3_dense_supported(4096, 60, 24, 768, 64) == 0 and lib.eap_so3_dense_supported(4090, 60, 24, 768, 128) == 0


def test_the_cap_is_read_from_the_library():
    lib = _lib()
    assert lib.eap_so3_dense_max_rows() == 1024
    from vgtk import _hip
    assert _hip.DENSE_MAX_ROWS == 1024 and _hip.DENSE_NARROW_ROWS == 512


def test_table_sizes_at_1024_rows_match_the_closed_forms():
    """eap_so3_dense_steps_words / eap_so3_dense_mask_words against the closed forms vgtk._hip.DenseGeometry.steps allocates by."""
    lib = _lib()
    for (b, p, ks, rp) in ((8, 4096, 24, 1024), (2, 2048, 24, 1024), (2, 4096, 24, 1008), (3, 1024, 24, 544), (8, 8192, 24, 784)):
        for direction in (0, 1):
            kd = (ks * rp + 31) // 32 * 32
            blocks_n = ((p if direction else ks * rp) + 255) // 256
            k_steps = (kd if direction else p) // 32
            assert lib.eap_so3_dense_steps_words(b, p, ks, rp, direction) == b * blocks_n * (k_steps + 1), (b, p, ks, rp, direction)
            # one 32-bit word per lane, k-step and 64-column wave tile, counted in 64-bit words
            assert lib.eap_so3_dense_mask_words(b, p, ks, rp, direction) == (b * 4 * blocks_n * k_steps * 64 + 1) // 2, (b, p, ks, rp, direction)
    # the forward's contraction axis at the cap: 768 k-steps (the k-step list behind the operand ring holds 1024)
    assert lib.eap_so3_dense_steps_words(1, 256, 24, 1024, 1) == 768 + 1


def test_wide_entries_are_exported_and_declared():
    lib = _lib()
    text = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in WIDE:
        assert hasattr(lib, name), name
        assert re.search(r'\b' + name + r'\s*\(', code), f'{name} is not declared in include/eap_hip.h'
    # the header states layout and limits of the wide tables
    assert 'memb uint32 [b,p,32]' in text and 'keys int64 [b,p]' in text and 'rp <= 1024' in text
