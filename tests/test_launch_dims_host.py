"""CPU: the limits every kernel launch is checked against (csrc/common.h launch_dims, reached through the host-only entry
eap_launch_dims_ok -- no kernel runs), and the one place a launch may be spelled."""
import ctypes
import glob
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CSRC = os.path.join(ROOT, 'equi-articulated-pose_amd', 'csrc')
INVALID_VALUE = 1           # hipErrorInvalidValue


def _lib():
    so = os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so')
    assert os.path.exists(so), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(so)
    lib.eap_launch_dims_ok.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int] * 3
    lib.eap_launch_dims_ok.restype = ctypes.c_int
    lib.eap_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize('grid, block', [
    ((1, 1, 1), (256, 1, 1)),
    ((2 ** 24 - 1, 1, 1), (256, 1, 1)),             # the most 256-thread blocks: (2^24 - 1) * 256 < 2^32
    ((2 ** 32 - 1, 1, 1), (1, 1, 1)),
    ((1, 65535, 65535), (64, 1, 1)),
])
def test_accepted(grid, block):
    assert _lib().eap_launch_dims_ok(*grid, *block) == 0


@pytest.mark.parametrize('grid, block', [
    ((2 ** 24, 1, 1), (256, 1, 1)),                 # 2^24 * 256 = 2^32 work items along x
    ((2 ** 31 - 1, 1, 1), (256, 1, 1)),             # the bound the entries used to check by hand
    ((2 ** 32 + 5, 1, 1), (256, 1, 1)),             # used to wrap to a grid of 5
    ((1, 65536, 1), (256, 1, 1)),
    ((1, 1, 65536), (256, 1, 1)),
    ((0, 1, 1), (256, 1, 1)),
    ((1, 0, 1), (256, 1, 1)),
    ((1, 1, -3), (256, 1, 1)),
    ((-7, 1, 1), (256, 1, 1)),
    ((1, 1, 1), (2048, 1, 1)),
    ((1, 1, 1), (32, 32, 2)),                       # 2048 threads over three dimensions
    ((1, 1, 1), (256, 0, 1)),
])
def test_refused_with_the_sizes_in_the_message(grid, block):
    lib = _lib()
    assert lib.eap_launch_dims_ok(*grid, *block) == INVALID_VALUE
    msg = lib.eap_last_error().decode()
    assert '(%d, %d, %d)' % grid in msg and '(%d, %d, %d)' % block in msg, msg
    assert '2^32' in msg and '65535' in msg and '1024' in msg, msg


def test_launches_are_spelled_in_common_h_only():
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert len(files) >= 30
    for path in files:
        text = open(path).read()
        found = [s for s in ('hipLaunchKernelGGL', '<<<', 'hipFuncSetAttribute') if s in text]
        if os.path.basename(path) == 'common.h':
            assert 'hipLaunchKernelGGL' in found and 'hipFuncSetAttribute' in found
        else:
            assert not found, f'{os.path.basename(path)} spells {found}: launches go through eap::run_kernel (csrc/common.h)'
