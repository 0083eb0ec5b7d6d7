"""CPU: the typed prototypes vgtk/_hip.py reads from include/eap_hip.h (`_hip.abi.<name>`), on host-only entries and on entries that
return before they launch anything (b = 0): every declared entry is bound with the arity and the return type of its declaration, 64-bit
values cross in both directions, and a call the prototype does not take is refused BEFORE the entry runs -- eap_last_error() keeps the
message an earlier call left.  `_hip.call` itself needs a device (tests/test_gpu_abi_binding.py); the count and the error translation it
relies on are `_hip._invoke`, which needs none."""
import ctypes
import glob
import importlib.util
import os
import re

import pytest
import torch

from test_abi_symbols import declared_symbols

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PKG = os.path.join(ROOT, 'equi-articulated-pose_amd')
INVALID_VALUE = 1           # hipErrorInvalidValue


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def _declarations():
    """name -> (return type, parameter count) read off the header with one expression per entry: not the package's parser"""
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eap_hip.h')).read(), flags=re.S)
    found = {}
    for name in declared_symbols():
        m = re.search(r'(const\s+char\s*\*|\bint64_t|\bint)\s*\b' + name + r'\s*\(([^)]*)\)\s*;', text)
        assert m, name
        params = m.group(2).strip()
        found[name] = (' '.join(m.group(1).split()), 0 if params == 'void' else params.count(',') + 1)
    return found


def test_every_declared_entry_has_its_prototype(hip):
    kinds = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char *': ctypes.c_char_p}
    decl = _declarations()
    assert len(decl) >= 152 and sorted(vars(hip.abi)) == sorted(decl)
    for name, (ret, count) in decl.items():
        fn = getattr(hip.abi, name)
        assert len(fn.argtypes) == count, name
        assert fn.restype is kinds[ret], name
    assert {r for r, _ in decl.values()} == set(kinds)
    assert hip.abi.eap_abi_version.restype is ctypes.c_int and hip.abi.eap_so3_dense_mask_words.restype is ctypes.c_int64 and \
        hip.abi.eap_last_error.restype is ctypes.c_char_p
    assert hip.abi.eap_abi_version() == 1


def test_the_library_handle_stays_untyped(hip):
    """tests and tools call `_hip.lib` with values they wrapped themselves: no argtypes there, and only the returns a C int would cut"""
    for name, (ret, _) in _declarations().items():
        fn = getattr(hip.lib, name)
        assert fn.argtypes is None, name
        assert fn.restype is {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char *': ctypes.c_char_p}[ret], name


def test_a_64_bit_parameter_arrives_whole(hip):
    assert hip.abi.eap_launch_dims_ok(2 ** 32 + 7, 1, 1, 256, 1, 1) == INVALID_VALUE
    assert '4294967303' in hip.abi.eap_last_error().decode()
    assert hip.abi.eap_launch_dims_ok(hip._I64(2 ** 32 + 9), 1, 1, 256, 1, 1) == INVALID_VALUE        # (a caller that still wraps)
    assert '4294967305' in hip.abi.eap_last_error().decode()


def test_a_64_bit_return_arrives_whole(hip):
    b, p, ks, rp = 512, 32768, 24, 1024
    # include/eap_hip.h, eap_so3_dense_mask_words, direction 1: [b][64-column wave tile][k-step of 32][64 lanes], one bit per weight of a
    # lane's k-step -- a 32-bit entry each, two to a uint64 word
    entries = b * (p // 64) * ((ks * rp + 31) // 32) * 64
    assert entries // 2 == 6442450944 > 2 ** 32
    assert hip.abi.eap_so3_dense_mask_words(b, p, ks, rp, 1) == entries // 2


def _marked(hip):
    """leave a known message in eap_last_error()"""
    assert hip.abi.eap_launch_dims_ok(2 ** 32 + 7, 1, 1, 256, 1, 1) == INVALID_VALUE
    msg = hip.abi.eap_last_error()
    assert b'4294967303' in msg
    return msg


def test_a_call_the_prototype_does_not_take_never_reaches_the_entry(hip):
    msg = _marked(hip)
    with pytest.raises(TypeError):                                  # one argument too few: ctypes itself
        hip.abi.eap_launch_dims_ok(1, 1, 1, 256, 1)
    assert hip.abi.eap_last_error() == msg
    for args in ((1, 1, 1, 256, 1), (1, 1, 1, 256, 1, 1, 1)):      # ... and the count `call` makes, which also sees one too many
        with pytest.raises(RuntimeError, match=r'eap_launch_dims_ok takes 6 arguments.* %d given' % len(args)):
            hip._invoke('eap_launch_dims_ok', args)
        assert hip.abi.eap_last_error() == msg
    with pytest.raises(ctypes.ArgumentError, match='argument 4'):   # a 64-bit instance for an `int`
        hip.abi.eap_launch_dims_ok(1, 1, 1, ctypes.c_int64(256), 1, 1)
    assert hip.abi.eap_last_error() == msg
    with pytest.raises(RuntimeError, match='eap_launch_dims_ok: argument 4'):
        hip._invoke('eap_launch_dims_ok', (1, 1, 1, ctypes.c_int64(256), 1, 1))
    with pytest.raises(ctypes.ArgumentError, match='argument 1'):   # ... and a float for an `int64_t`
        hip.abi.eap_launch_dims_ok(1.0, 1, 1, 256, 1, 1)
    assert hip.abi.eap_last_error() == msg
    assert hip._invoke('eap_launch_dims_ok', (1, 1, 1, 256, 1, 1)) == 0


def test_pointer_parameters_take_addresses_and_device_tensors_only(hip):
    """eap_bn_stats_f32(b, c, n, x, psum, psq, stream) with b = 0 returns before it touches a pointer"""
    for x in (1 << 40, ctypes.c_void_p(1 << 40), None, hip._ptr(None)):
        assert hip.abi.eap_bn_stats_f32(0, 1, 4, x, None, None, None) == 0
    msg = _marked(hip)
    host = torch.zeros(4, dtype=torch.float32)
    with pytest.raises(ctypes.ArgumentError, match='argument 4.*CUDA'):
        hip.abi.eap_bn_stats_f32(0, 1, 4, host, None, None, None)
    with pytest.raises(RuntimeError, match='eap_bn_stats_f32: argument 4.*CUDA'):
        hip._invoke('eap_bn_stats_f32', (0, 1, 4, host, None, None, None))
    with pytest.raises(RuntimeError, match='eap_bn_stats_f32: argument 4.*float64.*4-byte'):      # the width, whatever the device
        hip._invoke('eap_bn_stats_f32', (0, 1, 4, host.double(), None, None, None))
    with pytest.raises(RuntimeError, match='eap_bn_stats_f32: argument 5'):
        hip._invoke('eap_bn_stats_f32', (0, 1, 4, None, [0.0], None, None))
    assert hip.abi.eap_last_error() == msg
    # one class per pointee width; `void *` takes any
    widths = {n: t.width for n, t in zip(('b', 'm', 'l', 'na', 'seg', 'pitch', 'mapped', 'n_rows', 'rowmax', 'colmap', 'src', 'scale', 'planes'),
                                         hip.abi.eap_so3_dense_split_f32.argtypes) if hasattr(t, 'width')}
    assert widths == {'n_rows': 4, 'rowmax': 4, 'colmap': 4, 'src': 4, 'scale': 4, 'planes': 0}
    assert hip.abi.eap_so3_anchor_perm.argtypes[5].width == 1 and hip.abi.eap_so3_anchor_perm.argtypes[6].width == 8
    assert hip.abi.eap_ball_query_f64.argtypes[5].width == 8


@pytest.mark.parametrize('param', ['unsigned int n', 'size_t n', 'const int n', 'float **rows', 'double x', 'int32_t n', 'hipStream_t stream',
                                   'const float *const x'])
def test_a_type_outside_the_vocabulary_stops_the_import(hip, param):
    with pytest.raises(ImportError, match='eap_new_entry'):
        hip._argtype('eap_new_entry', param)


def test_a_missing_header_is_its_own_import_error(hip, tmp_path):
    """after the library check (tests/test_abi_symbols.py test_package_refuses_without_library), naming the path"""
    pkg = tmp_path / 'fake' / 'vgtk'
    pkg.mkdir(parents=True)
    (pkg / '_hip.py').write_text(open(os.path.join(PKG, 'vgtk', '_hip.py')).read())
    os.symlink(hip.LIB_PATH, tmp_path / 'fake' / 'libeap_hip.so')
    spec = importlib.util.spec_from_file_location('fake_hip_no_header', str(pkg / '_hip.py'))
    with pytest.raises(ImportError) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert str(tmp_path / 'include' / 'eap_hip.h') in str(e.value) and 'no CPU fallback' not in str(e.value)


def test_the_package_directory_brings_the_header_along(hip):
    """a copy of equi-articulated-pose_amd/ alone still imports (Option A): the package holds a link to the one header"""
    inside = os.path.join(PKG, 'include', 'eap_hip.h')
    assert os.path.samefile(inside, os.path.join(ROOT, 'include', 'eap_hip.h')) and hip.HEADER_PATH == inside


def test_the_package_wraps_no_argument_by_hand():
    """the types come from the header: the wrappers and `.restype` appear where vgtk/_hip.py defines them and nowhere else in the package"""
    files = sorted(glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True))
    assert len(files) >= 20
    text = {os.path.relpath(f, PKG): open(f).read() for f in files}
    count = lambda pattern: {f: len(re.findall(pattern, t)) for f, t in text.items() if re.search(pattern, t)}
    assert count(r'_I64\(') == {} and count(r'_F32\(') == {}
    assert count(r'\b_ptr\(') == {'vgtk/_hip.py': 1} and 'def _ptr(t):' in text['vgtk/_hip.py']
    assert count(r'\.restype') == {'vgtk/_hip.py': 1}
    assert count(r'\blib\.eap_') == {}
