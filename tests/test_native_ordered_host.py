"""CPU: the ordered (atomics-free) backwards of the point gather and the two native zpconv operators -- csrc/native_ordered.hip,
eap_{gather_points,intra_zpconv,inter_zpconv}_bwd_ordered_{f32,f64} and eap_inter_zpconv_bwd_ordered_workspace -- as far as they
go without a device: declared and exported with the header's arity, the shape checks every entry makes before its first launch,
the `ordered=` keyword of the three Python operators, and the policy helper that follows torch's contract where no ordered kernel
can serve a call (raise under torch.use_deterministic_algorithms(True), warn under warn_only=True, silent otherwise)."""
import contextlib
import ctypes
import inspect
import os
import re
import warnings

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HIP_ERROR_INVALID_VALUE = 1

# entry -> (scalar type, number of parameters with the stream)
ENTRIES = {
    'eap_gather_points_bwd_ordered_f32': ('float', 11), 'eap_gather_points_bwd_ordered_f64': ('double', 11),
    'eap_intra_zpconv_bwd_ordered_f32': ('float', 12), 'eap_intra_zpconv_bwd_ordered_f64': ('double', 12),
    'eap_inter_zpconv_bwd_ordered_f32': ('float', 13), 'eap_inter_zpconv_bwd_ordered_f64': ('double', 13),
}
WORKSPACES = {'eap_inter_zpconv_bwd_ordered_workspace': 6, 'eap_inv_lists_entries_workspace': 4}


def _declarations():
    text = open(os.path.join(ROOT, 'include', 'eap_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _params(text, ret, name):
    decl = re.search(r'\b' + ret + r'\s+' + name + r'\s*\(([^)]*)\)\s*;', text)
    assert decl, f'{name} is not declared in include/eap_hip.h'
    return [' '.join(p.split()) for p in decl.group(1).split(',')]


def test_entries_are_declared_and_exported_with_the_headers_arity():
    from vgtk import _hip
    text = _declarations()
    lib = ctypes.CDLL(os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so'))
    for name, (scalar, arity) in ENTRIES.items():
        params = _params(text, 'int', name)
        other = 'float' if scalar == 'double' else 'double'
        assert len(params) == arity and params[-1] == 'eap_stream_t stream', (name, params)
        assert any(p.startswith(f'const {scalar} *') for p in params) and not any(other in p for p in params), (name, params)
        assert params[-2 if 'inter' not in name else -3].startswith(f'{scalar} *'), (name, params)      # the gradient written, at the width
        assert hasattr(lib, name), f'{name} is not exported by libeap_hip.so'
        assert len(getattr(_hip.abi, name).argtypes) == arity, name
    for name, arity in WORKSPACES.items():
        params = _params(text, 'int64_t', name)
        assert len(params) == arity and all(p.startswith('int ') for p in params), (name, params)
        assert hasattr(lib, name), f'{name} is not exported by libeap_hip.so'
        assert len(getattr(_hip.abi, name).argtypes) == arity, name
    # each ordered zpconv entry takes the operand list of its scatter twin (the inter one plus its workspace)
    for width in ('f32', 'f64'):
        assert _params(text, 'int', f'eap_intra_zpconv_bwd_ordered_{width}') == _params(text, 'int', f'eap_intra_zpconv_bwd_{width}')
        got = _params(text, 'int', f'eap_inter_zpconv_bwd_ordered_{width}')
        assert got[:-2] + got[-1:] == _params(text, 'int', f'eap_inter_zpconv_bwd_{width}') and got[-2] == 'void *workspace'


def _gather(abi, width, b, c, n, m):
    return getattr(abi, 'eap_gather_points_bwd_ordered_' + width)(b, c, n, m, None, None, None, None, None, None, None)


def _intra(abi, width, b, np_, na_in, na_out, ks, ann, c):
    return getattr(abi, 'eap_intra_zpconv_bwd_ordered_' + width)(b, np_, na_in, na_out, ks, ann, c, None, None, None, None, None)


def _inter(abi, width, b, np_, nq, na, ks, ann, c):
    return getattr(abi, 'eap_inter_zpconv_bwd_ordered_' + width)(b, np_, nq, na, ks, ann, c, None, None, None, None, None, None)


@pytest.mark.parametrize('width', ['f32', 'f64'])
def test_empty_shapes_return_zero_before_any_launch(width):
    """no output element: nothing to do, whatever the other sizes (null operands, no device here)"""
    from vgtk._hip import abi
    for b, c, n in ((0, 3, 5), (2, 0, 5), (2, 3, 0)):
        assert _gather(abi, width, b, c, n, 7) == 0
    for b, c, np_, na_in in ((0, 3, 5, 7), (2, 0, 5, 7), (2, 3, 0, 7), (2, 3, 5, 0)):
        assert _intra(abi, width, b, np_, na_in, 5, 2, 3, c) == 0
    for b, c, nq, na in ((0, 3, 5, 4), (2, 0, 5, 4), (2, 3, 0, 4), (2, 3, 5, 0)):
        assert _inter(abi, width, b, 9, nq, na, 3, 5, c) == 0


@pytest.mark.parametrize('width', ['f32', 'f64'])
def test_more_than_16384_target_rows_is_an_argument_error(width):
    """the list builders' limit, refused on the host: no device is touched (there is none here)"""
    from vgtk._hip import abi
    for call in (lambda: _gather(abi, width, 2, 3, 16385, 7), lambda: _intra(abi, width, 2, 5, 16385, 5, 2, 3, 3),
                 lambda: _inter(abi, width, 2, 9, 16385, 4, 3, 5, 3)):
        assert call() == HIP_ERROR_INVALID_VALUE
        assert b'16384' in abi.eap_last_error()


def test_inter_workspace_is_the_index_copy_the_entry_list_and_the_list_builders_tables():
    from vgtk._hip import abi

    def up(x):
        return (x + 255) // 256 * 256

    for (b, np_, nq, na, ks, ann) in ((1, 1, 1, 1, 1, 1), (2, 9, 11, 4, 3, 5), (2, 8, 9, 60, 24, 64), (1, 1024, 1024, 60, 24, 64)):
        clouds, entries = b * na, b * na * np_ * ks * ann
        chunks = (np_ * ks * ann + 8191) // 8192                      # of the entry builder's counting sort
        assert abi.eap_inv_lists_entries_workspace(clouds, np_, nq, ks * ann) == up(4 * clouds * chunks * nq)
        assert abi.eap_inter_zpconv_bwd_ordered_workspace(b, np_, nq, na, ks, ann) == (2 * up(4 * entries) + 4 * up(4 * clouds * nq) + up(4 * clouds) +
                                                                                        up(4 * clouds * chunks * nq))


def test_the_chunked_entry_builder_checks_its_sizes_on_the_host():
    from vgtk._hip import abi
    text = _declarations()
    params = _params(text, 'int', 'eap_inv_lists_entries_ws')
    old = _params(text, 'int', 'eap_inv_lists_entries')
    assert params == old[:-1] + ['void *workspace', old[-1]] and len(abi.eap_inv_lists_entries_ws.argtypes) == len(params)
    for b, p, n, nn in ((0, 5, 7, 3), (2, 0, 7, 3), (2, 5, 0, 3), (2, 5, 7, 0)):
        assert abi.eap_inv_lists_entries_ws(b, p, n, nn, None, None, None, None, None, None) == 0
    assert abi.eap_inv_lists_entries_ws(2, 5, 16385, 3, None, None, None, None, None, None) == HIP_ERROR_INVALID_VALUE
    assert b'16384' in abi.eap_last_error()


def test_the_three_operators_accept_ordered():
    import vgtk.cuda.gathering as G
    import vgtk.cuda.zpconv as Z
    for fn in (G.gather_points_backward, Z.intra_zpconv_backward, Z.inter_zpconv_backward):
        p = inspect.signature(fn).parameters.get('ordered')
        assert p is not None and p.default is None, fn.__name__
    # the autograd wrappers pass nothing: they follow torch's flag through the default
    src = open(os.path.join(ROOT, 'equi-articulated-pose_amd', 'vgtk', 'spconv', 'functional.py')).read()
    assert 'ordered' not in src


@contextlib.contextmanager
def _flag(on, warn_only=False):
    """torch.use_deterministic_algorithms(on, warn_only=...) for the block; flag and warn_only come back afterwards"""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on, warn_only=warn_only)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.are_deterministic_algorithms_enabled() == was and torch.is_deterministic_algorithms_warn_only_enabled() == warn


def test_policy_raises_under_the_flag():
    from vgtk import _hip
    with _flag(True):
        with pytest.raises(RuntimeError, match='some_op does not have a deterministic implementation for this call') as err:
            _hip.no_deterministic('some_op', 'the reason')
    assert 'the reason' in str(err.value)


def test_policy_warns_under_warn_only():
    from vgtk import _hip
    with _flag(True, warn_only=True), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        _hip.no_deterministic('some_op', 'the reason')
    assert len(seen) == 1 and 'some_op does not have a deterministic implementation for this call' in str(seen[0].message)
    assert 'the reason' in str(seen[0].message)


def test_policy_is_silent_with_the_flag_off():
    from vgtk import _hip
    with _flag(False), warnings.catch_warnings():
        warnings.simplefilter('error')
        _hip.no_deterministic('some_op', 'the reason')
        # ... unless the caller itself asked for ordered=True: then there is nothing quiet to fall back to
        with pytest.raises(RuntimeError, match='some_op does not have a deterministic implementation'):
            _hip.no_deterministic('some_op', 'the reason', requested=True)


def test_ordered_keyword_follows_the_flag_only_when_none():
    from vgtk import _hip
    with _flag(False):
        assert (_hip.use_ordered(None), _hip.use_ordered(True), _hip.use_ordered(False)) == (False, True, False)
    with _flag(True, warn_only=True):
        assert (_hip.use_ordered(None), _hip.use_ordered(True), _hip.use_ordered(False)) == (True, True, False)


def test_the_order_check_of_the_gpu_test_has_teeth():
    """tests/test_gpu_native_ordered.py compares the kernels with a sequential NumPy evaluation bit for bit.  On its own random
    float32 operands, the same terms added in the REVERSE order, or with the product carried unrounded into the add, give other bits in
    some element of every operator: a kernel that summed that way would fail there."""
    import numpy as np
    import test_gpu_native_ordered as T
    idx, g = T.gather_case('n37', 'f32')[:2]
    want = T.gather_case('n37', 'f32')[3]['ordered']
    assert not np.array_equal(T.seq_gather(idx[:, ::-1], g[:, :, ::-1], 37), want)
    idx, w, g = T.intra_case('60x60', 'f32')[:3]
    want = T.intra_case('60x60', 'f32')[5]
    assert not np.array_equal(T.seq_intra(idx[::-1], w[::-1], g[..., ::-1], 60), want['ordered'])
    # (unrounded product: the float64 evaluation rounded to float32 at the end is not the float32 evaluation either)
    assert not np.array_equal(want['f64'].astype(np.float32), want['ordered'])
    idx, w, g = T.inter_case('irregular', 'f32')[:3]
    want = T.inter_case('irregular', 'f32')[5]
    assert not np.array_equal(T.seq_inter(idx[:, ::-1], w[:, ::-1], g[:, :, :, ::-1], 11), want['ordered'])
    assert not np.array_equal(want['f64'].astype(np.float32), want['ordered'])
