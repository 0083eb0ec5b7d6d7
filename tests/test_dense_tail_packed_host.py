"""CPU: the packed gradient tail of the dense layers (eap_so3_dense_product_packed_f32 and what consumes packed Z).  The packing index math
against a numpy restatement, the live column counts at the edges of a 16-row group, the new entries declared in include/eap_hip.h, exported
and bound with their arities, and every host-side refusal -- hipErrorInvalidValue and a message that starts with the entry's name, before
any device call.  The pointers are made-up addresses nothing may dereference."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
INVALID_VALUE = 1           # hipErrorInvalidValue
A = [0x10000000 + 0x100000 * i for i in range(16)]      # 16-byte aligned addresses, never read
ARITY = {'eap_so3_dense_product_packed_f32': 17, 'eap_so3_dense_live16': 2, 'eap_so3_dense_zbound_packed_f32': 12, 'eap_rows_gather_packed_f32': 12,
         'eap_rows_scatter_packed_f32': 13, 'eap_gemm_bf16x3_reduce_tail_f32': 15, 'eap_gemm_f16x2_splitk_tail_f32': 21}
NA = 60


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def test_entries_are_declared_exported_and_bound(hip):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eap_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(eap_[a-z0-9_]+)\s*\(', text))
    for name, arity in ARITY.items():
        assert name in declared, f'{name} is not declared in include/eap_hip.h'
        assert hasattr(hip.lib, name), f'{name} is not exported'
        assert hasattr(hip.abi, name), f'{name} is not bound'
        assert len(getattr(hip.abi, name).argtypes) == arity, name
    # the entries whose layout and zero fill stay: same arities as before
    assert len(hip.abi.eap_so3_dense_product_steps_f32.argtypes) == 18 and len(hip.abi.eap_so3_dense_product_f32.argtypes) == 17
    assert len(hip.abi.eap_gemm_f16x2_splitk_f32.argtypes) == 20 and len(hip.abi.eap_gemm_bf16x3_reduce_f32.argtypes) == 14
    assert len(hip.abi.eap_so3_dense_zbound_f32.argtypes) == 11 and len(hip.abi.eap_rows_gather_f32.argtypes) == 10


@pytest.mark.parametrize('rp', [16, 64, 144, 1024])
def test_live_rows_and_columns_at_the_edges_of_a_group(hip, rp):
    """live16 = ceil16(min(n_rows, rp)) and ncols = na * live16 for n_rows of 0, 1, 15, 16, 17, rp - 1, rp and more than rp"""
    for n, want in ((0, 0), (1, 16), (15, 16), (16, 16), (17, min(32, rp)), (rp - 1, rp), (rp, rp), (rp + 1, rp), (3 * rp + 5, rp)):
        assert hip.dense_live16(n, rp) == want, (n, rp)
        assert NA * hip.dense_live16(n, rp) == NA * min(-(-min(n, rp) // 16) * 16, rp)
        assert hip.dense_live16(n, rp) % 16 == 0 and (NA * hip.dense_live16(n, rp)) % 16 == 0       # whole bound words, whole k-tiles


def test_packing_index_math_against_numpy(hip):
    """column (a, r) of cloud i at a * live16[i] + r: the live columns of every cloud are exactly the prefix 0 .. na * live16[i] - 1 of its
    row, in the order of the zero-filled layout's live columns (a * rp + r with r < live16[i])"""
    rp = 96
    n_rows = np.array([96, 80, 37, 1, 200, 17])
    live = np.minimum((np.minimum(n_rows, rp) + 15) // 16 * 16, rp)
    for i, (n, lv) in enumerate(zip(n_rows, live)):
        a, r = np.meshgrid(np.arange(NA), np.arange(lv), indexing='ij')
        packed = np.array([[hip.dense_packed_column(x, y, int(n), rp) for y in range(lv)] for x in range(NA)])
        assert np.array_equal(packed, a * lv + r)
        assert np.array_equal(np.sort(packed.ravel()), np.arange(NA * lv))                      # one prefix, no hole, no overlap
        unpacked = (a * rp + r).ravel()
        assert np.array_equal(np.argsort(unpacked, kind='stable'), np.argsort(packed.ravel(), kind='stable'))     # the same order
        assert packed.max() < hip.dense_pitch(NA * rp)
    assert hip.dense_pitch(NA * rp) % 128 == 0


def test_the_layer_predicate(hip):
    """both tail products on the split kernels: 128 input channels; the 64-channel layer keeps the zero-filled layout"""
    assert hip.dense_tail_packed_takes(128, 512 * 24, NA * 144, hip.dense_pitch(NA * 144))
    assert hip.dense_tail_packed_takes(128, 128 * 24, NA * 16, hip.dense_pitch(NA * 16))
    assert not hip.dense_tail_packed_takes(64, 128 * 24, NA * 144, hip.dense_pitch(NA * 144))
    assert not hip.dense_tail_packed_takes(256, 512 * 24, NA * 144, hip.dense_pitch(NA * 144))
    assert not hip.dense_tail_packed_takes(128, 512 * 24, NA * 144, NA * 144 + 2)


def _product(hip, b=2, o=128, p=64, na=NA, ks=24, rp=16, ldz=1024, ptr=None):
    q = list(A[:8]) if ptr is None else ptr
    return hip.abi.eap_so3_dense_product_packed_f32(b, o, p, na, ks, rp, ldz, 0.5, *q, None)


def _zbound(hip, b=2, na=NA, rp=16, p=64, ldz=1024, stride=64, ptr=None):
    q = list(A[:5]) if ptr is None else ptr
    return hip.abi.eap_so3_dense_zbound_packed_f32(b, na, rp, p, ldz, stride, *q, None)


def _gather(hip, b=2, c=8, n=100, na=NA, rp=16, rows_ld=100, ld=1024, ptr=None):
    q = list(A[:4]) if ptr is None else ptr
    return hip.abi.eap_rows_gather_packed_f32(b, c, n, na, rp, rows_ld, ld, *q, None)


def _scatter(hip, b=2, c=8, c_ld=8, n=100, na=NA, rp=16, rows_ld=100, ld=1024, ptr=None):
    q = list(A[:4]) if ptr is None else ptr
    return hip.abi.eap_rows_scatter_packed_f32(b, c, c_ld, n, na, rp, rows_ld, ld, *q, None)


def _reduce(hip, M=128, N=256, K=1024, lda=1024, sa=128 * 1024, ldb=1024, sb=256 * 1024, ldc=256, batch=2, a=A[0], bm=A[1], c=A[2], ncols=A[3], ws=A[4]):
    return hip.abi.eap_gemm_bf16x3_reduce_tail_f32(M, N, K, a, lda, sa, bm, ldb, sb, c, ldc, batch, ncols, ws, None)


def _splitk(hip, M=128, N=256, K=2048, lda=2048, ldb=256, sb=2048 * 256, ldc=256, sc=128 * 256, batch=2, a=A[0], bm=A[1], c=A[2], abs_a=A[3], abs_b=A[4],
            grp=4, mult=1.0, slabs=2, ws=A[5], floats=128 * 256 * 2 * 2, ncols=A[6]):
    return hip.abi.eap_gemm_f16x2_splitk_tail_f32(M, N, K, a, lda, bm, ldb, sb, c, ldc, sc, batch, abs_a, abs_b, grp, mult, slabs, ws, floats, ncols, None)


def _nulled(k, i):
    return [None if j == i else a for j, a in enumerate(A[:k])]


REFUSED = [
    # (entry prefix of the message, words in it, call)
    ('so3_dense_product_packed', 'n_rows is required', lambda h: _product(h, ptr=_nulled(8, 0))),
    ('so3_dense_product', 'shape not taken', lambda h: _product(h, p=33)),
    ('so3_dense_product', 'shape not taken', lambda h: _product(h, rp=24)),
    ('so3_dense_product', 'shape not taken', lambda h: _product(h, o=96)),
    ('so3_dense_product', 'ldz < na rp', lambda h: _product(h, ldz=NA * 16 - 4)),
    *[('so3_dense_zbound_packed', 'null pointer', lambda h, i=i: _zbound(h, ptr=_nulled(5, i))) for i in range(5)],
    *[('so3_dense_zbound_packed', 'positive', lambda h, k=k: _zbound(h, **{k: 0})) for k in ('b', 'na', 'rp', 'p', 'ldz')],
    ('so3_dense_zbound_packed', 'multiple of 16', lambda h: _zbound(h, rp=20, ldz=2048)),
    ('so3_dense_zbound_packed', 'multiple of 4', lambda h: _zbound(h, ldz=1022)),
    ('so3_dense_zbound_packed', 'ldz >= na * rp', lambda h: _zbound(h, ldz=956)),
    ('so3_dense_zbound_packed', 'row stride', lambda h: _zbound(h, stride=12)),
    ('so3_dense_zbound_packed', 'outside the launch limits', lambda h: _zbound(h, b=65536)),
    *[('rows_gather_packed', 'null pointer', lambda h, i=i: _gather(h, ptr=_nulled(4, i))) for i in range(4)],
    *[('rows_gather_packed', 'positive', lambda h, k=k: _gather(h, **{k: 0})) for k in ('b', 'c', 'n', 'na', 'rp')],
    ('rows_gather_packed', 'multiple of 16', lambda h: _gather(h, rp=12)),
    ('rows_gather_packed', 'row stride', lambda h: _gather(h, rows_ld=8)),
    ('rows_gather_packed', 'ld >= na * rp', lambda h: _gather(h, ld=NA * 16 - 1)),
    ('rows_gather_packed', 'na <= 64', lambda h: _gather(h, na=68, ld=2048)),
    ('rows_gather_packed', 'outside the launch limits', lambda h: _gather(h, b=65536)),
    *[('rows_scatter_packed', 'null pointer', lambda h, i=i: _scatter(h, ptr=_nulled(4, i))) for i in range(4)],
    *[('rows_scatter_packed', 'positive', lambda h, k=k: _scatter(h, **{k: 0})) for k in ('b', 'c', 'n', 'na', 'rp')],
    ('rows_scatter_packed', 'multiple of 16', lambda h: _scatter(h, rp=12)),
    ('rows_scatter_packed', 'row stride', lambda h: _scatter(h, rows_ld=8)),
    ('rows_scatter_packed', 'ld >= na * rp', lambda h: _scatter(h, ld=NA * 16 - 1)),
    ('rows_scatter_packed', 'na <= 64', lambda h: _scatter(h, na=68, ld=2048)),
    ('rows_scatter_packed', 'c_ld >= c', lambda h: _scatter(h, c_ld=4)),
    *[('gemm_bf16x3_reduce_tail_f32', 'must be positive', lambda h, k=k: _reduce(h, **{k: 0})) for k in ('M', 'N', 'batch')],
    *[('gemm_bf16x3_reduce_tail_f32', 'are required', lambda h, k=k: _reduce(h, **{k: None})) for k in ('a', 'bm', 'c', 'ncols', 'ws')],
    ('gemm_bf16x3_reduce_tail_f32', 'unsupported operands', lambda h: _reduce(h, K=1000)),
    ('gemm_bf16x3_reduce_tail_f32', 'unsupported operands', lambda h: _reduce(h, M=64)),
    ('gemm_bf16x3_reduce_tail_f32', 'unsupported operands', lambda h: _reduce(h, lda=1026)),
    ('gemm_bf16x3_reduce_tail_f32', 'unsupported operands', lambda h: _reduce(h, c=A[2] + 4)),
    ('gemm_bf16x3_reduce_tail_f32', 'unsupported operands', lambda h: _reduce(h, a=A[0] + 8)),
    ('gemm_bf16x3_reduce_tail_f32', '65535', lambda h: _reduce(h, batch=65536)),
    *[('gemm_f16x2_splitk_tail_f32', 'must be positive', lambda h, k=k: _splitk(h, **{k: 0})) for k in ('M', 'N', 'batch')],
    *[('gemm_f16x2_splitk_tail_f32', 'are required', lambda h, k=k: _splitk(h, **{k: None})) for k in ('a', 'bm', 'c', 'ncols')],
    *[('gemm_f16x2_splitk_tail_f32', 'operand magnitudes', lambda h, k=k: _splitk(h, **{k: None})) for k in ('abs_a', 'abs_b')],
    ('gemm_f16x2_splitk_tail_f32', 'operand magnitudes', lambda h: _splitk(h, mult=0.0)),
    ('gemm_f16x2_splitk_tail_f32', 'operand magnitudes', lambda h: _splitk(h, grp=3)),
    ('gemm_f16x2_splitk_tail_f32', 'one 128-row tile', lambda h: _splitk(h, M=256)),
    ('gemm_f16x2_splitk_tail_f32', 'one 128-row tile', lambda h: _splitk(h, K=2040)),
    ('gemm_f16x2_splitk_tail_f32', 'slab count', lambda h: _splitk(h, slabs=3)),
    ('gemm_f16x2_splitk_tail_f32', 'slab count', lambda h: _splitk(h, slabs=16)),
    ('gemm_f16x2_splitk_tail_f32', '65535', lambda h: _splitk(h, batch=40000)),
    ('gemm_f16x2_splitk_tail_f32', 'strideC = M ldc', lambda h: _splitk(h, sc=128 * 256 + 4)),
    ('gemm_f16x2_splitk_tail_f32', 'strideC = M ldc', lambda h: _splitk(h, c=A[2] + 4)),
    ('gemm_f16x2_splitk_tail_f32', 'workspace is too small', lambda h: _splitk(h, floats=100)),
    ('gemm_f16x2_splitk_tail_f32', 'workspace is too small', lambda h: _splitk(h, ws=None)),
]


@pytest.mark.parametrize('case', range(len(REFUSED)))
def test_refused_before_any_device_call(hip, case):
    entry, words, call = REFUSED[case]
    assert call(hip) == INVALID_VALUE
    msg = hip.abi.eap_last_error().decode()
    assert msg.startswith(entry) and words in msg, msg


def test_python_side_refusals(hip):
    """the wrappers name what they were not given, before anything is launched"""
    import torch
    rows, n_rows = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='tensor must be a CUDA'):
        hip.rows_gather_packed(torch.zeros(2, 4, 8, 60), rows.int(), n_rows, 16, 1024)
    with pytest.raises(RuntimeError, match='rows and n_rows must be int32'):
        hip._packed_rows_args(rows, n_rows, 'rows_gather_packed')
    with pytest.raises(RuntimeError, match='rows and n_rows must be int32'):
        hip._packed_rows_args(rows.int(), n_rows.long(), 'rows_scatter_packed')
    with pytest.raises(RuntimeError, match='cnt and n_rows must be int32'):
        hip.so3_dense_zbound_packed(torch.zeros(2, 60), rows, n_rows, 16, 64, 1024)
    A_, B_, out = torch.zeros(128, 64), torch.zeros(2, 64, 256), torch.zeros(2, 128, 256)
    assert not hip.matmul_tail_takes(A_, B_, out, None)                       # no bound on the columns: not the two-plane kernel
    with pytest.raises(RuntimeError, match='matmul_tail: the operands do not qualify'):
        hip.matmul_tail(A_, B_, out, torch.zeros(2, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match='matmul_reduce_tail: the operands do not qualify'):
        hip.matmul_reduce_tail(torch.zeros(2, 64, 100), torch.zeros(2, 100, 256), torch.zeros(64, 256), torch.zeros(2, dtype=torch.int32))
