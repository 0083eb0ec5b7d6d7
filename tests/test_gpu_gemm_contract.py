"""GPU: every GEMM entry of the C ABI on padded, offset and strided operands (tests/gemm_contract.py): integer operands, so
every kernel owes the exact product; NaN in every padding, gap and guard of the inputs, one NaN bit pattern in C, the
residual's padding and the workspaces.  Three properties per call: nothing outside the logical elements of an input reaches a
result (0 x NaN would), the pitch is used where the pitch is meant, nothing outside [M, N] of an item of C is written.

Entries are called directly through _hip.call, so each kernel is known to run; a case asserts what a host function reveals
about the path it is meant to hit (the `_supported` predicates, the split count from the `*_workspace` entries, the tile template
from eap_last_kernel()).  The last group goes through the dispatchers of vgtk._hip.  Every case prints one line (entry | kernel |
variant | shape | seconds); EAP_GEMM_CONTRACT_LOG=<file> collects them (profiles/gemm_contract_cases.txt).

Shapes are the smallest that reach each code path.  The skinny kernel's shapes have an odd K, so their `tight` layout
(lda = K) is one the entry's contract refuses: those cases assert the refusal and run `padded` (and an odd ldc)."""
import ctypes
import time

import pytest
import torch

import gemm_contract as gc
from gemm_contract import Case

pytestmark = pytest.mark.gpu

TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
C_ODD = {'A': 'padded', 'B': 'padded', 'C': 'odd'}
B_ODD = {'A': 'padded', 'B': 'odd', 'C': 'odd'}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def I(v):
    return ctypes.c_int64(int(v))


def P(op):
    return ctypes.c_void_p(0 if op is None else op if isinstance(op, int) else op.ptr())


def T(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def launch(call, name, *args, check=True):
    """one entry on the case's buffers -> the kernel name it reported; timed, recorded, checked"""
    from vgtk import _hip
    _hip.lib.eap_last_kernel()                                # (clear)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _hip.call(name, call.C.buf, *args)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kernel = _hip.lib.eap_last_kernel().decode()
    gc.record(call, kernel, dt)
    if check:
        call.check()
    return kernel


def abc(call):
    A, B, C = call.A, call.B, call.C
    return A, B, C


def strides_of_a(batch):
    """shared A (strideA = 0) and one A per item, where there is more than one item"""
    return (True, False) if batch > 1 else (False,)


# ---- eap_gemm_f32 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ta,tb', TRANS)
@pytest.mark.parametrize('M,N,K,batch', [(7, 60, 5, 1), (37, 19, 17, 2), (130, 129, 50, 2), (260, 100, 33, 1)])
def test_gemm_f32(dev, M, N, K, batch, ta, tb):
    """the three block tiles (M <= 64, M < 256, M >= 256), a ragged k-tail; `odd` takes the non-VEC kernels, `padded` the VEC kernels
    (with a ragged width the last piece of a row falls back to masked scalar loads)"""
    for variant in gc.VARIANTS:
        for shared in strides_of_a(batch):
            call = Case('eap_gemm_f32', M, N, K, batch, ta, tb, variant, shared_a=shared).materialise(dev)
            A, B, C = abc(call)
            launch(call, 'eap_gemm_f32', ta, tb, M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), I(C.stride), batch)


@pytest.mark.parametrize('tb,M,N,K', [(0, 37, 52, 17), (1, 37, 19, 20)])
def test_gemm_f32_blocked_b(dev, tb, M, N, K):
    """eap_gemm_f32_xb / _reduce_xb: the blocked dimension (N without transB, K with it) a multiple of 4 but not of the tile"""
    from vgtk import _hip
    for variant in ('tight', 'padded'):
        for ta in (0, 1):
            call = Case('eap_gemm_f32_xb', M, N, K, 2, ta, tb, variant, b_blocked=True).materialise(dev)
            A, B, C = abc(call)
            launch(call, 'eap_gemm_f32_xb', ta, tb, M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.brows), I(B.stride), P(C), I(C.ld), I(C.stride), 2)
            call = Case('eap_gemm_f32_reduce_xb', M, N, K, 2, ta, tb, variant, b_blocked=True, reduce=True).materialise(dev)
            A, B, C = abc(call)
            ws = call.workspace(_hip.lib.eap_gemm_f32_reduce_workspace(M, N, K, 2))
            launch(call, 'eap_gemm_f32_reduce_xb', ta, tb, M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.brows), I(B.stride), P(C), I(C.ld), 2, T(ws))


@pytest.mark.parametrize('ta,tb', [(0, 1), (1, 0)])
@pytest.mark.parametrize('M,N,K,batch,splits', [(100, 40, 8201, 16, 64), (37, 19, 1043, 2, None)])
def test_gemm_f32_reduce(dev, M, N, K, batch, splits, ta, tb):
    """(100, 40, 8201, 16): 64 splits of 144 -- splits 57 .. 63 are empty (they owe a zero slab), split 56 is ragged, K is odd"""
    from vgtk import _hip
    words = _hip.lib.eap_gemm_f32_reduce_workspace(M, N, K, batch)
    if splits:
        assert words == M * N * batch * splits
    for variant in gc.VARIANTS:
        for shared in strides_of_a(batch):
            call = Case('eap_gemm_f32_reduce', M, N, K, batch, ta, tb, variant, shared_a=shared, reduce=True).materialise(dev)
            A, B, C = abc(call)
            ws = call.workspace(words)
            launch(call, 'eap_gemm_f32_reduce', ta, tb, M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), batch, T(ws))


# ---- eap_gemm_dma_f32 --------------------------------------------------------------------------------------------------------

def dma_supported(ta, tb, M, N, K, A, B):
    from vgtk import _hip
    return bool(_hip.lib.eap_gemm_dma_f32_supported(ta, tb, M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride)))


def run_dma(dev, M, N, K, batch, ta, tb, template, variants=('tight', 'padded', C_ODD)):
    from vgtk import _hip
    for variant in variants:
        for shared in strides_of_a(batch):
            call = Case('eap_gemm_dma_f32', M, N, K, batch, ta, tb, variant, shared_a=shared).materialise(dev)
            A, B, C = abc(call)
            args = (ta, tb, M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), I(C.stride), batch)
            if (ta and M % 4) or (not tb and N % 4):
                assert not dma_supported(ta, tb, M, N, K, A, B)
                with pytest.raises(RuntimeError):
                    _hip.call('eap_gemm_dma_f32', C.buf, *args)
                torch.cuda.synchronize()
                assert bool((C.buf.view(torch.int32) == gc.FILL_BITS).all())
                continue
            assert dma_supported(ta, tb, M, N, K, A, B)
            kernel = launch(call, 'eap_gemm_dma_f32', *args)
            assert kernel.startswith(f'gemm_dma_f32_kernel<{template}, {"true" if ta else "false"}, {"false" if tb else "true"}>'), kernel


@pytest.mark.parametrize('ta,tb', TRANS)
@pytest.mark.parametrize('M,N,K,batch,template', [
    (52, 520, 48, 2, '1, 4, 2, 4'),          # 64 x 512
    (520, 52, 48, 2, '4, 1, 4, 2'),          # 512 x 64
    (100, 260, 48, 2, '1, 4, 4, 2'),         # 128 x 256
    (260, 100, 48, 2, '4, 1, 2, 4'),         # 256 x 128
    (260, 516, 48, 2, '2, 2, 4, 4'),         # 256 x 256
    (50, 258, 48, 2, '1, 4, 2, 4'),          # M, N not multiples of 4: the row-contiguous forms are refused
])
def test_gemm_dma(dev, M, N, K, batch, template, ta, tb):
    """one shape per tile of launch_shape, three k-tiles (the ring's start-up with exactly STAGES tiles)"""
    run_dma(dev, M, N, K, batch, ta, tb, template)


@pytest.mark.parametrize('ta,tb', TRANS)
def test_gemm_dma_wide_tile(dev, ta, tb):
    """128 x 512: two column tiles x 512 items reach the `>= 1024` condition"""
    run_dma(dev, 100, 516, 16, 512, ta, tb, '1, 4, 4, 4', variants=('tight', 'padded'))


@pytest.mark.parametrize('K', [16, 32, 64, 80])
def test_gemm_dma_ring_start(dev, K):
    """the ring with 1, 2, 4 and 5 k-tiles on the 256 x 256 tile"""
    for ta, tb in TRANS:
        run_dma(dev, 260, 516, K, 2, ta, tb, '2, 2, 4, 4', variants=('padded',))


@pytest.mark.parametrize('ta,tb', [(0, 1), (1, 0)])
@pytest.mark.parametrize('M,N,K,batch,splits', [(128, 128, 8208, 16, 64), (100, 40, 2080, 3, None)])
def test_gemm_dma_reduce(dev, M, N, K, batch, splits, ta, tb):
    """(128, 128, 8208, 16): 64 splits of 144, seven of them empty (a zero slab each)"""
    from vgtk import _hip
    words = _hip.lib.eap_gemm_dma_f32_reduce_workspace(M, N, K, batch)
    if splits:
        assert words == M * N * batch * splits
    for variant in ('tight', 'padded', C_ODD):
        for shared in (False, True):
            call = Case('eap_gemm_dma_f32_reduce', M, N, K, batch, ta, tb, variant, shared_a=shared, reduce=True).materialise(dev)
            A, B, C = abc(call)
            assert dma_supported(ta, tb, M, N, K, A, B)
            ws = call.workspace(words)
            launch(call, 'eap_gemm_dma_f32_reduce', ta, tb, M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), batch, T(ws))


# ---- the split kernels -------------------------------------------------------------------------------------------------------

class presplit:
    """with presplit(v): eap_gemm_bf16x3_presplit(v), restored on exit"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from vgtk import _hip
        self.was = _hip.lib.eap_gemm_bf16x3_presplit(self.v)

    def __exit__(self, *exc):
        from vgtk import _hip
        _hip.lib.eap_gemm_bf16x3_presplit(self.was)


def split_supported(tb, M, N, K, A, B):
    from vgtk import _hip
    fn = _hip.lib.eap_gemm_bf16x3_f32_supported if tb else _hip.lib.eap_gemm_bf16x3_nn_f32_supported
    return bool(fn(M, N, K, P(A), I(A.ld), P(B), I(B.ld), I(B.stride)))


SPLIT_SHAPES = [(128, 384, 48, 3), (256, 256, 16, 1), (384, 768, 1040, 2)]


def split_name(kind, M, tb):
    return f'gemm_{kind}_kernel<{4 if M % 256 == 0 else 2}, 4{"" if tb else ", nn"}>'


@pytest.mark.parametrize('tb', [1, 0])
@pytest.mark.parametrize('M,N,K,batch', SPLIT_SHAPES)
def test_gemm_bf16x3(dev, M, N, K, batch, tb):
    """eap_gemm_bf16x3_f32 (tb = 1) / _nn_f32 (tb = 0): 128-row tiles with a last 128-column half-tile, a single k-tile, pre-split
    weights with lda > K; with the weights split once per call (2) and in the k-loop (0) -- bit-equal.  The row-major B may sit at any
    4-byte aligned base with any ldb >= N."""
    entry = 'eap_gemm_bf16x3_f32' if tb else 'eap_gemm_bf16x3_nn_f32'
    for variant in ('tight', 'padded', C_ODD) + (() if tb else (B_ODD,)):
        outs = []
        for pre in (2, 0):
            call = Case(entry, M, N, K, batch, 0, tb, variant, shared_a=True).materialise(dev)
            A, B, C = abc(call)
            assert split_supported(tb, M, N, K, A, B)
            with presplit(pre):
                kernel = launch(call, entry, M, N, K, P(A), I(A.ld), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), I(C.stride), batch)
            assert kernel == split_name('bf16x3', M, tb), kernel
            outs.append(C.buf.view(torch.int32))
        assert torch.equal(outs[0], outs[1])


def magnitudes(call, tb, grp):
    """abs_a, abs_b of eap_gemm_f16x2_f32 from eap_absmax_rows_f32 / eap_absmax_colgroups_f32 on the poisoned buffers (ld > cols): they
    must be those of the logical elements"""
    from vgtk import _hip
    A, B = call.A, call.B
    abs_a = torch.full((A.rows,), -1, dtype=torch.int32, device=call.device)
    _hip.call('eap_absmax_rows_f32', abs_a, P(A), 1, A.rows, A.cols, I(A.ld), I(0), T(abs_a))
    gc.check_absmax(abs_a, A, what='eap_absmax_rows_f32(A)')
    if tb:
        assert grp == 1
        abs_b = torch.full((B.nb, B.rows), -1, dtype=torch.int32, device=call.device)
        _hip.call('eap_absmax_rows_f32', abs_b, P(B), B.nb, B.rows, B.cols, I(B.ld), I(B.stride), T(abs_b))
        gc.check_absmax(abs_b, B, what='eap_absmax_rows_f32(B)')
    else:
        abs_b = torch.full((B.nb, B.cols // grp), -1, dtype=torch.int32, device=call.device)
        _hip.call('eap_absmax_colgroups_f32', abs_b, P(B), B.nb, B.rows, B.cols, I(B.ld), I(B.stride), grp, T(abs_b))
        gc.check_absmax(abs_b, B, grp=grp, what=f'eap_absmax_colgroups_f32(B, {grp})')
    return abs_a, abs_b


@pytest.mark.parametrize('tb', [1, 0])
@pytest.mark.parametrize('M,N,K,batch', SPLIT_SHAPES[:2])
def test_gemm_bf16x3_epilogue(dev, M, N, K, batch, tb):
    """eap_gemm_bf16x3_ep_f32: scale = +-2^j, integer shift, slope 1/4, integer residual at pitch ldc with its own item stride"""
    for variant in ('tight', 'padded', C_ODD) + (() if tb else (B_ODD,)):
        for ep in ('ep', 'res'):
            call = Case('eap_gemm_bf16x3_ep_f32', M, N, K, batch, 0, tb, variant, shared_a=True, epilogue=ep).materialise(dev)
            A, B, C = abc(call)
            assert split_supported(tb, M, N, K, A, B)
            R = call.R
            kernel = launch(call, 'eap_gemm_bf16x3_ep_f32', tb, M, N, K, P(A), I(A.ld), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), I(C.stride), batch,
                            T(call.scale), T(call.shift), ctypes.c_float(call.slope), P(R), I(R.stride if R else 0))
            assert kernel == split_name('bf16x3', M, tb), kernel


@pytest.mark.parametrize('tb', [1, 0])
@pytest.mark.parametrize('M,N,K,batch', SPLIT_SHAPES[:2])
def test_gemm_f16x2(dev, M, N, K, batch, tb):
    """eap_gemm_f16x2_f32 with and without the epilogue; abs_b per row of a k-contiguous B (grp_b = 1), per 4 columns of a row-major B, per
    12 columns where N = 384"""
    groups = (1,) if tb else (4, 12) if N % 12 == 0 else (4,)
    for variant in ('tight', 'padded', C_ODD):
        for grp in groups:
            for ep in (None, 'ep', 'res'):
                for pre in (1, 2) if ep is None else (1,):
                    call = Case('eap_gemm_f16x2_f32', M, N, K, batch, 0, tb, variant, shared_a=True, epilogue=ep).materialise(dev)
                    A, B, C = abc(call)
                    assert split_supported(tb, M, N, K, A, B)
                    abs_a, abs_b = magnitudes(call, tb, grp)
                    R = call.R
                    with presplit(pre):
                        kernel = launch(call, 'eap_gemm_f16x2_f32', tb, M, N, K, P(A), I(A.ld), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), I(C.stride),
                                        batch, T(abs_a), T(abs_b), grp, ctypes.c_float(1.0), T(call.scale), T(call.shift), ctypes.c_float(call.slope),
                                        P(R), I(R.stride if R else 0))
                    assert kernel == split_name('f16x2', M, tb), kernel


def test_gemm_f16x2_presplit_weights(dev):
    """the K >= 1024 path of the two-plane kernel (presplit_h_kernel) with lda > K"""
    M, N, K, batch = SPLIT_SHAPES[2]
    outs = []
    for pre in (1, 0):
        call = Case('eap_gemm_f16x2_f32', M, N, K, batch, 0, 1, 'padded', shared_a=True).materialise(dev)
        A, B, C = abc(call)
        abs_a, abs_b = magnitudes(call, 1, 1)
        with presplit(pre):
            launch(call, 'eap_gemm_f16x2_f32', 1, M, N, K, P(A), I(A.ld), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), I(C.stride), batch,
                   T(abs_a), T(abs_b), 1, ctypes.c_float(1.0), None, None, ctypes.c_float(0.0), None, I(0))
        outs.append(C.buf.view(torch.int32))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('M,N,K,batch,slabs', [(128, 256, 4096, 2, 4), (128, 256, 1024, 1, 1)])
def test_gemm_bf16x3_reduce(dev, M, N, K, batch, slabs):
    from vgtk import _hip
    words = _hip.lib.eap_gemm_bf16x3_reduce_workspace(M, N, K, batch)
    assert words == M * N * batch * slabs
    for variant in ('tight', 'padded'):
        for shared in strides_of_a(batch):
            call = Case('eap_gemm_bf16x3_reduce_f32', M, N, K, batch, 0, 1, variant, shared_a=shared, reduce=True).materialise(dev)
            A, B, C = abc(call)
            assert _hip.lib.eap_gemm_bf16x3_reduce_f32_supported(M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), I(C.ld))
            ws = call.workspace(words)
            kernel = launch(call, 'eap_gemm_bf16x3_reduce_f32', M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), batch, T(ws))
            assert kernel == 'gemm_bf16x3_kernel<2, 4>', kernel


# ---- eap_gemm_skinny_reduce_f32 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M,N,K,batch', [(40, 17, 4099, 2), (64, 32, 4223, 1), (7, 3, 5001, 2)])
def test_gemm_skinny_reduce(dev, M, N, K, batch):
    """odd contraction lengths: the scalar k-tail with one index left over; one and two row tiles"""
    from vgtk import _hip
    words = _hip.lib.eap_gemm_skinny_reduce_workspace(M, N, K, batch)
    for variant in ('tight', 'padded', C_ODD):
        for shared in strides_of_a(batch):
            call = Case('eap_gemm_skinny_reduce_f32', M, N, K, batch, 0, 1, variant, shared_a=shared, reduce=True).materialise(dev)
            A, B, C = abc(call)
            ok = bool(_hip.lib.eap_gemm_skinny_reduce_f32_supported(M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride)))
            args = (M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), P(C), I(C.ld), batch, T(call.workspace(words)))
            if variant == 'tight':                            # lda = K is odd: not made of 16-byte pieces
                assert not ok
                with pytest.raises(RuntimeError):
                    _hip.call('eap_gemm_skinny_reduce_f32', C.buf, *args)
                torch.cuda.synchronize()
                assert bool((C.buf.view(torch.int32) == gc.FILL_BITS).all())
                continue
            assert ok
            kernel = launch(call, 'eap_gemm_skinny_reduce_f32', *args)
            assert kernel == f'gemm_skinny_kernel<{2 if M > 32 else 1}>', kernel


# ---- the dispatchers ---------------------------------------------------------------------------------------------------------

def launched(fn):
    """-> (result of fn(), names of the C-ABI entries it launched)"""
    from vgtk import _hip
    rec = []
    _hip.KERNEL_TIMES = rec
    try:
        out = fn()
    finally:
        _hip.KERNEL_TIMES = None
    return out, [n for n, *_ in rec]


def accepts(entry, c, A, B, C):
    """does the predicate of the entry that ran accept these operands?"""
    from vgtk import _hip
    lib = _hip.lib
    dma = lambda: bool(lib.eap_gemm_dma_f32_supported(c.transA, c.transB, c.M, c.N, c.K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride)))
    if entry in ('eap_gemm_bf16x3_f32', 'eap_gemm_bf16x3_nn_f32', 'eap_gemm_bf16x3_ep_f32', 'eap_gemm_f16x2_f32'):
        return not c.transA and (A.stride == 0 or c.batch == 1) and split_supported(c.transB, c.M, c.N, c.K, A, B)
    if entry in ('eap_gemm_dma_f32', 'eap_gemm_dma_f32_reduce'):
        return dma()
    if entry == 'eap_gemm_bf16x3_reduce_f32':
        return (c.transA, c.transB) == (0, 1) and C.ptr() % 16 == 0 and \
            bool(lib.eap_gemm_bf16x3_reduce_f32_supported(c.M, c.N, c.K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), I(C.ld)))
    if entry == 'eap_gemm_skinny_reduce_f32':
        return (c.transA, c.transB) == (0, 1) and \
            bool(lib.eap_gemm_skinny_reduce_f32_supported(c.M, c.N, c.K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride)))
    return entry in ('eap_gemm_f32', 'eap_gemm_f32_reduce')       # take everything


def dispatch(call, fn):
    t0 = time.perf_counter()
    out, names = launched(fn)
    torch.cuda.synchronize()
    gemms = [n for n in names if 'gemm' in n]
    assert len(gemms) == 1, names
    gc.record(call, 'via dispatcher: ' + gemms[0], time.perf_counter() - t0)
    call.check()
    assert accepts(gemms[0], call.case, call.A, call.B, call.C), (gemms[0], call.case.variant_name())
    return out, gemms[0]


DISPATCHER_GEMM = [
    (128, 384, 48, 3, 0, 1, True, 'eap_gemm_bf16x3_f32'),
    (128, 384, 48, 3, 0, 0, True, 'eap_gemm_bf16x3_nn_f32'),
    (100, 260, 48, 2, 0, 1, False, 'eap_gemm_dma_f32'),
    (128, 384, 48, 3, 1, 0, False, 'eap_gemm_dma_f32'),
    (37, 19, 17, 2, 0, 0, False, 'eap_gemm_f32'),
]
DISPATCHER_GEMM_EPILOGUE = [(128, 384, 48, 3, 1, True), (256, 256, 16, 1, 0, True), (100, 260, 48, 2, 1, False)]
DISPATCHER_GEMM_REDUCE = [
    (128, 256, 1024, 1, 0, 1, 'eap_gemm_bf16x3_reduce_f32', 'eap_gemm_bf16x3_reduce_f32'),
    (40, 17, 4099, 2, 0, 1, 'eap_gemm_f32_reduce', 'eap_gemm_skinny_reduce_f32'),
    (100, 40, 2080, 3, 0, 1, 'eap_gemm_dma_f32_reduce', 'eap_gemm_dma_f32_reduce'),
    (100, 40, 2080, 3, 1, 0, 'eap_gemm_dma_f32_reduce', 'eap_gemm_dma_f32_reduce'),
    (37, 19, 1043, 2, 0, 1, 'eap_gemm_f32_reduce', 'eap_gemm_f32_reduce'),
]


@pytest.mark.parametrize('M,N,K,batch,ta,tb,shared,tight_entry', DISPATCHER_GEMM)
def test_dispatcher_gemm(dev, M, N, K, batch, ta, tb, shared, tight_entry):
    from vgtk import _hip
    for variant in gc.VARIANTS:
        call = Case('_hip.gemm', M, N, K, batch, ta, tb, variant, shared_a=shared).materialise(dev)
        A, B, C = abc(call)
        _, entry = dispatch(call, lambda: _hip.gemm(ta, tb, M, N, K, A.tensor(), A.ld, A.stride, B.tensor(), B.ld, B.stride, C.tensor(), C.ld, C.stride,
                                                    batch))
        if variant == 'tight':
            assert entry == tight_entry
        if variant == 'odd':
            assert entry == 'eap_gemm_f32'


@pytest.mark.parametrize('M,N,K,batch,tb,takes', DISPATCHER_GEMM_EPILOGUE)
def test_dispatcher_gemm_epilogue(dev, M, N, K, batch, tb, takes):
    """_hip.gemm_epilogue launches the split kernel where its predicate accepts the operands, and nothing at all where it does not
    (without a residual: the dispatcher passes one at C's item stride, the harness lays it out at its own)"""
    from vgtk import _hip
    for variant in gc.VARIANTS:
        call = Case('_hip.gemm_epilogue', M, N, K, batch, 0, tb, variant, shared_a=True, epilogue='ep').materialise(dev)
        A, B, C = abc(call)
        fn = lambda: _hip.gemm_epilogue(tb, M, N, K, A.tensor(), A.ld, B.tensor(), B.ld, B.stride, C.tensor(), C.ld, C.stride, batch,
                                        call.scale, call.shift, call.slope)
        out, names = launched(fn)
        torch.cuda.synchronize()
        assert out == (takes and variant != 'odd')            # (an odd lda is not made of 16-byte pieces)
        if out:
            gemms = [n for n in names if 'gemm' in n]
            assert len(gemms) == 1, names
            gc.record(call, 'via dispatcher: ' + gemms[0], 0.0)
            call.check()
            assert accepts(gemms[0], call.case, A, B, C)
        else:                                                 # nothing launched, nothing written
            assert not names and bool((C.buf.view(torch.int32) == gc.FILL_BITS).all())


@pytest.mark.parametrize('M,N,K,batch,ta,tb,tight_entry,padded_entry', DISPATCHER_GEMM_REDUCE)
def test_dispatcher_gemm_reduce(dev, M, N, K, batch, ta, tb, tight_entry, padded_entry):
    from vgtk import _hip
    for variant in gc.VARIANTS + (C_ODD,):
        for shared in strides_of_a(batch):
            call = Case('_hip.gemm_reduce', M, N, K, batch, ta, tb, variant, shared_a=shared, reduce=True).materialise(dev)
            A, B, C = abc(call)
            _, entry = dispatch(call, lambda: _hip.gemm_reduce(ta, tb, M, N, K, A.tensor(), A.ld, A.stride, B.tensor(), B.ld, B.stride, C.tensor(), C.ld,
                                                               batch))
            if variant == 'tight':
                assert entry == tight_entry
            if variant == 'padded':
                assert entry == padded_entry
            if variant == 'odd':
                assert entry == 'eap_gemm_f32_reduce'


def test_dispatcher_gemm_reduce_with_c_inside_its_storage(dev):
    """gemm_reduce(0, 1, 128, 256, 1024, ...) with C a view that starts 4 bytes into its storage: the split kernel's predicate never
    sees C, its entry refuses a C that is not 16-byte aligned -- the dispatcher has to fall through to a kernel that takes it"""
    from vgtk import _hip
    M, N, K = 128, 256, 1024
    for variant in ('tight', 'padded'):
        call = Case('_hip.gemm_reduce', M, N, K, 1, 0, 1, variant, reduce=True, c_base_extra=1).materialise(dev)
        A, B, C = abc(call)
        assert C.ptr() % 16 == 4 and C.ld % 4 == 0
        assert _hip.lib.eap_gemm_bf16x3_reduce_f32_supported(M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), I(C.ld))
        _, entry = dispatch(call, lambda: _hip.gemm_reduce(0, 1, M, N, K, A.tensor(), A.ld, A.stride, B.tensor(), B.ld, B.stride, C.tensor(), C.ld, 1))
        assert entry == 'eap_gemm_dma_f32_reduce'


# ---- the same through the view-based calls -----------------------------------------------------------------------------------

def views(call):
    """the case's operands as strided views over A.tensor(), B.tensor(), C.tensor(): what _hip.matmul* take (a shared A and the C of a
    reduction are 2-D; an operand stored transposed is the transpose of its stored matrix)"""
    c = call.case

    def view(op, trans, flat):
        t = op.tensor()
        v = torch.as_strided(t, (op.rows, op.cols), (op.ld, 1)) if flat else torch.as_strided(t, (op.nb, op.rows, op.cols), (op.item_stride, op.ld, 1))
        return v.transpose(-1, -2) if trans else v
    return view(call.A, c.transA, c.shared_a), view(call.B, c.transB, False), view(call.C, 0, c.reduce)


def positional_pick(case, dev, fn):
    """the entry the positional dispatcher launches for this case (fn(_hip, call): the positional call), on buffers of its own"""
    from vgtk import _hip
    call = case.materialise(dev)
    _, names = launched(lambda: fn(_hip, call))
    torch.cuda.synchronize()
    gemms = [n for n in names if 'gemm' in n]
    assert len(gemms) == 1, names
    return gemms[0]


def _gemm(_hip, call):
    c, (A, B, C) = call.case, abc(call)
    _hip.gemm(c.transA, c.transB, c.M, c.N, c.K, A.tensor(), A.ld, A.stride, B.tensor(), B.ld, B.stride, C.tensor(), C.ld, C.stride, c.batch)


def _gemm_reduce(_hip, call):
    c, (A, B, C) = call.case, abc(call)
    _hip.gemm_reduce(c.transA, c.transB, c.M, c.N, c.K, A.tensor(), A.ld, A.stride, B.tensor(), B.ld, B.stride, C.tensor(), C.ld, c.batch)


@pytest.mark.parametrize('M,N,K,batch,ta,tb,shared,tight_entry', DISPATCHER_GEMM)
def test_views_gemm(dev, M, N, K, batch, ta, tb, shared, tight_entry):
    """test_dispatcher_gemm through _hip.matmul: one entry, the one the positional call picks, the same contract"""
    from vgtk import _hip
    for variant in gc.VARIANTS:
        case = Case('_hip.matmul', M, N, K, batch, ta, tb, variant, shared_a=shared)
        call = case.materialise(dev)
        _, entry = dispatch(call, lambda: _hip.matmul(*views(call)))
        assert entry == positional_pick(case, dev, _gemm)
        if variant == 'tight':
            assert entry == tight_entry
        if variant == 'odd':
            assert entry == 'eap_gemm_f32'


@pytest.mark.parametrize('M,N,K,batch,tb,takes', DISPATCHER_GEMM_EPILOGUE)
def test_views_gemm_epilogue(dev, M, N, K, batch, tb, takes):
    """test_dispatcher_gemm_epilogue through _hip.matmul_epilogue: the split kernel where it takes the operands, else False and nothing launched"""
    from vgtk import _hip
    for variant in gc.VARIANTS:
        call = Case('_hip.matmul_epilogue', M, N, K, batch, 0, tb, variant, shared_a=True, epilogue='ep').materialise(dev)
        A, B, C = abc(call)
        out, names = launched(lambda: _hip.matmul_epilogue(*views(call), call.scale, call.shift, call.slope))
        torch.cuda.synchronize()
        assert out == (takes and variant != 'odd')
        if out:
            gemms = [n for n in names if 'gemm' in n]
            assert len(gemms) == 1, names
            gc.record(call, 'via dispatcher: ' + gemms[0], 0.0)
            call.check()
            assert accepts(gemms[0], call.case, A, B, C)
        else:
            assert not names and bool((C.buf.view(torch.int32) == gc.FILL_BITS).all())


@pytest.mark.parametrize('M,N,K,batch,ta,tb,tight_entry,padded_entry', DISPATCHER_GEMM_REDUCE)
def test_views_gemm_reduce(dev, M, N, K, batch, ta, tb, tight_entry, padded_entry):
    """test_dispatcher_gemm_reduce through _hip.matmul_reduce"""
    from vgtk import _hip
    for variant in gc.VARIANTS + (C_ODD,):
        for shared in strides_of_a(batch):
            case = Case('_hip.matmul_reduce', M, N, K, batch, ta, tb, variant, shared_a=shared, reduce=True)
            call = case.materialise(dev)
            _, entry = dispatch(call, lambda: _hip.matmul_reduce(*views(call)))
            assert entry == positional_pick(case, dev, _gemm_reduce)
            if variant == 'tight':
                assert entry == tight_entry
            if variant == 'padded':
                assert entry == padded_entry
            if variant == 'odd':
                assert entry == 'eap_gemm_f32_reduce'


def test_views_gemm_reduce_with_c_inside_its_storage(dev):
    """test_dispatcher_gemm_reduce_with_c_inside_its_storage through _hip.matmul_reduce; matmul_reduce_takes_split sees C and says no"""
    from vgtk import _hip
    M, N, K = 128, 256, 1024
    for variant in ('tight', 'padded'):
        call = Case('_hip.matmul_reduce', M, N, K, 1, 0, 1, variant, reduce=True, c_base_extra=1).materialise(dev)
        A, B, C = abc(call)
        assert C.ptr() % 16 == 4 and C.ld % 4 == 0
        assert _hip.lib.eap_gemm_bf16x3_reduce_f32_supported(M, N, K, P(A), I(A.ld), I(A.stride), P(B), I(B.ld), I(B.stride), I(C.ld))
        assert not _hip.matmul_reduce_takes_split(*views(call))
        _, entry = dispatch(call, lambda: _hip.matmul_reduce(*views(call)))
        assert entry == 'eap_gemm_dma_f32_reduce'


def test_views_refuse_before_anything_is_launched(dev):
    """host-side refusals: an input view that claims a column more than its storage holds, an out whose items overlap -- RuntimeError,
    no entry launched, C untouched"""
    from vgtk import _hip
    M, N, K, batch = 37, 19, 17, 2
    call = Case('_hip.matmul', M, N, K, batch, 0, 0, 'tight').materialise(dev)
    A, B, C = views(call)
    claims = torch.zeros(batch, K, N, dtype=torch.float32, device=dev)
    claims.untyped_storage().resize_(4 * (claims.numel() - 1))                     # the last column of its last row is gone
    overlapping = torch.as_strided(call.C.tensor(), (batch, M, N), (M * N - 1, N, 1))
    rec = []
    _hip.KERNEL_TIMES = rec
    try:
        for fn in (lambda: _hip.matmul(A, claims, C), lambda: _hip.matmul_reduce(A, claims, C[0]), lambda: _hip.matmul(A, B, overlapping),
                   lambda: _hip.matmul_epilogue(A[0], B, overlapping, call.A.buf[:M], call.A.buf[:M], 0.25)):
            with pytest.raises(RuntimeError):
                fn()
    finally:
        _hip.KERNEL_TIMES = None
    torch.cuda.synchronize()
    assert rec == [] and bool((call.C.buf.view(torch.int32) == gc.FILL_BITS).all())
