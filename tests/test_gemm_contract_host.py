"""CPU: (1) the GEMM contract harness (tests/gemm_contract.py) against entries emulated in torch that take the same
(base buffer, offset, pitch, stride) description as the HIP entries -- a correct one passes under every layout variant, each
planted fault is caught (the evidence that tests/test_gpu_gemm_contract.py can fail); (2) the `_supported` predicates of the
built library: the accepted baseline, every single violation, the accepted boundary values (host-only entries: the pointers
are made-up addresses, never dereferenced); (3) the split counts the GPU cases rely on, read from the `*_workspace` entries."""
import ctypes
import os

import pytest
import torch

import gemm_contract as gc
from gemm_contract import Case, ContractViolation

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CPU = torch.device('cpu')


# ---- entries emulated in torch ---------------------------------------------------------------------------------------------

def mat(op, z, rows, cols, ld=None, off=None, stride=None):
    """item z of an operand as the entry addresses it: base + z * stride + r * ld + c"""
    return torch.as_strided(op.buf, (rows, cols), (op.ld if ld is None else ld, 1),
                            (op.off if off is None else off) + z * (op.stride if stride is None else stride))


def emulated_gemm(call, fault=None):
    """C_z = op(A_z) op(B_z) (or their sum over z), optional row epilogue, in float64 from the described buffers."""
    c = call.case
    A, B, C = call.A, call.B, call.C
    total = None
    for z in range(c.batch):
        ra, ca = (c.K, c.M) if c.transA else (c.M, c.K)
        kw = {}
        if fault == 'base_ignored':
            kw['off'] = gc.GUARD
        if fault == 'shared_a_strided':
            kw['stride'] = A.item_stride
        a = mat(A, z, ra, ca, **kw)
        a = (a.t() if c.transA else a).double()
        if c.b_blocked:
            b = B.logical()[z].double()
            b = b.t() if c.transB else b
        else:
            rb, cb = (c.N, c.K) if c.transB else (c.K, c.N)
            b = mat(B, z, rb, cb, ld=cb if fault == 'ldb_is_width' else None)
            b = (b.t() if c.transB else b).double()
        if fault == 'k_term_dropped':
            a, b = a[:, :-1], b[:-1]
        if fault == 'ktail_times_zero':           # the k-tile's tail comes from A's padding and meets zeros on the B side
            assert not c.transA and A.ld > c.K
            a = mat(A, z, c.M, A.ld).double()
            b = torch.cat([b, torch.zeros(A.ld - c.K, c.N, dtype=torch.float64)])
        p = a @ b
        if c.reduce:
            total = p if total is None else total + p
            continue
        if c.epilogue:
            p = p * call.scale.double()[:, None] + call.shift.double()[:, None]
            p = torch.where(p >= 0, p, p * call.slope)
            if call.R is not None:
                p = p + mat(call.R, z, c.M, c.N).double()
        mat(C, z, c.M, c.N).copy_(p.float())
    if c.reduce:
        mat(C, 0, c.M, c.N).copy_(total.float())
    last = C.off + (C.nb - 1) * C.item_stride
    if fault == 'col_past_n':
        C.buf[C.off + c.N] = 1.0
    if fault == 'row_after_m':
        C.buf[last + c.M * C.ld] = 1.0
    if fault == 'item_gap':
        C.buf[C.off + C.item_stride - 1] = 1.0


def emulated_absmax_rows(op, over_pitch=False):
    cols = op.ld if over_pitch else op.cols
    v = torch.as_strided(op.buf, (op.nb, op.rows, cols), (op.item_stride, op.ld, 1), op.off)
    return v.abs().amax(2).contiguous().view(torch.int32)


def run(fault=None, **kw):
    case = Case('emulated', kw.pop('M', 7), kw.pop('N', 10), kw.pop('K', 5), kw.pop('batch', 2), **kw)
    call = case.materialise(CPU)
    emulated_gemm(call, fault)
    call.check()


@pytest.mark.parametrize('variant', gc.VARIANTS)
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_correct_emulation_passes(variant, ta, tb):
    for shared in (False, True):
        run(variants=variant, transA=ta, transB=tb, shared_a=shared)
        run(variants=variant, transA=ta, transB=tb, shared_a=shared, reduce=True)
        run(variants=variant, transA=ta, transB=tb, shared_a=shared, epilogue='ep')
        run(variants=variant, transA=ta, transB=tb, shared_a=shared, epilogue='res')
    if variant != 'odd':
        run(variants=variant, transA=ta, transB=tb, b_blocked=True, N=12, K=8)


def test_layouts_are_what_the_table_says():
    call = Case('emulated', 8, 12, 16, 2, variants='padded').materialise(CPU)
    assert (call.A.ld, call.B.ld, call.C.ld) == (16 + 4, 12 + 8, 12 + 12)
    assert (call.A.stride, call.A.off) == (8 * 20 + 20, gc.GUARD + 12) and call.C.stride == 8 * 24 + 20
    call = Case('emulated', 8, 12, 16, 2, variants='odd', shared_a=True).materialise(CPU)
    assert (call.A.ld, call.B.ld, call.C.ld) == (17, 15, 17) and call.A.stride == 0 and call.A.nb == 1
    assert call.B.stride % 2 == 1 and call.C.stride % 2 == 1 and call.B.off == gc.GUARD + 1
    call = Case('emulated', 8, 12, 16, 2).materialise(CPU)
    assert (call.A.ld, call.A.stride, call.A.off, call.C.ld, call.C.stride) == (16, 128, gc.GUARD, 12, 96)
    # everything outside the logical elements of an input is NaN, C holds the fill pattern
    call = Case('emulated', 8, 12, 16, 2, variants='padded', epilogue='res').materialise(CPU)
    for op in (call.A, call.B):
        assert int(torch.isnan(op.buf).sum()) == op.buf.numel() - op.view().numel() and not torch.isnan(op.view()).any()
    assert bool((call.C.buf.view(torch.int32) == gc.FILL_BITS).all())
    assert call.R.ld == call.C.ld and call.R.stride != call.C.stride
    assert int((call.R.buf.view(torch.int32) == gc.FILL_BITS).sum()) == call.R.buf.numel() - call.R.view().numel()
    A, B, _ = call.case.reference()
    assert A.abs().min() >= 1 and A.abs().max() <= 4 and B.abs().min() >= 1 and torch.equal(A, A.round())


@pytest.mark.parametrize('fault,kw', [
    ('col_past_n', {}),                                      # one element stored just past column N of C
    ('row_after_m', {}),                                     # one stored in the row after M (of the last item: the guard band)
    ('item_gap', {}),                                        # one stored into the gap between two items
    ('ktail_times_zero', {}),                                # a k-tail staged from the padding and multiplied by zero
    ('ldb_is_width', {}),                                    # the logical width used as the pitch for B
    ('base_ignored', {}),                                    # the base offset ignored
    ('shared_a_strided', {'shared_a': True}),                # the second item of a shared A read at a non-zero stride
    ('k_term_dropped', {}),                                  # one k-term dropped
])
def test_planted_fault_is_caught(fault, kw):
    run(variants='padded', **kw)                             # (the same case without the fault passes)
    with pytest.raises(ContractViolation):
        run(fault, variants='padded', **kw)


def test_faults_in_the_arithmetic_are_caught_on_tight_operands_too():
    with pytest.raises(ContractViolation):
        run('k_term_dropped', variants='tight')
    with pytest.raises(ContractViolation):
        run('k_term_dropped', variants='odd', reduce=True)


def test_absmax_over_the_pitch_is_caught():
    call = Case('emulated', 8, 12, 16, 2, variants='padded').materialise(CPU)
    gc.check_absmax(emulated_absmax_rows(call.B), call.B)
    words = call.B.view().abs().amax(1).view(2, 3, 4).amax(2).contiguous().view(torch.int32)
    gc.check_absmax(words, call.B, grp=4)
    with pytest.raises(ContractViolation):
        gc.check_absmax(emulated_absmax_rows(call.B, over_pitch=True), call.B)


def test_workspace_guards_are_checked():
    call = Case('emulated', 7, 10, 5, 2, variants='padded', reduce=True).materialise(CPU)
    ws = call.workspace(40)
    assert ws.numel() == 40 and ws.data_ptr() % 16 == 0
    emulated_gemm(call)
    ws.fill_(0.0)
    call.check()
    call._ws[0][0][gc.GUARD + 40] = 0.0                     # the word after the workspace
    with pytest.raises(ContractViolation):
        call.check()


# ---- the predicates of the built library -----------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'equi-articulated-pose_amd', 'libeap_hip.so')
    assert os.path.exists(so), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(so)
    for n in ('eap_gemm_f32_reduce_workspace', 'eap_gemm_dma_f32_reduce_workspace', 'eap_gemm_bf16x3_reduce_workspace',
              'eap_gemm_skinny_reduce_workspace'):
        getattr(lib, n).restype = ctypes.c_int64
    return lib


PA, PB = 0x7F0000001000, 0x7F0000801000            # made-up 16-byte aligned addresses
I64, VP = ctypes.c_int64, ctypes.c_void_p

# argument order of each predicate; pointers by name
ORDER = {
    'eap_gemm_bf16x3_f32_supported': ('M', 'N', 'K', 'A', 'lda', 'B', 'ldb', 'strideB'),
    'eap_gemm_bf16x3_nn_f32_supported': ('M', 'N', 'K', 'A', 'lda', 'B', 'ldb', 'strideB'),
    'eap_gemm_bf16x3_reduce_f32_supported': ('M', 'N', 'K', 'A', 'lda', 'strideA', 'B', 'ldb', 'strideB', 'ldc'),
    'eap_gemm_dma_f32_supported': ('transA', 'transB', 'M', 'N', 'K', 'A', 'lda', 'strideA', 'B', 'ldb', 'strideB'),
    'eap_gemm_skinny_reduce_f32_supported': ('M', 'N', 'K', 'A', 'lda', 'strideA', 'B', 'ldb', 'strideB'),
}


def ask(lib, name, args):
    conv = []
    for k in ORDER[name]:
        v = args[k]
        conv.append(VP(v) if k in ('A', 'B') else I64(v) if k.startswith(('ld', 'stride')) else int(v))
    return int(getattr(lib, name)(*conv))


SPLIT_NT = dict(M=256, N=512, K=64, A=PA, lda=64 + 4, B=PB, ldb=64 + 8, strideB=512 * 72 + 20)
SPLIT_NN = dict(M=256, N=512, K=64, A=PA, lda=64 + 4, B=PB, ldb=512 + 8, strideB=64 * 520 + 20)
SPLIT_RED = dict(SPLIT_NT, strideA=256 * 68 + 20, ldc=512 + 12)
DMA = dict(transA=0, transB=1, M=100, N=260, K=48, A=PA, lda=52, strideA=100 * 52 + 20, B=PB, ldb=56, strideB=260 * 56 + 20)
SKINNY = dict(M=40, N=17, K=4099, A=PA, lda=4104, strideA=40 * 4104 + 20, B=PB, ldb=4108, strideB=17 * 4108 + 20)

SPLIT_DIMS_BAD = [dict(M=64), dict(N=128), dict(M=192), dict(M=384 + 64), dict(N=512 + 64), dict(K=8), dict(K=72)]
SPLIT_DIMS_OK = [dict(M=128), dict(N=256), dict(K=16), dict(M=128, N=256, K=16), dict(M=384), dict(N=384)]

TABLES = {
    'eap_gemm_bf16x3_f32_supported': (SPLIT_NT, SPLIT_DIMS_BAD + [
        dict(lda=66), dict(ldb=70), dict(strideB=512 * 72 + 21), dict(strideB=512 * 72 + 22), dict(A=PA + 4), dict(A=PA + 8), dict(B=PB + 4),
        dict(B=PB + 8), dict(lda=1 << 23), dict(ldb=1 << 23)],
        SPLIT_DIMS_OK + [dict(lda=(1 << 23) - 4), dict(ldb=(1 << 23) - 4), dict(strideB=0), dict(lda=64, ldb=64)]),
    'eap_gemm_bf16x3_nn_f32_supported': (SPLIT_NN, SPLIT_DIMS_BAD + [
        dict(lda=66), dict(A=PA + 4), dict(A=PA + 8), dict(ldb=511), dict(B=PB + 1), dict(B=PB + 2), dict(lda=1 << 23), dict(ldb=1 << 30)],
        SPLIT_DIMS_OK + [dict(ldb=512), dict(ldb=512 + 3), dict(B=PB + 4), dict(B=PB + 12), dict(strideB=64 * 520 + 21), dict(ldb=(1 << 30) - 1),
                         dict(lda=(1 << 23) - 4)]),
    'eap_gemm_bf16x3_reduce_f32_supported': (SPLIT_RED, SPLIT_DIMS_BAD + [
        dict(lda=66), dict(ldb=70), dict(strideA=256 * 68 + 21), dict(strideB=512 * 72 + 22), dict(ldc=512 + 13), dict(ldc=512 + 14), dict(A=PA + 4),
        dict(B=PB + 8), dict(lda=1 << 23), dict(ldb=1 << 23)],
        SPLIT_DIMS_OK + [dict(strideA=0), dict(ldc=512), dict(lda=(1 << 23) - 4)]),
    'eap_gemm_dma_f32_supported': (DMA, [
        dict(K=8), dict(K=40), dict(K=0), dict(lda=54), dict(ldb=58), dict(strideA=100 * 52 + 21), dict(strideB=260 * 56 + 22), dict(A=PA + 4),
        dict(A=PA + 8), dict(B=PB + 4), dict(transA=1, M=102), dict(transA=1, M=2), dict(transB=0, N=258), dict(transB=0, N=2), dict(M=0), dict(N=0)],
        [dict(K=16), dict(strideA=0), dict(M=1, N=1), dict(transA=1), dict(transB=0), dict(transA=1, transB=0, M=4, N=4), dict(M=102, N=258)]),
    'eap_gemm_skinny_reduce_f32_supported': (SKINNY, [
        dict(M=65), dict(N=33), dict(K=4095), dict(lda=4102), dict(ldb=4099), dict(strideA=40 * 4104 + 21), dict(strideB=17 * 4108 + 22), dict(A=PA + 4),
        dict(B=PB + 8), dict(M=0), dict(N=0)],
        [dict(M=64), dict(N=32), dict(K=4096), dict(M=1, N=1), dict(strideA=0), dict(K=5001)]),
}


@pytest.mark.parametrize('name', sorted(TABLES))
def test_predicate_table(lib, name):
    base, rejected, accepted = TABLES[name]
    assert ask(lib, name, base) == 1, ('baseline', base)
    for change in rejected:
        assert ask(lib, name, dict(base, **change)) == 0, ('must be rejected', change)
    for change in accepted:
        assert ask(lib, name, dict(base, **change)) == 1, ('must be accepted', change)


def test_split_counts_the_gpu_cases_rely_on(lib):
    """64 splits of 144 for K = 8201 / 8208 (splits 57 .. 63 are empty), 4 slabs and 1 slab on the split kernel"""
    def splits(fn, M, N, K, batch):
        words = int(getattr(lib, fn)(M, N, K, batch))
        assert words % (M * N * batch) == 0
        return words // (M * N * batch)

    assert splits('eap_gemm_f32_reduce_workspace', 100, 40, 8201, 16) == 64
    assert splits('eap_gemm_dma_f32_reduce_workspace', 128, 128, 8208, 16) == 64
    assert splits('eap_gemm_bf16x3_reduce_workspace', 128, 256, 4096, 2) == 4
    assert splits('eap_gemm_bf16x3_reduce_workspace', 128, 256, 1024, 1) == 1
    # the k-chunk both split-K reducers derive from 64 splits is 144: 57 * 144 >= K, seven splits start at or past the end
    for K in (8201, 8208):
        kchunk = ((K + 63) // 64 + 15) // 16 * 16
        assert kchunk == 144 and sum(1 for s in range(64) if s * kchunk >= K) == 7
