"""ctypes binding of libeap_hip.so -- the C ABI declared in include/eap_hip.h.

PyTorch is used for device memory and streams only: every call takes torch tensors, checks
them the way the reference's C++ wrappers do (device + contiguous, e.g.
vgtk/vgtk/cuda/zpconv_cuda.cpp:L37-39 CHECK_INPUT -> RuntimeError), and launches on the
CURRENT torch stream of the tensor's device (the reference launches on the legacy default
stream with no device guard, zpconv_cuda_kernel.cu:L219).

There is NO CPU or eager fallback: if the shared library is missing this module raises at
import, and non-device tensors are rejected.
"""
import ctypes
import os
import re
import struct
import types
import warnings
import weakref

import torch

_PKG_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
LIB_PATH = os.path.join(_PKG_ROOT, 'libeap_hip.so')

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f'{LIB_PATH} not found: build the HIP extension first '
        '(python -c "import __graft_entry__ as g; g.build()" or make -C equi-articulated-pose_amd/csrc). '
        'This package has no CPU fallback.')

lib = ctypes.CDLL(LIB_PATH)

# ---- typed prototypes, read from the header ---------------------------------------------------------
# include/eap_hip.h is plain C over a small fixed vocabulary (stated at its top).  Every `ret eap_name(params);` in it becomes one
# ctypes prototype, abi.<name>: the arity, the 64-bit and float positions and the 64-bit / string returns come from the declaration
# instead of from wrappers at the call sites, and a declaration outside the vocabulary stops the import.

# (the package carries a link to the header, so a copy of the package directory alone brings it along; the repository's own file otherwise)
_HEADERS = (os.path.join(_PKG_ROOT, 'include', 'eap_hip.h'), os.path.join(os.path.dirname(_PKG_ROOT), 'include', 'eap_hip.h'))
HEADER_PATH = next((p for p in _HEADERS if os.path.exists(p)), _HEADERS[-1])

_I64 = ctypes.c_int64
_F32 = ctypes.c_float


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class _Pointer:
    """argtype of a pointer parameter: None (NULL), an int address, a ctypes.c_void_p, or a DEVICE tensor whose element size is the
    pointee's (width 0, `void *`: any).  Width, not dtype: int32 views travel as `uint32_t *`, float bit patterns as `int32_t *`."""
    width = 0

    @classmethod
    def from_param(cls, v):
        if isinstance(v, torch.Tensor):
            if cls.width and v.element_size() != cls.width:
                raise RuntimeError(f'a {v.dtype} tensor ({v.element_size()} bytes per element) for a pointer to {cls.width}-byte elements')
            if not v.is_cuda:
                raise RuntimeError('tensor must be a CUDA(HIP) tensor')
            return ctypes.c_void_p(v.data_ptr())
        if isinstance(v, ctypes.c_void_p):
            return v
        if v is None or isinstance(v, int):
            return ctypes.c_void_p(v)
        raise TypeError(f'None, an address, a ctypes.c_void_p or a device tensor expected, not {type(v).__name__}')


_POINTERS = {w: type(f'_Pointer{w}', (_Pointer,), {'width': w}) for w in (0, 1, 4, 8)}
_POINTEES = {'void': 0, 'uint8_t': 1, 'float': 4, 'int32_t': 4, 'uint32_t': 4, 'double': 8, 'int64_t': 8, 'uint64_t': 8}
_SCALARS = {'int': ctypes.c_int, 'int64_t': _I64, 'float': _F32, 'eap_stream_t': ctypes.c_void_p}
_RETURNS = {'int': ctypes.c_int, 'int64_t': _I64, 'const char *': ctypes.c_char_p}


def _argtype(name, param):
    m = re.fullmatch(r'(const )?(\w+) ?(\*?) ?\w*', param)
    const, base, star = m.groups() if m else (None, None, None)
    if star and base in _POINTEES:
        return _POINTERS[_POINTEES[base]]
    if m and not star and not const and base in _SCALARS:
        return _SCALARS[base]
    raise ImportError(f'{HEADER_PATH}: {name}: parameter `{param}` is outside the vocabulary the binding accepts')


def _bind_header():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f'{HEADER_PATH} not found: the C ABI is bound from its header')
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER_PATH).read(), flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    abi = types.SimpleNamespace()
    for ret, name, params in re.findall(r'([^;{}()]*?)\b(eap_\w+)\s*\(([^()]*)\)\s*;', text):
        ret, params = ' '.join(ret.split()), [' '.join(p.split()) for p in params.split(',')]
        if ret not in _RETURNS:
            raise ImportError(f'{HEADER_PATH}: {name}: return type `{ret}` is outside the vocabulary the binding accepts')
        argtypes = [] if params == ['void'] else [_argtype(name, p) for p in params]
        setattr(abi, name, ctypes.CFUNCTYPE(_RETURNS[ret], *argtypes)((name, lib)))
        if ret != 'int':                 # `lib` stays an untyped handle: only the returns a C `int` would truncate are told to it
            getattr(lib, name).restype = _RETURNS[ret]
    return abi


abi = _bind_header()


def check_input(*tensors):
    """CHECK_INPUT of the reference C++ wrappers: device tensor + contiguous."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError('tensor must be a CUDA(HIP) tensor')
        if not t.is_contiguous():
            raise RuntimeError('tensor must be contiguous')


def stream_of(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


# Optional per-launch timing (bench.py): when KERNEL_TIMES is a list, every launch is bracketed
# by two HIP events recorded on the launch stream and (name, tag, start, stop) is appended.
KERNEL_TIMES = None


def _invoke(name, args):
    """abi.<name>(*args) with the argument count checked here (ctypes lets a surplus argument through) and a refused argument reported
    as the RuntimeError the callers of this package expect, naming the entry and the argument's position."""
    fn = getattr(abi, name)
    if len(args) != len(fn.argtypes):
        raise RuntimeError(f'{name} takes {len(fn.argtypes)} arguments (the stream last), {len(args)} given')
    try:
        return fn(*args)
    except ctypes.ArgumentError as e:
        raise RuntimeError(f'{name}: {e}') from None


def call(name, ref_tensor, *args, tag=None):
    """Invoke abi.<name>(*args, stream) under the device of `ref_tensor`; raise on error."""
    with torch.cuda.device(ref_tensor.device):
        if KERNEL_TIMES is not None:
            stream = torch.cuda.current_stream(ref_tensor.device)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            abi.eap_last_kernel()        # (clear)
            e0.record(stream)
            rc = _invoke(name, args + (stream_of(ref_tensor),))
            e1.record(stream)
            if tag is not None:          # the HIP kernel (with its template arguments) this entry just launched
                tag = dict(tag, kernel=abi.eap_last_kernel().decode() or name)
            KERNEL_TIMES.append((name, tag, e0, e1))
        else:
            rc = _invoke(name, args + (stream_of(ref_tensor),))
    if rc != 0:
        raise RuntimeError(f'{name} failed (hip error {rc}): {abi.eap_last_error().decode()}')


def suffix(t):
    if t.dtype == torch.float32:
        return 'f32'
    if t.dtype == torch.float64:
        return 'f64'
    raise RuntimeError(f'unsupported dtype {t.dtype} (float32 / float64 only)')


def use_ordered(ordered):
    """The `ordered=` keyword of the backward operators that have both a scatter kernel and an ordered one: None follows
    torch.are_deterministic_algorithms_enabled() (the rule of chamfer.backward), True / False force the choice."""
    return torch.are_deterministic_algorithms_enabled() if ordered is None else bool(ordered)


def no_deterministic(op, why, requested=False):
    """torch's contract for an op that is about to run a float-atomic scatter because no ordered kernel can serve the call: under
    torch.use_deterministic_algorithms(True) raise, under warn_only=True warn the same text and let the caller scatter, with the
    flag off say nothing.  requested: the caller passed ordered=True itself -- then the call is refused whatever the flag says."""
    msg = (f'{op} does not have a deterministic implementation for this call ({why}), but you set '
           '\'torch.use_deterministic_algorithms(True)\' or asked for ordered=True. You can turn off determinism just for this '
           'operation, or pass ordered=False to run its atomicAdd scatter.')
    if torch.are_deterministic_algorithms_enabled():
        if not torch.is_deterministic_algorithms_warn_only_enabled():
            raise RuntimeError(msg)
        warnings.warn(msg, stacklevel=3)
    elif requested:
        raise RuntimeError(msg)


# ---- raw launchers used by the operator layer ---------------------------------------------------

# csrc/gemm_dma_f32.hip (DMA-fed three-stage ring) serves every GEMM whose operands it can take (K a multiple of 16,
# 16-byte aligned rows); csrc/gemm_f32.hip the rest (first layer K = 24, blocked intermediates, odd shapes).


def _dma_ok(transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB):
    return bool(abi.eap_gemm_dma_f32_supported(int(transA), int(transB), M, N, K, A, lda, strideA,
                                               B, ldb, strideB))


# Contractions whose A operand is shared by the batch (the inter conv's forward contraction on the transposed
# intermediate, the pointwise contraction so3_contract, the implicit intra conv) on the 16-bit matrix cores with split
# operands, fp32 in, fp32 accumulate (csrc/gemm_bf16x3.hip).  False: the fp32-MFMA kernels everywhere.
SPLIT_BF16_CONTRACTION = True
# Planes per operand on those kernels: 3 = three bf16 planes, six products (exact splits); 2 = two fp16 planes after a
# power-of-two scale per tensor, three products (include/eap_hip.h, eap_gemm_f16x2_f32: representation error <= 2^-23 per
# element, bounded against fp64 by the fp32-MFMA kernel's error in tests/test_gpu_split_planes.py).
# Accuracy bar of the default (2): every product carries a representation error <= 2^-21 |a||b| (the l l' term is dropped: NOT
# bit-for-bit an fp32 product), and an operand row scaled from a BOUND on its magnitude that is L times too large adds an absolute
# 2^-39 L max|row| per element; against float64 the result stays within 1.25 x (max) / 1.1 x (rms) of the fp32-MFMA kernel's
# error on the same operands, with bounds up to 2^20 too large (README.md "Numerics", tests/test_gpu_split_planes.py).  3 planes
# are exact splits (dropped terms <= 2^-23 |a||b|) and need no magnitudes.
def _split_planes_from_env():
    v = os.environ.get('EAP_SPLIT_PLANES', '2')
    if v not in ('2', '3'):
        raise ImportError(f'EAP_SPLIT_PLANES={v!r}: 2 (two fp16 planes, three products) or 3 (three bf16 planes, six products)')
    return int(v)


SPLIT_PLANES = _split_planes_from_env()      # (EAP_SPLIT_PLANES: a numerics mode, README.md "Numerics")


SPLIT_PLANES_SCAN_ROWS = 384     # see _planes2 (tests set it to 0 to reach the two-plane kernel at every shape)


def _pieces_ok(t, *dims):
    return not any(int(d) & 3 for d in dims) and t.data_ptr() % 16 == 0


def absmax_rows(t, batch, rows, cols, ld, stride):
    """Largest magnitude of every row of a [batch][rows][cols] view (row pitch ld, item stride) -> int32 [batch, rows] holding
    float bit patterns, or None when the view is not made of whole, aligned 16-byte pieces."""
    if not _pieces_ok(t, cols, ld, stride):
        return None
    out = torch.empty(batch, rows, dtype=torch.int32, device=t.device)
    call('eap_absmax_rows_f32', t, t, batch, rows, cols, ld, stride, out)
    return out


def absmax_colgroups(t, batch, rows, cols, ld, stride, grp):
    """Largest magnitude over the rows and over each group of grp consecutive columns -> int32 [batch, cols // grp], or None."""
    if not _pieces_ok(t, cols, ld, stride, grp) or cols % grp:
        return None
    out = torch.empty(batch, cols // grp, dtype=torch.int32, device=t.device)
    call('eap_absmax_colgroups_f32', t, t, batch, rows, cols, ld, stride, grp, out)
    return out


def so3_grouped_bound(feats, idx):
    """A bound per point on the inter conv's grouped tensor, from the features' per-point maxima (include/eap_hip.h,
    eap_so3_grouped_bound_f32): feats [b,c,n,na], idx int32 [b,p,nn] -> int32 [b, p] (float bit patterns), or None."""
    b, c, n, na = feats.shape
    pm = absmax_colgroups(feats, b, c, n * na, n * na, c * n * na, na) if na % 4 == 0 else None
    if pm is None:
        return None
    out = torch.empty(b, idx.shape[1], dtype=torch.int32, device=feats.device)
    call('eap_so3_grouped_bound_f32', feats, b, idx.shape[1], idx.shape[2], n, pm, idx, out)
    return out


def _planes2(transB, M, N, K, A, lda, batch, B, ldb, strideB, b_bound):
    """The magnitude words of eap_gemm_f16x2_f32 -> (abs_a, abs_b, grp_b, mult_b), or None: take the three-plane kernel.
    b_bound = (words [batch, N // grp], grp, factor) when the caller knows a bound on B's columns."""
    if SPLIT_PLANES != 2:
        return None
    if b_bound is None and M < SPLIT_PLANES_SCAN_ROWS:
        # without a bound the kernel needs a pass over B first: 4 bytes per element at ~5 TB/s against the M / 2 fp32-equivalent
        # products per element it saves at ~245 TFLOP/s -- pays from M = 384 rows upwards
        return None
    abs_a = absmax_rows(A, 1, M, K, lda, 0)
    if abs_a is None:
        return None
    if b_bound is not None:
        return abs_a, b_bound[0], int(b_bound[1]), float(b_bound[2])
    abs_b = absmax_rows(B, batch, N, K, ldb, strideB) if transB else absmax_colgroups(B, batch, K, N, ldb, strideB, 4)
    return None if abs_b is None else (abs_a, abs_b, 1 if transB else 4, 1.0)


def _gemm_split(transB, M, N, K, A, lda, B, ldb, strideB, C, ldc, strideC, batch, b_bound, tag, epilogue=None):
    """C_z = A B_z on the split-operand kernels (csrc/gemm_bf16x3.hip: A shared by the batch, 'nt' or 'nn'), two fp16 planes where _planes2
    has the magnitudes, else three bf16 planes; epilogue = (scale, shift, slope, residual) of gemm_epilogue.  -> False when the operands do
    not qualify (nothing launched)."""
    tb = int(bool(transB))
    split = 'eap_gemm_bf16x3_f32' if tb else 'eap_gemm_bf16x3_nn_f32'
    if not getattr(abi, split + '_supported')(M, N, K, A, lda, B, ldb, strideB):
        return False
    ops = (M, N, K, A, lda, B, ldb, strideB, C, ldc, strideC, batch)
    ep = (None, None, 0.0, None, 0) if epilogue is None else (*epilogue, strideC)
    two = _planes2(tb, M, N, K, A, lda, batch, B, ldb, strideB, b_bound)
    if two is not None:
        call('eap_gemm_f16x2_f32', C, tb, *ops, two[0], two[1], two[2], two[3], *ep, tag=tag)
    elif epilogue is None:
        call(split, C, *ops, tag=tag)
    else:
        call('eap_gemm_bf16x3_ep_f32', C, tb, *ops, *ep, tag=tag)
    return True


def gemm(transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, batch, b_blocked=False, b_bound=None):
    """b_blocked: B is stored blocked by 4 (include/eap_hip.h); `ldb` is then ignored.  b_bound = (words int32 [batch, N // grp] holding
    non-negative float bit patterns, grp = consecutive columns per word, factor): words * factor bounds the magnitudes of B's columns,
    see _planes2 (saves the two-plane kernel its pass over B)."""
    tag = {'flops': 2.0 * M * N * K * batch, 'shape': ('gemm', int(transA), int(transB), M, N, K, batch)}
    if SPLIT_BF16_CONTRACTION and not b_blocked and not transA and (strideA == 0 or batch == 1) and \
            _gemm_split(transB, M, N, K, A, lda, B, ldb, strideB, C, ldc, strideC, batch, b_bound, tag):
        return
    if not b_blocked and _dma_ok(transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB):
        call('eap_gemm_dma_f32', C, int(transA), int(transB), M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, batch, tag=tag)
        return
    call('eap_gemm_f32_xb' if b_blocked else 'eap_gemm_f32', C, int(transA), int(transB), M, N, K, A, lda, strideA, B,
         (N if transB else K) if b_blocked else ldb, strideB, C, ldc, strideC, batch, tag=tag)


def gemm_epilogue(transB, M, N, K, A, lda, B, ldb, strideB, C, ldc, strideC, batch, scale, shift, slope, residual=None, b_bound=None):
    """C_z = leaky_relu(scale[row] * (A B_z) + shift[row], slope) (+ residual_z, laid out like C) on the split kernel
    (eap_gemm_bf16x3_ep_f32): an inference-mode BatchNorm + activation folded into the contraction.  -> False when the
    operands do not qualify for that kernel (nothing launched: the caller runs product and epilogue separately)."""
    tag = {'flops': 2.0 * M * N * K * batch, 'shape': ('gemm_epilogue', 0, int(transB), M, N, K, batch)}
    return bool(SPLIT_BF16_CONTRACTION and _gemm_split(transB, M, N, K, A, lda, B, ldb, strideB, C, ldc, strideC, batch, b_bound, tag,
                                                       (scale, shift, slope, residual)))


def gemm_reduce(transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, batch, b_blocked=False):
    tag = {'flops': 2.0 * M * N * K * batch, 'shape': ('gemm_reduce', int(transA), int(transB), M, N, K, batch)}
    ops = (M, N, K, A, lda, strideA, B, ldb, strideB)
    nt = not b_blocked and not transA and transB
    lead = (int(transA), int(transB))
    # (the predicate never sees C, whose float4 stores the entry requires 16-byte aligned: checked here, so such a C falls through)
    if SPLIT_BF16_CONTRACTION and nt and C.data_ptr() % 16 == 0 and abi.eap_gemm_bf16x3_reduce_f32_supported(*ops, ldc):
        name, ws_words, lead = 'eap_gemm_bf16x3_reduce_f32', abi.eap_gemm_bf16x3_reduce_workspace, ()      # ('nt' only: no transposition flags)
    elif nt and abi.eap_gemm_skinny_reduce_f32_supported(*ops):
        # a small output over a long contraction (the first layer's weight gradient): streaming reduction, csrc/gemm_skinny.hip
        name, ws_words, lead = 'eap_gemm_skinny_reduce_f32', abi.eap_gemm_skinny_reduce_workspace, ()
    elif not b_blocked and _dma_ok(transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB):
        name, ws_words = 'eap_gemm_dma_f32_reduce', abi.eap_gemm_dma_f32_reduce_workspace
    else:
        name, ws_words = 'eap_gemm_f32_reduce_xb' if b_blocked else 'eap_gemm_f32_reduce', abi.eap_gemm_f32_reduce_workspace
        if b_blocked:
            ops = ops[:7] + (N if transB else K,) + ops[8:]
    ws = torch.empty(max(int(ws_words(M, N, K, batch)), 1), dtype=torch.float32, device=C.device)
    call(name, C, *lead, *ops, C, ldc, batch, ws, tag=tag)


# ---- the same products stated as tensor views -----------------------------------------------------
# What vgtk/so3conv/functional.py calls: each operand a 2-D view [rows, cols] or a stack [batch, rows, cols] -- a slice of a larger buffer
# (row pitch, item stride, storage offset), transposed or not.  The numbers of gemm / gemm_reduce / gemm_epilogue are read off the
# views and checked against each other and against the views' storage before anything is launched.

def operand(t, name='operand', dtype=torch.float32):
    """A float32 (dtype: float64 for the float64 regime) matrix view -> (trans, ld, stride, batch, rows, cols): what a GEMM entry is told about the memory behind it.  rows, cols
    are the view's last two sizes; a 2-D view is one matrix shared by the batch (batch 1, stride 0), a 3-D view has batch = size(0) and
    stride = stride(0).  trans = 0: the columns are contiguous (stride(-1) == 1) and ld = stride(-2) as torch reports it; trans = 1: the rows
    are (stride(-2) == 1, the .transpose(-1, -2) of a row-major matrix) and ld = stride(-1).  A dimension of size 1 can make both readings
    possible: trans = 0 wins.  Raises RuntimeError for another dtype or rank, when neither of the two strides is 1, and when the elements
    addressed -- (batch - 1) * stride + (outer - 1) * ld + inner from the first -- do not fit the view's storage."""
    shape, strides = t.shape, t.stride()
    if t.dtype != dtype or len(shape) not in (2, 3):
        raise RuntimeError(f'{name}: a {str(dtype)[6:]} view [rows, cols] or [batch, rows, cols], not {t.dtype} {tuple(shape)}')
    rows, cols = shape[-2], shape[-1]
    if strides[-1] == 1:
        trans, ld, outer, inner = 0, strides[-2], rows, cols
    elif strides[-2] == 1:
        trans, ld, outer, inner = 1, strides[-1], cols, rows
    else:
        raise RuntimeError(f'{name}: neither the rows nor the columns are contiguous (strides {strides})')
    batch, stride = (shape[0], strides[0]) if len(shape) == 3 else (1, 0)
    extent = (batch - 1) * stride + (outer - 1) * ld + inner
    if t.element_size() * (t.storage_offset() + extent) > t.untyped_storage().nbytes():
        raise RuntimeError(f'{name}: {tuple(shape)} with strides {strides} at offset {t.storage_offset()} addresses {extent} elements, '
                           f'its storage holds {t.untyped_storage().nbytes() // t.element_size()}')
    return trans, ld, stride, batch, rows, cols


def _product(A, B, out, reduce=False):
    """The numbers of out_z = A_z B_z (reduce: out = sum_z A_z B_z, out 2-D) from the three views, after the checks of `operand` and: the
    inner sizes, the outer sizes and the batch counts agree, out is row-major and its rows and items do not overlap.
    The three views are float32, or ALL float64 (the float64 regime, csrc/so3_f64.hip): a mixed set is refused, naming the offender.
    -> (transA, transB, M, N, K, lda, strideA, ldb, strideB, ldc, strideC, batch)"""
    dtype = torch.float64 if all(t.dtype == torch.float64 for t in (A, B, out)) else torch.float32
    ta, lda, sa, ba, M, K = operand(A, 'A', dtype)
    tb, ldb, sb, batch, Kb, N = operand(B, 'B', dtype)
    tc, ldc, sc, bc, Mc, Nc = operand(out, 'out', dtype)
    if B.dim() != 3 or out.dim() != 3 - reduce:
        raise RuntimeError(f'B is a stack of matrices, out {"one matrix" if reduce else "a stack"}: got B {tuple(B.shape)}, out {tuple(out.shape)}')
    if K != Kb or (M, N) != (Mc, Nc) or (A.dim() == 3 and ba != batch) or bc != (1 if reduce else batch):
        raise RuntimeError(f'A {tuple(A.shape)} x B {tuple(B.shape)} -> out {tuple(out.shape)}: the sizes do not agree')
    if tc:
        raise RuntimeError(f'out must be row-major (strides {tuple(out.stride())})')
    if (M > 1 and ldc < N) or (bc > 1 and sc < (M - 1) * ldc + N):
        raise RuntimeError(f'out {tuple(out.shape)} with strides {tuple(out.stride())} overlaps itself')
    return ta, tb, M, N, K, lda, sa, ldb, sb, ldc, sc, batch


# One 128-row tile and a long contraction (the dense layers' feature gradient dF = W2 Z: 34 column tiles x 8 clouds = 272 workgroups of
# 768 k-tiles on 256 CUs) runs with its contraction cut into slabs (eap_gemm_f16x2_splitk_f32).  False: one slab, as `gemm` runs it.
SPLIT_K_ONE_ROW_TILE = True


def _matmul_split_k(M, N, K, A, lda, B, ldb, sb, out, ldc, sc, batch, b_bound):
    """the two-plane 'nn' product of the shape class M = 128, K >= 16 * 64 over several k-slabs -> False when the product is not of that
    class, the launcher would take one slab or the operands do not qualify (nothing launched)"""
    if not (SPLIT_K_ONE_ROW_TILE and SPLIT_BF16_CONTRACTION and M == 128 and K >= 16 * 64 and out.is_cuda and sc == M * ldc and ldc % 4 == 0
            and out.data_ptr() % 16 == 0 and abi.eap_gemm_bf16x3_nn_f32_supported(M, N, K, A, lda, B, ldb, sb)):
        return False
    slabs = abi.eap_gemm_f16x2_splitk_slabs(M, N, K, batch, 0)
    if slabs <= 1:
        return False
    two = _planes2(0, M, N, K, A, lda, batch, B, ldb, sb, b_bound)
    if two is None:
        return False
    floats = int(abi.eap_gemm_f16x2_splitk_workspace(M, N, batch, slabs))
    work = torch.empty(floats, dtype=torch.float32, device=out.device)
    tag = {'flops': 2.0 * M * N * K * batch, 'shape': ('gemm', 0, 0, M, N, K, batch)}
    call('eap_gemm_f16x2_splitk_f32', out, M, N, K, A, lda, B, ldb, sb, out, ldc, sc, batch, two[0], two[1], two[2], two[3], slabs, work, floats, tag=tag)
    return True


def matmul(A, B, out, b_bound=None):
    """out_z = A_z B_z: `gemm` with its numbers taken from the views (b_bound: see gemm)."""
    ta, tb, M, N, K, lda, sa, ldb, sb, ldc, sc, batch = _product(A, B, out)
    if out.dtype == torch.float64:       # the float64 regime: one kernel for every form (csrc/so3_f64.hip)
        call('eap_gemm_f64', out, int(ta), int(tb), M, N, K, A, lda, sa, B, ldb, sb, out, ldc, sc, batch,
             tag={'flops': 2.0 * M * N * K * batch, 'shape': ('gemm_f64', int(ta), int(tb), M, N, K, batch)})
        return
    if not ta and not tb and (sa == 0 or batch == 1) and _matmul_split_k(M, N, K, A, lda, B, ldb, sb, out, ldc, sc, batch, b_bound):
        return
    gemm(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, out, ldc, sc, batch, b_bound=b_bound)


def matmul_reduce(A, B, out, accumulate=False):
    """out [M, N] = sum_z A_z B_z: `gemm_reduce` with its numbers taken from the views.  float64 views: every item's product from zero,
    added in item order; accumulate (float64 only): onto what out holds -- the slabs of one batch give the bits of one call."""
    ta, tb, M, N, K, lda, sa, ldb, sb, ldc, _, batch = _product(A, B, out, reduce=True)
    if out.dtype == torch.float64:
        call('eap_gemm_f64_reduce', out, int(ta), int(tb), M, N, K, A, lda, sa, B, ldb, sb, out, ldc, batch, int(bool(accumulate)),
             tag={'flops': 2.0 * M * N * K * batch, 'shape': ('gemm_f64_reduce', int(ta), int(tb), M, N, K, batch)})
        return
    if accumulate:
        raise RuntimeError('matmul_reduce: accumulate is the float64 regime\'s (float32 products reduce through a workspace)')
    gemm_reduce(ta, tb, M, N, K, A, lda, sa, B, ldb, sb, out, ldc, batch)


def matmul_reduce_takes_split(A, B, out):
    """Would matmul_reduce(A, B, out) run on the split-bf16 kernel?  Asks what gemm_reduce asks before it takes that kernel: besides the
    kernel's own predicate (all gemm_reduce_takes_split asked), that the product is 'nt' and that out is 16-byte aligned."""
    ta, tb, M, N, K, lda, sa, ldb, sb, ldc, _, _ = _product(A, B, out, reduce=True)
    return bool(out.dtype == torch.float32 and SPLIT_BF16_CONTRACTION and not ta and tb and out.data_ptr() % 16 == 0 and
                abi.eap_gemm_bf16x3_reduce_f32_supported(M, N, K, A, lda, sa, B, ldb, sb, ldc))


def matmul_epilogue(A, B, out, scale, shift, slope, residual=None, b_bound=None):
    """`gemm_epilogue` with its numbers taken from the views: A one row-major matrix shared by the batch; the residual a float32 tensor of
    out's shape (trailing dimensions may be split or merged) whose elements sit at out's pitch and item stride: contiguous where out is, else
    with out's strides.  -> False when the split kernel does not take the operands (nothing launched)."""
    ta, tb, M, N, K, lda, sa, ldb, sb, ldc, sc, batch = _product(A, B, out)
    if out.dtype != torch.float32:
        raise RuntimeError('matmul_epilogue: the folded epilogue is float32 only, float64 products have none')
    if ta or (sa != 0 and batch != 1):
        raise RuntimeError(f'A must be one row-major matrix shared by the batch, not {tuple(A.shape)} with strides {tuple(A.stride())}')
    if residual is not None:
        tight = residual.is_contiguous() and residual.numel() == batch * M * N and (ldc, sc) == (N, M * N)
        if residual.dtype != torch.float32 or not (tight or (residual.shape == out.shape and residual.stride() == out.stride())):
            raise RuntimeError(f'residual: float32 laid out like out {tuple(out.shape)} with strides {out.stride()}, not {residual.dtype} '
                               f'{tuple(residual.shape)} with strides {residual.stride()}')
        operand(residual.view(batch, M, N) if tight else residual, 'residual')
    return gemm_epilogue(tb, M, N, K, A, lda, B, ldb, sb, out, ldc, sc, batch, scale, shift, slope, residual, b_bound)


def so3_prep(q_xyz, s_xyz, idx, q_pose, s_pose, anchors, identity_anchor):
    b, _, p = q_xyz.shape
    n = s_xyz.shape[2]
    nn = idx.shape[2]
    gx = torch.empty(b, p, nn, 4, dtype=torch.float32, device=q_xyz.device)
    nonident = torch.empty(b, dtype=torch.int32, device=q_xyz.device)
    call('eap_so3_prep_f32', gx, b, p, n, nn, anchors.shape[0], q_xyz, s_xyz, idx, q_pose, s_pose, anchors, int(identity_anchor), gx, nonident)
    return gx, nonident


def so3_inter_weights(gx, rk, sigma):
    b, p, nn, _ = gx.shape
    na, ks, _ = rk.shape
    w = torch.empty(b, p, na, ks, nn, dtype=torch.float32, device=gx.device)
    call('eap_so3_inter_weights_f32', w, b, p, nn, na, ks, sigma, gx, rk, w)
    return w


# ---- the float64 regime of the SO(3) conv layers (csrc/so3_f64.hip) -----------------------------------------

def _all_f64(op, **tensors):
    """every floating tensor of a float64 call is a float64 DEVICE tensor, else RuntimeError naming the offender"""
    for name, t in tensors.items():
        if t is not None and t.dtype != torch.float64:
            raise RuntimeError(f'{op}: {name} is {t.dtype} in a float64 call (every tensor of a call has one width)')
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise RuntimeError(f'{op}: {name} must be a device tensor (the float64 regime has no CPU path either)')


def so3_prep_f64(q_xyz, s_xyz, idx, q_pose, s_pose, anchors, identity_anchor):
    """-> g float64 [b,p,nn,3], r int32 [b,p,nn], nonident int32 [b] (include/eap_hip.h)"""
    _all_f64('so3_prep_f64', q_xyz=q_xyz, s_xyz=s_xyz, q_pose=q_pose, s_pose=s_pose, anchors=anchors)
    check_input(q_xyz, s_xyz, idx, q_pose, s_pose, anchors)
    b, _, p = q_xyz.shape
    n = s_xyz.shape[2]
    nn = idx.shape[2]
    g = torch.empty(b, p, nn, 3, dtype=torch.float64, device=q_xyz.device)
    r = torch.empty(b, p, nn, dtype=torch.int32, device=q_xyz.device)
    nonident = torch.empty(b, dtype=torch.int32, device=q_xyz.device)
    call('eap_so3_prep_f64', g, b, p, n, nn, anchors.shape[0], q_xyz, s_xyz, idx, q_pose, s_pose, anchors, int(identity_anchor), g, r, nonident)
    return g, r, nonident


def so3_inter_weights_f64(g, rk, sigma):
    _all_f64('so3_inter_weights_f64', g=g, rk=rk)
    check_input(g, rk)
    b, p, nn, _ = g.shape
    na, ks, _ = rk.shape
    w = torch.empty(b, p, na, ks, nn, dtype=torch.float64, device=g.device)
    call('eap_so3_inter_weights_f64', w, b, p, nn, na, ks, _f64_bits(sigma), g, rk, w)
    return w


def so3_inter_group_fwd_f64(feats, idx, g, r, rk, mult, sigma):
    """-> X float64 [b,c,ks,p,na]"""
    _all_f64('so3_inter_group_fwd_f64', feats=feats, g=g, rk=rk)
    check_input(feats, idx, g, r, rk, mult)
    b, c, n, na = feats.shape
    p, nn = idx.shape[1], idx.shape[2]
    ks = rk.shape[1]
    if rk.shape[0] != na or tuple(g.shape) != (b, p, nn, 3) or tuple(r.shape) != (b, p, nn):
        raise RuntimeError('so3_inter_group_fwd_f64: feats [b,c,n,na], idx [b,p,nn], g [b,p,nn,3], r [b,p,nn], rk [na,ks,3] do not agree')
    out = torch.empty(b, c, ks, p, na, dtype=torch.float64, device=feats.device)
    call('eap_so3_inter_group_fwd_f64', out, b, c, p, n, nn, na, ks, _f64_bits(sigma), feats, idx, g, r, rk, mult, out,
         tag={'flops': 2.0 * b * c * ks * p * nn * na, 'shape': ('group_fwd_f64', b, c, p, nn, na, ks)})
    return out


def inv_lists_entries(idx, rows, off):
    """the entry numbers p * nn + n of every referenced row of idx [b,p,nn], ascending, at [off, off + cnt) -> int32 [b, p*nn]"""
    check_input(idx, rows, off)
    b, p, nn = idx.shape
    ent = torch.empty(b, p * nn, dtype=torch.int32, device=idx.device)
    call('eap_inv_lists_entries', idx, b, p, rows.shape[1], nn, idx, rows, off, ent)
    return ent


def so3_inter_group_bwd_f64(gout, lists, g, r, rk, multinv, sigma, n, nn):
    """gout [b,c,ks,p,na], lists = (rows, off, cnt, ent) -> gfeats float64 [b,c,n,na]; no float atomics, one order"""
    _all_f64('so3_inter_group_bwd_f64', gout=gout, g=g, rk=rk)
    rows, off, cnt, ent = lists
    check_input(gout, rows, off, cnt, ent, g, r, rk, multinv)
    b, c, ks, p, na = gout.shape
    if tuple(rows.shape) != (b, n) or tuple(ent.shape) != (b, p * nn) or tuple(g.shape) != (b, p, nn, 3) or tuple(rk.shape) != (na, ks, 3):
        raise RuntimeError('so3_inter_group_bwd_f64: gout [b,c,ks,p,na], rows [b,n], ent [b,p*nn], g [b,p,nn,3], rk [na,ks,3] do not agree')
    gfeats = torch.empty(b, c, n, na, dtype=torch.float64, device=gout.device)
    call('eap_so3_inter_group_bwd_f64', gfeats, b, c, p, n, nn, na, ks, _f64_bits(sigma), gout, rows, off, cnt, ent, g, r, rk, multinv, gfeats,
         tag={'flops': 2.0 * b * c * ks * p * nn * na, 'shape': ('group_bwd_f64', b, c, p, nn, na, ks)})
    return gfeats


def so3_intra_group_fwd_f64(feats, intra_idx):
    _all_f64('so3_intra_group_fwd_f64', feats=feats)
    check_input(feats, intra_idx)
    b, c, p, na = feats.shape
    t = intra_idx.shape[1]
    if intra_idx.shape[0] != na:
        raise RuntimeError(f'so3_intra_group_fwd_f64: {na} anchors, an index table of {intra_idx.shape[0]} rows')
    out = torch.empty(b, c, t, p, na, dtype=torch.float64, device=feats.device)
    call('eap_so3_intra_group_fwd_f64', out, b, c, p, na, t, feats, intra_idx, out)
    return out


def so3_intra_group_bwd_f64(gout, intra_idx):
    _all_f64('so3_intra_group_bwd_f64', gout=gout)
    check_input(gout, intra_idx)
    b, c, t, p, na = gout.shape
    if tuple(intra_idx.shape) != (na, t):
        raise RuntimeError(f'so3_intra_group_bwd_f64: gout {tuple(gout.shape)}, an index table {tuple(intra_idx.shape)}')
    gfeats = torch.empty(b, c, p, na, dtype=torch.float64, device=gout.device)
    call('eap_so3_intra_group_bwd_f64', gfeats, b, c, p, na, t, gout, intra_idx, gfeats)
    return gfeats


def so3_anchor_perm(gx, mult):
    b, p, nn, _ = gx.shape
    na = mult.shape[0]
    perm = torch.empty(b, p, nn, na, dtype=torch.int64, device=gx.device)
    call('eap_so3_anchor_perm', gx, b, p, nn, na, gx, mult, perm)
    return perm




def so3_anchor_map(idx, q_pose, s_pose, anchors):
    """The per-entry anchor index of an anchor set that is not a group (csrc/so3_anchor_map.hip; so3conv/functional.py:L1199-1204):
    idx int32 [b,p,nn], q_pose [b,p,4,4], s_pose [b,n,4,4], anchors [na,3,3] -> (amap uint8 [b,p,nn,na], nontrivial int32 [b])."""
    check_input(idx, q_pose, s_pose, anchors)
    b, p, nn = idx.shape
    na = anchors.shape[0]
    if tuple(q_pose.shape) != (b, p, 4, 4) or s_pose.shape[0] != b or tuple(s_pose.shape[2:]) != (4, 4):
        raise RuntimeError('so3_anchor_map: poses must be [b,p,4,4] (query) and [b,n,4,4] (support)')
    amap = torch.empty(b, p, nn, na, dtype=torch.uint8, device=idx.device)
    nontrivial = torch.empty(b, dtype=torch.int32, device=idx.device)
    call('eap_so3_anchor_map_f32', amap, b, p, s_pose.shape[1], nn, na, idx, q_pose, s_pose, anchors, amap, nontrivial)
    return amap, nontrivial


def _check_map(amap, idx, na):
    if amap.dtype != torch.uint8 or tuple(amap.shape) != tuple(idx.shape) + (na,) or not amap.is_contiguous():
        raise RuntimeError('anchor map: contiguous uint8 [b,p,nn,na] expected')


def so3_inter_group_fwd_map(feats, idx, gx, rk, amap, sigma):
    """-> X [b,c,ks,p,na] (reference layout), the gather through the per-entry anchor map (csrc/so3_inter_map.hip)"""
    b, c, n, na = feats.shape
    p, nn = idx.shape[1], idx.shape[2]
    ks = rk.shape[1]
    _check_map(amap, idx, na)
    out = torch.empty(b, c, ks, p, na, dtype=torch.float32, device=feats.device)
    call('eap_so3_inter_group_fwd_map_f32', out, b, c, p, n, nn, na, ks, sigma, feats, idx, gx, rk, amap, out,
         tag={'flops': 2.0 * b * c * ks * p * nn * na, 'shape': ('group_fwd_map', b, c, p, nn, na, ks)})
    return out


def so3_inter_group_bwd_map(gout, idx, gx, rk, amap, sigma, n):
    """gout [b,c,ks,p,na] -> gfeats [b,c,n,na] through the per-entry anchor map; no float atomics (csrc/so3_inter_map.hip)"""
    b, c, ks, p, na = gout.shape
    nn = idx.shape[2]
    _check_map(amap, idx, na)
    gfeats = torch.empty(b, c, n, na, dtype=torch.float32, device=gout.device)
    ws = torch.empty(max(1, int(abi.eap_so3_inter_group_bwd_map_workspace(b, c, p, n, na))), dtype=torch.float32, device=gout.device)
    call('eap_so3_inter_group_bwd_map_f32', gfeats, b, c, p, n, nn, na, ks, sigma, gout, idx, gx, rk, amap, gfeats, ws)
    return gfeats


# ---- the `use_2d` variant with really permuted residual indices (csrc/so3_inter_res.hip) ----------

RESIDUAL_IDENTITY_BYTE = 0xE4        # field z = z


def residual_index_pack(fields):
    """rotated_anchor_idx [...,4] with values 0..3 (any integer dtype, host or device) -> uint8 [...]: field z in bits 2z, 2z+1, the byte
    eap_so3_residual_index_f32 writes and the `use_2d` grouping kernels read"""
    if fields.shape[-1] != 4 or fields.dtype.is_floating_point or bool(((fields < 0) | (fields > 3)).any()):
        raise RuntimeError('residual index: integers 0..3 in a last dimension of 4')
    f = fields.to(torch.int32)
    return (f[..., 0] | (f[..., 1] << 2) | (f[..., 2] << 4) | (f[..., 3] << 6)).to(torch.uint8)


def residual_index_unpack(packed):
    """uint8 [...] -> int64 [...,4]: the inverse of residual_index_pack (what torch.argmax returns in the reference)"""
    if packed.dtype != torch.uint8:
        raise RuntimeError('residual index: uint8 bytes expected')
    v = packed.to(torch.int64)
    return torch.stack([(v >> (2 * z)) & 3 for z in range(4)], dim=-1)


def so3_residual_index(idx, q_pose, s_pose, res):
    """The per-entry residual index of the `use_2d` conv (so3conv/functional.py:L1934-1938): idx int32 [b,p,nn], q_pose [b,p,4,4],
    s_pose [b,n,4,4], res [4,3,3] -> (shift uint8 [b,p,nn], see residual_index_unpack; nontrivial int32 [b])."""
    check_input(idx, q_pose, s_pose, res)
    b, p, nn = idx.shape
    if tuple(q_pose.shape) != (b, p, 4, 4) or s_pose.dim() != 4 or s_pose.shape[0] != b or tuple(s_pose.shape[2:]) != (4, 4):
        raise RuntimeError('so3_residual_index: poses must be [b,p,4,4] (query) and [b,n,4,4] (support)')
    if tuple(res.shape) != (4, 3, 3) or idx.dtype != torch.int32 or any(t.dtype != torch.float32 for t in (q_pose, s_pose, res)):
        raise RuntimeError('so3_residual_index: int32 idx, float32 poses, float32 res [4,3,3]')
    shift = torch.empty(b, p, nn, dtype=torch.uint8, device=idx.device)
    nontrivial = torch.empty(b, dtype=torch.int32, device=idx.device)
    call('eap_so3_residual_index_f32', shift, b, p, s_pose.shape[1], nn, idx, q_pose, s_pose, res, shift, nontrivial)
    return shift, nontrivial


def _check_res(feats_like, idx, gx, rk, shift, na4):
    check_input(feats_like, idx, gx, rk, shift)
    if na4 % 4 != 0 or tuple(rk.shape) != (na4, rk.shape[1], 3):
        raise RuntimeError('use_2d grouping: na x 4 anchors, rk [na*4,ks,3]')
    if shift.dtype != torch.uint8 or tuple(shift.shape) != tuple(idx.shape) or idx.dtype != torch.int32:
        raise RuntimeError('use_2d grouping: idx int32 [b,p,nn] and the residual index uint8 [b,p,nn]')
    if tuple(gx.shape) != tuple(idx.shape) + (4,) or any(t.dtype != torch.float32 for t in (feats_like, gx, rk)):
        raise RuntimeError('use_2d grouping: float32 tensors, gx [b,p,nn,4]')


def so3_inter_group_fwd_res(feats, idx, gx, rk, shift, sigma):
    """feats [b,c,n,na*4] -> X [b,c,ks,p,na*4] (reference layout): the gather through the per-entry residual index, any byte
    (csrc/so3_inter_res.hip)"""
    b, c, n, na4 = feats.shape
    p, nn = idx.shape[1], idx.shape[2]
    ks = rk.shape[1]
    _check_res(feats, idx, gx, rk, shift, na4)
    out = torch.empty(b, c, ks, p, na4, dtype=torch.float32, device=feats.device)
    call('eap_so3_inter_group_fwd_res_f32', out, b, c, p, n, nn, na4 // 4, ks, sigma, feats, idx, gx, rk, shift, out,
         tag={'flops': 2.0 * b * c * ks * p * nn * na4, 'shape': ('group_fwd_res', b, c, p, nn, na4, ks)})
    return out


def so3_inter_group_bwd_res(gout, idx, gx, rk, shift, sigma, n):
    """gout [b,c,ks,p,na*4] -> gfeats [b,c,n,na*4] through the per-entry residual index; no float atomics (csrc/so3_inter_res.hip)"""
    b, c, ks, p, na4 = gout.shape
    nn = idx.shape[2]
    _check_res(gout, idx, gx, rk, shift, na4)
    gfeats = torch.empty(b, c, n, na4, dtype=torch.float32, device=gout.device)
    ws = torch.empty(max(1, int(abi.eap_so3_inter_group_bwd_res_workspace(b, c, p, n, na4 // 4))), dtype=torch.float32, device=gout.device)
    call('eap_so3_inter_group_bwd_res_f32', gfeats, b, c, p, n, nn, na4 // 4, ks, sigma, gout, idx, gx, rk, shift, gfeats, ws,
         tag={'flops': 2.0 * b * c * ks * p * nn * na4, 'shape': ('group_bwd_res', b, c, p, nn, na4, ks)})
    return gfeats


def so3_inter_group_fwd_can_block(c, n, na, ks, has_mult, has_flag):
    return bool(abi.eap_so3_inter_group_fwd_can_block(c, n, na, ks, int(has_mult), int(has_flag)))


_TP_COLUMNS = {}


def so3_group_fwd_tp_takes(c, na, ks):
    return bool(abi.eap_so3_group_fwd_tp_takes(int(c), int(na), int(ks)))


def so3_group_fwd_tp_columns(c, ks, device):
    """int64 [c*ks] on `device`: position j of a row of the store-order transposed intermediate holds column perm[j] of the
    plain one (include/eap_hip.h: eap_so3_group_fwd_tp_columns)."""
    key = (int(c), int(ks), str(device))
    hit = _TP_COLUMNS.get(key)
    if hit is None:
        import numpy as np
        perm = np.empty(c * ks, np.int32)
        if abi.eap_so3_group_fwd_tp_columns(int(c), int(ks), perm.ctypes.data_as(ctypes.c_void_p)) != 0:
            raise RuntimeError(abi.eap_last_error().decode())
        hit = _TP_COLUMNS[key] = torch.from_numpy(perm.astype(np.int64)).to(device)
    return hit


def so3_inter_group_fwd(feats, idx, gx, rk, mult, sigma, nonident=None, blocked=False, coset=None, store_order=False):
    """-> X [b,c,ks,p,na]; with `blocked` the same numbers as [b,p,na/4,c,ks,4] (returned with the
    nominal shape: only eap_gemm_f32_xb may read it).  coset = the coset tables of `mult`
    (vgtk.so3conv.functional._coset_tables): permuted clouds of the transposed layout take the two-tile kernel.
    store_order: the transposed intermediate with its columns in the kernel's store order (so3_group_fwd_tp_columns) -- only a
    contraction with W[:, columns] may read it."""
    b, c, n, na = feats.shape
    p, nn = idx.shape[1], idx.shape[2]
    ks = rk.shape[1]
    out = torch.empty(b, c, ks, p, na, dtype=torch.float32, device=feats.device)
    tag = lambda kind: {'flops': 2.0 * b * c * ks * p * nn * na, 'shape': (kind, b, c, p, nn, na, ks)}
    if (coset is not None and int(blocked) == 2 and mult is not None and nonident is not None and nn > 0
            and so3_group_perm_lists2_takes(c, na, ks, n)):
        # clouds with anchor permutations on the two-tile kernel (csrc/so3_inter_lists2.hip, PERM): their features with a coset-major
        # anchor axis, the per-entry words of (idx, gx) prepared once; clouds whose flag is 0 cost three empty launches
        feats_c = torch.empty_like(feats)
        call('eap_anchor_reorder_clouds_f32', feats, b, c * n, na, feats, coset[0], nonident, feats_c)
        ent_pc, ent_gx2 = so3_perm_entries(idx.view(b, p * nn), gx.view(b, p * nn, 4), coset[1], None, 0, na, n, nonident)
        call('eap_so3_inter_group_fwd_perm2_t_f32', out, b, c, p, n, nn, na, ks, sigma, feats, feats_c, idx, gx, ent_pc, ent_gx2, rk, coset[0],
             nonident, int(bool(store_order)), out, tag=tag('group_fwd_perm2'))
        return out
    if store_order:
        if mult is not None or int(blocked) != 2:
            raise RuntimeError('store-order columns: transposed layout, clouds without permutation (or the coset tables for the flagged ones)')
        call('eap_so3_inter_group_fwd_tp_f32', out, b, c, p, n, nn, na, ks, sigma, feats, idx, gx, rk, out, tag=tag('group_fwd_tp'))
        return out
    call({0: 'eap_so3_inter_group_fwd_f32', 1: 'eap_so3_inter_group_fwd_xb_f32', 2: 'eap_so3_inter_group_fwd_t_f32'}[int(blocked)], out, b, c, p, n,
         nn, na, ks, sigma, feats, idx, gx, rk, mult, nonident, out, tag=tag('group_fwd'))
    return out


FORCE_ATOMIC_BWD = False


def so3_inter_group_bwd(gout, idx, gx, rk, mult, sigma, n, identity_anchor=0):
    b, c, ks, p, na = gout.shape
    nn = idx.shape[2]
    gfeats = torch.empty(b, c, n, na, dtype=torch.float32, device=gout.device)
    if ks <= 24 and na % 4 == 0 and not FORCE_ATOMIC_BWD:
        ws = torch.empty(int(abi.eap_so3_inter_group_bwd_workspace(b, c, p, n, na)), dtype=torch.float32,
                         device=gout.device)
        call('eap_so3_inter_group_bwd_slab_f32', gfeats, b, c, p, n, nn, na, ks, sigma, gout, idx, gx, rk, mult, int(identity_anchor), gfeats, ws)
        return gfeats
    # (the one SO(3) site that still scatters: float atomicAdd into gfeats)
    no_deterministic('so3_inter_group_bwd', 'FORCE_ATOMIC_BWD is set' if FORCE_ATOMIC_BWD else
                     f'ks = {ks}, na = {na}: the atomics-free kernel takes ks <= 24 and na % 4 == 0')
    call('eap_so3_inter_group_bwd_f32', gfeats, b, c, p, n, nn, na, ks, sigma, gout, idx, gx, rk, mult, gfeats)
    return gfeats


def so3_intra_group_fwd(feats, intra_idx):
    b, c, p, na = feats.shape
    t = intra_idx.shape[1]
    out = torch.empty(b, c, t, p, na, dtype=torch.float32, device=feats.device)
    call('eap_so3_intra_group_fwd_f32', out, b, c, p, na, t, feats, intra_idx, out)
    return out


def so3_intra_group_bwd(gout, intra_idx):
    b, c, t, p, na = gout.shape
    gfeats = torch.empty(b, c, p, na, dtype=torch.float32, device=gout.device)
    call('eap_so3_intra_group_bwd_f32', gfeats, b, c, p, na, t, gout, intra_idx, gfeats)
    return gfeats


def _quads(t):
    """`t` contiguous with its first element on a 16-byte boundary (the 2-D grouping kernels move an anchor's four residuals as one
    quad): `t` itself where it already is, else a copy."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _residuals(tot, na):
    """residuals per anchor of an anchor axis of `tot` = na * nr entries, the residual innermost"""
    if na <= 0 or tot % na:
        raise RuntimeError(f'an anchor axis of {tot} entries is not (na = {na}) x residuals')
    return tot // na


def so3_intra_group2d_fwd(feats, intra_idx):
    """feats [b,c,p,na*nr], intra_idx int32 [na,t] -> [b,c,t,p,na*nr] = feats[b,c,p,intra_idx[a,t],r], the residual r innermost."""
    b, c, p, tot = feats.shape
    na, t = intra_idx.shape
    out = torch.empty(b, c, t, p, tot, dtype=torch.float32, device=feats.device)
    call('eap_so3_intra_group2d_fwd_f32', out, b, c, p, na, _residuals(tot, na), t, _quads(feats), intra_idx, out)
    return out


def so3_intra_group2d_bwd(gout, intra_idx):
    b, c, t, p, tot = gout.shape
    na = intra_idx.shape[0]
    gfeats = torch.empty(b, c, p, tot, dtype=torch.float32, device=gout.device)
    call('eap_so3_intra_group2d_bwd_f32', gfeats, b, c, p, na, _residuals(tot, na), t, _quads(gout), intra_idx, gfeats)
    return gfeats


def so3_inter_group_inv(gy, rows, off, cnt, ent_p, ent_gx, rk, multinv, sigma, nn, identity_anchor=0, anchors=None, coset=None):
    """gy [b,o,p,na] + inverse neighbour lists -> z [b,o,ks,rcap,na] (see include/eap_hip.h).  coset = (order, code) of
    `multinv` (vgtk.so3conv.functional._coset_tables): the permuted clouds' operand is kept coset-major in LDS."""
    b, o, p, na = gy.shape
    rcap = rows.shape[1]
    ks = rk.shape[1]
    z = torch.empty(b, o, ks, rcap, na, dtype=torch.float32, device=gy.device)
    if multinv is not None and coset is not None:
        if na % 8 == 4:          # the kernel's DMA loader copies rows as they are: re-order the anchor axis once (csrc/so3_inter_inv.hip)
            gyc = torch.empty_like(gy)
            call('eap_anchor_reorder_f32', gy, b * o * p, na, gy, coset[0], gyc)
            gy = gyc
        call('eap_so3_inter_group_inv_coset_f32', z, b, o, p, nn, na, ks, rcap, sigma, gy, rows, off, cnt, ent_p, ent_gx, rk, multinv, anchors,
             int(identity_anchor), coset[0], coset[1], z, tag={'flops': 2.0 * b * o * ks * p * nn * na, 'shape': ('group_inv_coset', b, o, p, nn, na,
             ks, rcap)})
        return z
    call('eap_so3_inter_group_inv_f32', z, b, o, p, nn, na, ks, rcap, sigma, gy, rows, off, cnt, ent_p, ent_gx, rk, multinv,
         anchors if multinv is not None else None, int(identity_anchor), z, tag={'flops': 2.0 * b * o * ks * p * nn * na, 'shape': ('group_inv', b, o,
         p, nn, na, ks, rcap)})
    return z


def anchor_reorder(t, order):
    """t [..., na] -> the same with its last axis re-ordered: out[..., i] = t[..., order[i]] (order uint8 [>= na])."""
    t = t.contiguous()
    na = t.shape[-1]
    out = torch.empty_like(t)
    call('eap_anchor_reorder_f32', t, t.numel() // na, na, t, order, out)
    return out


def so3_group_perm_lists2_takes(channels, na, ks, n_support):
    return bool(abi.eap_so3_group_perm_lists2_takes(int(channels), int(na), int(ks), int(n_support)))


def so3_perm_entries(ent_p, ent_gx, code, anchors, identity_anchor, na, n_support, nonident=None):
    """per-entry words of the permuted two-tile kernel (include/eap_hip.h): -> ent_pc int32 [b,per,4,4], ent_gx2 [b,per,4]."""
    b, per = ent_p.shape[0], ent_p[0].numel()
    ent_pc = torch.empty(b, per, 4, 4, dtype=torch.int32, device=ent_p.device)
    ent_gx2 = torch.empty(b, per, 4, dtype=torch.float32, device=ent_p.device)
    anchors = anchors.contiguous() if anchors is not None else None
    call('eap_so3_perm_entries_f32', ent_p, b, per, int(na), int(n_support), ent_p, ent_gx, code, anchors, int(identity_anchor), nonident, ent_pc,
         ent_gx2)
    return ent_pc, ent_gx2


def so3_inter_group_inv_perm2(gy_c, rows, off, cnt, ent_pc, ent_gx2, rk, order, sigma, nn):
    """gy_c [b,o,p,na] (anchor axis coset-major) -> z [b,o,ks,rcap,na] (coset-major), see include/eap_hip.h."""
    b, o, p, na = gy_c.shape
    rcap, ks = rows.shape[1], rk.shape[1]
    z = torch.empty(b, o, ks, rcap, na, dtype=torch.float32, device=gy_c.device)
    call('eap_so3_inter_group_inv_perm2_f32', z, b, o, p, nn, na, ks, rcap, sigma, gy_c, rows, off, cnt, ent_pc, ent_gx2, rk, order, z,
         tag={'flops': 2.0 * b * o * ks * p * nn * na, 'shape': ('group_inv_perm2', b, o, p, nn, na, ks, rcap)})
    return z


def inv_lists_rows(idx, n):
    """idx int32 [b,p,nn] -> rows, off, cnt [b,n] and n_rows [b] (csrc/inv_lists.hip); no host sync."""
    b, p, nn = idx.shape
    dev = idx.device
    counts = torch.empty(b, n, dtype=torch.int32, device=dev)
    rows, off, cnt = torch.empty_like(counts), torch.empty_like(counts), torch.empty_like(counts)
    n_rows = torch.empty(b, dtype=torch.int32, device=dev)
    call('eap_inv_lists_rows', idx, b, p, n, nn, idx, counts, rows, off, cnt, n_rows)
    return rows, off, cnt, n_rows


INV_LISTS_MAX_ROWS = 16384      # target rows per cloud the list builders take (csrc/inv_lists.hip)
GRID_YZ_MAX = 65535             # grid.y / grid.z of a launch (eap_launch_dims_ok): clouds, channel groups, cloud x anchor pairs


def inv_lists(idx, n):
    """idx int32 [b,p,nn] -> (rows, off, cnt, ent): for every one of the n target rows the entry numbers p * nn + slot that name it,
    ascending (eap_inv_lists_rows + eap_inv_lists_entries_ws, the builder whose cost does not grow with the number of rows); what the
    ordered backward of the point gather walks."""
    check_input(idx)
    b, p, nn = idx.shape
    rows, off, cnt, _ = inv_lists_rows(idx, n)
    ent = torch.empty(b, p * nn, dtype=torch.int32, device=idx.device)
    ws = torch.empty((int(abi.eap_inv_lists_entries_workspace(b, p, n, nn)) + 3) // 4, dtype=torch.int32, device=idx.device)
    call('eap_inv_lists_entries_ws', idx, b, p, n, nn, idx, rows, off, ent, ws)
    return rows, off, cnt, ent


def inv_lists_fill(idx, gx, rows, off, rcap):
    """-> ent_p int32 [b,p*nn], ent_gx [b,p*nn,4] for the first rcap rows of every cloud."""
    b, p, nn = idx.shape
    n = rows.shape[1]
    ent_p = torch.empty(b, p * nn, dtype=torch.int32, device=idx.device)
    ent_gx = torch.empty(b, p * nn, 4, dtype=torch.float32, device=idx.device)
    call('eap_inv_lists_fill', idx, b, p, n, nn, int(rcap), idx, gx, rows, off, ent_p, ent_gx)
    return ent_p, ent_gx


def rows_gather(src, rows, rcap):
    """src [b,c,n,na], rows int32 [b,>=rcap] -> [b,c,rcap,na] (zeros for rows < 0)."""
    b, c, n, na = src.shape
    dst = torch.empty(b, c, rcap, na, dtype=torch.float32, device=src.device)
    call('eap_rows_gather_f32', src, b, c, n, na, int(rcap), rows.stride(0), rows, src, dst)
    return dst


def rows_scatter(src, rows, n):
    """src [b,c,rcap,na] -> [b,c,n,na], zero except the rows named by `rows`."""
    b, c, rcap, na = src.shape
    dst = torch.empty(b, c, n, na, dtype=torch.float32, device=src.device)
    call('eap_rows_scatter_f32', src, b, c, n, na, int(rcap), rows.stride(0), rows, src, dst)
    return dst


# ---- block-layer epilogue (csrc/bn_act.hip) -------------------------------------------------------

# ---- the inter conv re-associated over its referenced rows as a dense product (csrc/so3_dense.hip) ----------------------


def so3_dense_supported(p, na, ks, rp, o):
    return bool(abi.eap_so3_dense_supported(int(p), int(na), int(ks), int(rp), int(o)))


DENSE_MAX_ROWS = int(abi.eap_so3_dense_max_rows())        # 1024: the wide tables (32 membership words per point, int64 keys)
DENSE_NARROW_ROWS = 512                                   # up to here the 16-word tables and the int32 key (include/eap_hip.h)


def _dense_wide(memb):
    """the membership table is the 32-word form (the *_wide entries of include/eap_hip.h)"""
    return memb.shape[2] == 32


def so3_dense_member(idx, rows, n_rows, n):
    """Which of a cloud's referenced rows (rows [b, n], n_rows [b]; eap_inv_lists_rows) every neighbour list names:
    -> memb int32 [b,p,16] (bit masks; [b,p,32] when the support has more than 512 rows, so that up to 1024 referenced rows fit),
    flags int32 [b] (non-zero: the cloud cannot take the dense product -- a list names a row twice, or more than min(n, 1024) rows are
    referenced).  No host value is needed: runs before the row count is known, which is why the width follows the SUPPORT size;
    the list head narrows the table once it knows that at most 512 rows are referenced (so3_dense_narrow; DenseGeometry does the same
    for a caller that hands it a wide probe)."""
    b, p, nn = idx.shape
    dev = idx.device
    wide = n > DENSE_NARROW_ROWS
    memb = torch.empty(b, p, 32 if wide else 16, dtype=torch.int32, device=dev)
    flags = torch.empty(b, dtype=torch.int32, device=dev)
    slot_of = torch.empty(b, n, dtype=torch.int32, device=dev)
    call('eap_so3_dense_member_wide' if wide else 'eap_so3_dense_member', idx, b, p, n, nn, min(DENSE_MAX_ROWS if wide else DENSE_NARROW_ROWS, n),
         rows.stride(0), idx, rows, n_rows, slot_of, memb, flags)
    return memb, flags


def so3_dense_narrow(memb, rp):
    """The table the product's geometry is built from at rp row slots: up to 512 the 16-word form -- the first 16 words of a wide probe,
    whose words 16-31 are zero then -- so that keys, point order, masks and step lists are those of the 16-word tables."""
    if _dense_wide(memb) and rp <= DENSE_NARROW_ROWS:
        return memb[:, :, :16].contiguous()
    return memb


# The words the list head's host decisions read (rows, non-identity flag, dense_bad, groups16, norm_ill) from ONE entry
# (csrc/list_probe.hip) instead of about thirty tensor-op launches per layer while the forward waits.  False: the tensor expressions
# (tests, A/B runs); they also remain for pose tensors and norm parameters the entry does not read (so3_dense_probe_takes).
NATIVE_LIST_PROBE = True


def _probe_f32(t, last):
    return (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape[-2:]) == last and t.data_ptr() % 16 == 0
            and t.numel() > 0)


def so3_dense_probe_takes(poses, rot_cloud, norm_w, norm_b):
    """the operands eap_so3_dense_probe reads as they are: float32, contiguous, 16-byte aligned pose tensors [.., 4, 4] (at most two),
    a [b,3,3] per-cloud rotation, float32 norm parameters"""
    return bool(NATIVE_LIST_PROBE and len(poses) <= 2 and all(_probe_f32(t, (4, 4)) for t in poses)
                and (rot_cloud is None or (_probe_f32(rot_cloud, (3, 3)) and rot_cloud.dim() == 3))
                and all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1) for t in (norm_w, norm_b)))


def so3_dense_probe(p, n_rows, nonident, dflags, memb, poses, rot_cloud, norm_w, norm_b, ratio):
    """-> int32 [5] on the device: max n_rows, max nonident (1 without), dense_bad, groups16, norm_ill (include/eap_hip.h); no host sync.
    memb / dflags: so3_dense_member's, or None for a head without the dense probe."""
    b = n_rows.shape[0]
    dev = n_rows.device
    check_input(n_rows, nonident, dflags, memb)
    work = torch.empty(int(abi.eap_so3_dense_probe_workspace(b)), dtype=torch.int32, device=dev)
    out = torch.empty(5, dtype=torch.int32, device=dev)
    rot = [(t, t.numel() // 16) for t in poses] + [(None, 0)] * (2 - len(poses))
    call('eap_so3_dense_probe', n_rows, b, int(p), 0 if memb is None else memb.shape[2], n_rows, nonident, dflags, memb, rot[0][0], rot[0][1],
         rot[1][0], rot[1][1], rot_cloud, norm_w, norm_b, 0 if norm_w is None else norm_w.shape[0], float(ratio), work, out)
    return out


# Occupancy-sorted query points (round 6): a cloud's query points are handed to the dense product sorted by WHICH 16-row groups of the
# referenced rows their lists touch (eap_so3_dense_point_keys), and every 256-column block of the product runs only the k-steps in
# which it generates a weight that is not masked out (eap_so3_dense_steps).  On the bench clouds 31 % (128 -> 512 layer) to 52 %
# (64 -> 128) of the k-steps drop out; skipped steps would have added exact zeros, so the result is bit-equal to running them all
# in the same point order.  The point order is internal: the backward reads dY through it as a column map, the forward's re-ordering
# pass writes Y through it.  SORT_DENSE_POINTS = False: index order and every k-step, as round 5 (A/B runs, tests).
SORT_DENSE_POINTS = True
SKIP_DENSE_STEPS = True


class DenseGeometry:
    """What the dense product needs besides its stored operand, for one neighbourhood of a batch of clouds WITHOUT pose
    rotations: the lane masks of both directions (built on demand from the membership bits), the k-step lists of their column
    blocks, and the two float4 tables of the expanded weight, for the first rp referenced rows of every cloud."""

    def __init__(self, q_xyz, s_xyz, memb, rows, rp, rk, sigma, nn, n_rows=None, row_rot=None, sort=None):
        """row_rot float32 [b, rows.stride(0), 3, 3] (optional): one rotation per row slot applied to the kernel offsets -- the query
        points are ONE rigid part of a posed cloud (include/eap_hip.h: eap_so3_dense_tables_f32)."""
        b, p = memb.shape[:2]
        n = s_xyz.shape[2]
        na, ks, _ = rk.shape
        dev = memb.device
        # up to 512 row slots the 16-word tables and the int32 key, whatever width the probe had: the point order the sort below gives -- and
        # with it the backward's summation order -- is then the same for every support size
        memb = so3_dense_narrow(memb, rp)
        if memb.dtype != torch.int32 or not memb.is_contiguous() or memb.shape[2] not in (16, 32) or int(rp) > 32 * memb.shape[2]:
            raise RuntimeError('DenseGeometry: memb must be a contiguous int32 [b,p,16] (rp <= 512) or [b,p,32] (rp <= 1024)')
        self.wide = _dense_wide(memb)
        self.order = self.pivot_pos = None
        if SORT_DENSE_POINTS if sort is None else sort:
            # (32-word tables: one bit per group g < 64, an int64 key)
            keys = torch.empty(b, p, dtype=torch.int64 if _dense_wide(memb) else torch.int32, device=dev)
            call('eap_so3_dense_point_keys_wide' if _dense_wide(memb) else 'eap_so3_dense_point_keys', memb, b, p, memb, keys)
            order = torch.sort(keys, dim=1, stable=True).indices                               # int64 [b,p]: column j of the product is point order[b, j]
            if NATIVE_NORM_GLUE and q_xyz.dtype == torch.float32 and tuple(q_xyz.shape) == (b, 3, p):
                self.order, memb, q_xyz, self.pivot_pos = so3_dense_point_order(order.contiguous(), memb, q_xyz.contiguous())
            else:
                q_xyz = q_xyz.gather(2, order[:, None, :].expand(b, 3, p)).contiguous()
                memb = memb.gather(1, order[:, :, None].expand(b, p, memb.shape[2])).contiguous()
                self.order = order.to(torch.int32).contiguous()
                self.pivot_pos = (order[0] == 0).to(torch.int32).argmax().to(torch.int32).view(1)   # the column of cloud 0 that is point 0
        self.b, self.p, self.na, self.ks, self.rp, self.nn, self.memb, self.sigma = b, p, na, ks, int(rp), int(nn), memb, float(sigma)
        self.n_rows = n_rows                      # int32 [b] or None: the products stop at every cloud's own rows (include/eap_hip.h)
        p_pad, kd_pad = (p + 31) // 32 * 32, (ks * self.rp + 31) // 32 * 32
        self.centre = torch.empty(b, 4, dtype=torch.float32, device=dev)
        self.pt = torch.empty(b, p_pad, 4, dtype=torch.float32, device=dev)
        self.kr = torch.empty(b, na, kd_pad, 4, dtype=torch.float32, device=dev)
        if row_rot is not None and (row_rot.dtype != torch.float32 or not row_rot.is_contiguous() or row_rot.numel() != b * rows.stride(0) * 9):
            raise RuntimeError('DenseGeometry: row_rot must be a contiguous float32 [b, rows.stride(0), 3, 3]')
        call('eap_so3_dense_tables_f32', memb, b, p, n, na, ks, self.rp, rows.stride(0), sigma, q_xyz, s_xyz, rows, rk, row_rot, self.centre, self.pt,
             self.kr)
        self._masks, self._steps, self._composed = {}, {}, {}

    def mask(self, direction):
        m = self._masks.get(direction)
        if m is None:
            words = int(abi.eap_so3_dense_mask_words(self.b, self.p, self.ks, self.rp, int(direction)))
            m = torch.empty(words, dtype=torch.int64, device=self.memb.device)
            call('eap_so3_dense_masks_wide' if self.wide else 'eap_so3_dense_masks', m, self.b, self.p, self.ks, self.rp, int(direction), self.memb, m)
            self._masks[direction] = m
        return m

    def steps(self, direction):
        """int32 [b, column blocks, k-steps + 1] (count, then the k-steps a column block runs) or None (SKIP_DENSE_STEPS off: every k-step)."""
        if not SKIP_DENSE_STEPS:
            return None
        st = self._steps.get(direction)
        if st is None:
            kd = (self.ks * self.rp + 31) // 32 * 32
            blocks_n = ((self.p if direction else self.ks * self.rp) + 255) // 256
            k_steps = (kd if direction else self.p) // 32
            words = int(abi.eap_so3_dense_steps_words(self.b, self.p, self.ks, self.rp, int(direction)))
            assert words == self.b * blocks_n * (k_steps + 1)
            st = torch.empty(self.b, blocks_n, k_steps + 1, dtype=torch.int32, device=self.memb.device)
            call('eap_so3_dense_steps_wide' if self.wide else 'eap_so3_dense_steps', st, self.b, self.p, self.ks, self.rp, int(direction), 1,
                 self.n_rows, self.mask(direction), st)
            self._steps[direction] = st
        return self._steps[direction]

    def columns(self, col_map=None):
        """The column map of a launch: this geometry's point order composed with the caller's map (int32 [b,p]; negative: padding) -> int32
        [b,p] or None (index order, no map)."""
        if self.order is None:
            return col_map
        if col_map is None:
            return self.order
        hit = self._composed.get(id(col_map))
        if hit is None or hit[0] is not col_map:
            hit = (col_map, col_map.gather(1, self.order.long()).contiguous())
            self._composed = {id(col_map): hit}
        return hit[1]


def so3_dense_split(src, seg=0, seg_pitch=0, shape=None, mapped=False, n_rows=None, rowmax=None, colmap=None):
    """src [b,m,l,na] -> (scale [2,b,na,m], planes): the stored operand of the dense product (two fp16 planes of the scaled rows,
    fragment order).  seg > 0 (with shape = (b, m, l, na)): a row's l elements lie in l / seg segments of seg elements whose
    starts are seg_pitch floats apart (the rows of a GEMM output with padded columns).  mapped: the output's element l is the
    (k, r) pair with dense index l (the forward's operand), n_rows trims every cloud to its own rows.  rowmax int32 [b,m,na]: the
    rows' largest magnitudes (float bit patterns) when the producer already has them -- no pass over src for them (an upper bound will
    do).  colmap int32 [b,l']: the operand is the columns colmap[b, :] of src [b,m,l,na] (negative: a zero column)."""
    b, m, l, na = src.shape if shape is None else shape
    if colmap is not None:
        if colmap.dtype != torch.int32 or not colmap.is_contiguous() or colmap.shape[0] != b:
            raise RuntimeError('so3_dense_split: colmap must be a contiguous int32 [b, columns]')
        seg_pitch, l = l * na, colmap.shape[1]
    scale = torch.empty(2, b, na, m, dtype=torch.float32, device=src.device)      # [0]: [b,na,m]; [1]: the same numbers as [b,m,na]
    planes = torch.empty(b * na * m * ((l + 31) // 32 * 32), dtype=torch.int32, device=src.device)       # 4 bytes per element
    call('eap_so3_dense_split_f32', src, b, m, l, na, int(seg), seg_pitch, int(bool(mapped)), n_rows, rowmax, colmap, src, scale, planes)
    return scale, planes


def dense_pitch(n):
    """Row pitch for a matrix with n columns that the split contraction kernels take as an operand (whole 128-column tiles)."""
    return (n + 127) // 128 * 128


def _dense_executed_flops(geo, o, p, direction):
    """fp16 flops the product kernel executes for this geometry: 6 O A x 256 columns x 32 x (k-steps its column blocks run); without the
    step lists 6 O P A K x (every cloud's own rows rounded to 16).  The counts live on the device; they are read (a host wait) only while
    bench.py attributes launch times, else an upper bound nobody reads is returned."""
    rows = geo.rp * geo.b
    if KERNEL_TIMES is not None:
        st = geo.steps(direction)
        if st is not None and st.shape[2] - 1 <= 1024:      # (csrc/so3_dense.hip KC_LIST_BYTES / 4: longer lists are ignored)
            return 6.0 * o * geo.na * 256 * 32 * float(st[:, :, 0].sum().item())
        if geo.n_rows is not None:
            rows = sum(min((int(r) + 15) & ~15, geo.rp) for r in geo.n_rows.tolist())
    return 6.0 * o * p * geo.na * geo.ks * rows


def _dense_product(direction, geo, b, o, p, ld, scale, planes, out, flops, packed=False):
    """One launch of the product kernel over p columns with the stored operand (scale, planes): direction 0 -> Z [b,o,ks,ld] (the backward;
    row pitch ld), 1 -> Yt [b,na,o,p] (the forward; ld 0).  flops: what the launch stands for algorithmically (bench.py).  packed (direction
    0): every cloud's columns at its own anchor pitch (eap_so3_dense_product_packed_f32: no zero fill behind them).  -> out"""
    tag = {'flops': flops, 'executed_f16_flops': _dense_executed_flops(geo, o, p, direction), 'shape': ('so3_dense', direction, b, o, p, geo.na, geo.ks, geo.rp)}
    if packed:
        if direction != 0 or geo.n_rows is None:
            raise RuntimeError('_dense_product: packed rows are the backward product\'s, with the clouds\' row counts')
        call('eap_so3_dense_product_packed_f32', out, b, o, p, geo.na, geo.ks, geo.rp, ld, geo.sigma, geo.n_rows, planes, scale, geo.pt, geo.kr,
             geo.mask(0), geo.steps(0), out, tag=tag)
        return out
    call('eap_so3_dense_product_steps_f32', out, direction, b, o, p, geo.na, geo.ks, geo.rp, ld, geo.sigma, geo.n_rows, planes, scale, geo.pt, geo.kr,
         geo.mask(direction), geo.steps(direction), out, tag=tag)
    return out


def so3_dense_bwd(gy, geo, ldz=None, colmap=None, rowmax=False, packed=False):
    """gy [b,o,p,na] -> Z [b,o,ks,ldz] whose rows hold [na,rp] (the inverse-list kernel's Z with the anchor axis in front of the row
    axis); ldz >= na*rp (default: equal) pads the rows for the GEMMs that follow -- the padding is NOT written.
    colmap int32 [b,p']: the product runs over the columns colmap[b, :] of gy (the query points of one rigid part: geo is that part's);
    rowmax: row maxima of gy somebody already took from the hint (None: none available; default: ask the hint).
    packed: cloud i's column (a, r) at a * live16[i] + r instead of a * rp + r (dense_live16), nothing zeroed or written behind its na * live16[i]
    live columns."""
    b, o, p, na = gy.shape
    ldz = na * geo.rp if ldz is None else int(ldz)
    colmap = geo.columns(colmap)                                  # (the geometry's own point order: occupancy-sorted)
    scale, planes = so3_dense_split(gy, rowmax=take_rowmax_hint(gy) if rowmax is False else rowmax, colmap=colmap)
    if colmap is not None:
        p = colmap.shape[1]
    z = torch.empty(b, o, geo.ks, ldz, dtype=torch.float32, device=gy.device)
    return _dense_product(0, geo, b, o, p, ldz, scale, planes, z, 2.0 * b * o * p * na * geo.ks * geo.nn, packed=packed)


def so3_dense_gplanes(fc4, W3, geo):
    """The dense forward's stored operand G = W F over the referenced rows, made and written as the product's planes by ONE kernel
    (eap_so3_dense_gplanes_f32): fc4 [b,c,rp,na] the referenced feature rows, W3 [o*ks, c] -> (scale [2,b,na,o], planes), or None when the
    shape is not taken (the caller then runs a GEMM + so3_dense_split).  The plane scale of an output row comes from a bound on its
    magnitude: too large a bound costs dynamic range only."""
    b, c, rp, na = fc4.shape
    o = W3.shape[0] // geo.ks
    if not GPLANES or not abi.eap_so3_dense_gplanes_supported(o, c, na, geo.ks, rp):
        return None
    ft = fc4.permute(0, 3, 2, 1).contiguous()                                       # [b,na,rp,c]
    # |G[o,(k,r),a]| <= max_k sum_c |W[o,c,k]| x max_{c,r} |F[c,r,a]|: two reductions over small tensors (the tighter sum_c |W| max_r |F_c|
    # is a matrix product whose launch path cost more host time than it saved range)
    if NATIVE_NORM_GLUE:
        bound = so3_dense_gplanes_bound(W3, fc4, geo.ks)
    else:
        wsum = W3.abs().sum(1).view(o, geo.ks).amax(1)                                  # [o]
        fm = fc4.abs().amax((1, 2))                                                     # [b,na]
        bound = (fm[:, :, None] * (wsum * 1.0001)[None, None, :]).contiguous()          # [b,na,o]
    scale = torch.empty(2, b, na, o, dtype=torch.float32, device=fc4.device)
    planes = torch.empty(b * na * o * ((geo.ks * rp + 31) // 32 * 32), dtype=torch.int32, device=fc4.device)
    call('eap_so3_dense_gplanes_f32', fc4, b, o, c, na, geo.ks, rp, W3, ft, geo.n_rows, bound, scale, planes,
         tag={'flops': 0.0, 'shape': ('so3_dense_gplanes', b, o, c, na, geo.ks, rp)})      # (write-bound operand preparation: not priced as matrix work)
    return scale, planes


GPLANES = True      # False: G by a GEMM + the split pass, as round 5 (tests)


# ---- the per-channel bookkeeping of the conv + norm nodes, one launch per site (csrc/norm_fold.hip) ----------------------
# The arithmetic between the big kernels of a node (partial sums -> moments -> the affine map and the running statistics; the backward's
# coefficients and bounds; the bound of the forward's operand; what follows the sort of the query points) in the library instead of as
# 10 - 35 tensor expressions per site.  False: the tensor expressions (tests, A/B runs).  They also remain where an all-reduce stands
# between the sums and the coefficients (SyncBatchNorm) and for tensors that are not on the device.
NATIVE_NORM_GLUE = True


def _f64_bits(x):
    """a float64 scalar as the int64 with its bit pattern (the header's vocabulary has no double)"""
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


def norm_fold_train(ps, pq, pivot, count, gamma, beta, eps, momentum, running_mean, running_var):
    """ps, pq float32 [o, parts] (partial sums of y - pivot and its square), pivot a float32 view of o elements, a fixed stride apart ->
    scale, shift float32 [o], mean, invstd float64 [o], a copy of beta and inv_gamma float32 [o]; the running statistics (or None, None) are
    updated in place (vgtk.so3conv.blocks: batch_moments, update_running_stats, affine_from_moments)"""
    check_input(ps, pq, gamma, beta, running_mean, running_var)
    o, parts = ps.shape
    if pivot.dim() != 1 or pivot.shape[0] != o or pivot.dtype != torch.float32 or not pivot.is_cuda:
        raise RuntimeError('norm_fold_train: pivot must be a float32 device vector (any stride) of one element per channel')
    dev = ps.device
    scale, shift, beta_copy, inv_gamma = (torch.empty(o, dtype=torch.float32, device=dev) for _ in range(4))
    mean, invstd = (torch.empty(o, dtype=torch.float64, device=dev) for _ in range(2))
    call('eap_norm_fold_train_f32', ps, o, parts, max(int(pivot.stride(0)), 1), int(count), _f64_bits(eps), _f64_bits(momentum), ps, pq, pivot, gamma,
         beta, running_mean, running_var, scale, shift, mean, invstd, beta_copy, inv_gamma)
    return scale, shift, mean, invstd, beta_copy, inv_gamma


def norm_fold_bwd(pg, pgx, k1, count, beta=None, inv_gamma=None, gmax=None, xmax=None):
    """pg, pgx float32 [o, parts] (partial sums of g and g xhat), k1 = the forward's scale -> (d gamma, d beta, k2, k3) float32 [o]; with beta,
    inv_gamma [o] and the row maxima gmax, xmax [b,o,na] (the dense node) also coef [5,o], bound [b,o,na] and colmax [b,na]"""
    check_input(pg, pgx, k1, beta, inv_gamma, gmax, xmax)
    o, parts = pg.shape
    dev = pg.device
    dgamma, dbeta, k2, k3 = (torch.empty(o, dtype=torch.float32, device=dev) for _ in range(4))
    if gmax is None:
        call('eap_norm_fold_bwd_f32', pg, o, parts, 0, 0, int(count), pg, pgx, k1, None, None, None, None, dgamma, dbeta, k2, k3, None, None, None)
        return dgamma, dbeta, k2, k3
    b, _, na = gmax.shape
    coef = torch.empty(5, o, dtype=torch.float32, device=dev)
    bound = torch.empty(b, o, na, dtype=torch.float32, device=dev)
    colmax = torch.empty(b, na, dtype=torch.float32, device=dev)
    call('eap_norm_fold_bwd_f32', pg, o, parts, b, na, int(count), pg, pgx, k1, beta, inv_gamma, gmax, xmax, dgamma, dbeta, k2, k3, coef, bound, colmax)
    return dgamma, dbeta, k2, k3, coef, bound, colmax


def so3_dense_zbound(colmax, cnt, n_rows, rp, p, ldz):
    """-> words float32 [b, ldz / 4]: the bound on Z's columns, four to a word, from colmax [b,na] and the number of points that list every row
    (cnt int32 [b, >= rp], counted up to n_rows [b] and clamped to 0 .. p)"""
    b, na = colmax.shape
    if cnt.dtype != torch.int32 or n_rows.dtype != torch.int32 or cnt.stride(1) != 1 or not n_rows.is_contiguous():
        raise RuntimeError('so3_dense_zbound: cnt and n_rows must be int32, the rows of cnt contiguous')
    words = torch.empty(b, ldz // 4, dtype=torch.float32, device=colmax.device)
    call('eap_so3_dense_zbound_f32', colmax, b, na, int(rp), int(p), int(ldz), cnt.stride(0), colmax, cnt, n_rows, words)
    return words


# ---- the gradient tail on PACKED Z (vgtk/so3conv/functional.py _backward_dense) ----------------------------------------------------------
# The trimmed backward product ends at every cloud's own live16 = ceil16(min(n_rows, rp)) row slots.  Packed, column (a, r) of a cloud sits at
# a * live16 + r, so its na * live16 live columns are one prefix of the row and the two GEMMs behind the product end there: no zero fill, no
# product over dead columns.  Nothing of this path reads a column past the prefix (the buffers are torch.empty).

def dense_live16(n_rows, rp):
    """row slots of a cloud with n_rows referenced rows in a batch of rp: whole 16-row groups (the library's own arithmetic)"""
    return int(abi.eap_so3_dense_live16(int(n_rows), int(rp)))


def dense_packed_column(a, r, n_rows, rp):
    """the column of (anchor a, row slot r) in a packed row of a cloud with n_rows referenced rows"""
    return int(a) * dense_live16(n_rows, rp) + int(r)


def dense_tail_packed_takes(c, oks, ra, ldz):
    """Do both tail products of a layer with c input channels, Z rows of ra = na * rp columns at pitch ldz and oks = o * ks rows run on the
    packed kernels?  dF = W2 Z on the two-plane 'nn' kernel with one 128-row tile, dW = sum_b Fc_b Z_b^T on the three-plane reduce kernel
    (freshly allocated operands: 16-byte aligned)."""
    return bool(SPLIT_BF16_CONTRACTION and SPLIT_PLANES == 2 and c == 128 and oks % 4 == 0 and ldz % 4 == 0 and
                abi.eap_gemm_bf16x3_nn_f32_supported(c, ldz, oks, None, oks, None, ldz, oks * ldz) and
                abi.eap_gemm_bf16x3_reduce_f32_supported(c, oks, ra, None, ldz, c * ldz, None, ldz, oks * ldz, oks))


def so3_dense_zbound_packed(colmax, cnt, n_rows, rp, p, ldz):
    """so3_dense_zbound for packed Z -> (words float32 [b, ldz / 4], ncols int32 [b] = na * live16 per cloud)"""
    b, na = colmax.shape
    if cnt.dtype != torch.int32 or n_rows.dtype != torch.int32 or cnt.stride(1) != 1 or not n_rows.is_contiguous():
        raise RuntimeError('so3_dense_zbound_packed: cnt and n_rows must be int32, the rows of cnt contiguous')
    words = torch.empty(b, ldz // 4, dtype=torch.float32, device=colmax.device)
    ncols = torch.empty(b, dtype=torch.int32, device=colmax.device)
    call('eap_so3_dense_zbound_packed_f32', colmax, b, na, int(rp), int(p), int(ldz), cnt.stride(0), colmax, cnt, n_rows, words, ncols)
    return words, ncols


def _packed_rows_args(rows, n_rows, who):
    if rows.dtype != torch.int32 or n_rows.dtype != torch.int32 or rows.stride(1) != 1 or not n_rows.is_contiguous():
        raise RuntimeError(f'{who}: rows and n_rows must be int32, the rows of `rows` contiguous')


def rows_gather_packed(src, rows, n_rows, rp, ld):
    """src [b,c,n,na] -> [b,c,ld]: the referenced rows anchor-major and packed, element (a, r) of cloud i at a * live16[i] + r (zeros in the
    slots past n_rows[i] of the last 16-row group; nothing written past na * live16[i])"""
    b, c, n, na = src.shape
    check_input(src)
    _packed_rows_args(rows, n_rows, 'rows_gather_packed')
    dst = torch.empty(b, c, int(ld), dtype=torch.float32, device=src.device)
    call('eap_rows_gather_packed_f32', src, b, c, n, na, int(rp), rows.stride(0), int(ld), rows, n_rows, src, dst)
    return dst


def rows_scatter_packed(src, c, rows, n_rows, rp, n, na):
    """src [b,c_ld,ld] packed as above (its first c rows per cloud) -> [b,c,n,na], zero except the rows named by `rows`"""
    b, c_ld, ld = src.shape
    check_input(src)
    _packed_rows_args(rows, n_rows, 'rows_scatter_packed')
    dst = torch.empty(b, c, n, na, dtype=torch.float32, device=src.device)
    call('eap_rows_scatter_packed_f32', src, b, int(c), c_ld, int(n), int(na), int(rp), rows.stride(0), ld, rows, n_rows, src, dst)
    return dst


def matmul_tail_takes(A, B, out, b_bound):
    """Would matmul_tail run?  The two-plane 'nn' kernel with one 128-row tile, a bound on B's columns, A shared by the batch."""
    ta, tb, M, N, K, lda, sa, ldb, sb, ldc, sc, batch = _product(A, B, out)
    return bool(out.dtype == torch.float32 and SPLIT_BF16_CONTRACTION and SPLIT_PLANES == 2 and b_bound is not None and not ta and not tb and sa == 0 and
                M == 128 and sc == M * ldc and ldc % 4 == 0 and out.data_ptr() % 16 == 0 and _pieces_ok(A, K, lda) and
                abi.eap_gemm_bf16x3_nn_f32_supported(M, N, K, A, lda, B, ldb, sb))


def matmul_tail(A, B, out, ncols, b_bound):
    """out_z[:, :ncols[z]] = A (B_z[:, :ncols[z]]) on the two-plane kernel (eap_gemm_f16x2_splitk_tail_f32; the slab count of `matmul` on the same
    shapes, so the live columns get matmul's bits); the columns past ncols[z] are neither read nor written.  A missing qualification is an
    error (ask matmul_tail_takes)."""
    if not matmul_tail_takes(A, B, out, b_bound):
        raise RuntimeError('matmul_tail: the operands do not qualify for the two-plane tail kernel (matmul_tail_takes)')
    ta, tb, M, N, K, lda, sa, ldb, sb, ldc, sc, batch = _product(A, B, out)
    slabs = int(abi.eap_gemm_f16x2_splitk_slabs(M, N, K, batch, 0)) if (SPLIT_K_ONE_ROW_TILE and K >= 16 * 64) else 1
    abs_a = absmax_rows(A, 1, M, K, lda, 0)
    floats = int(abi.eap_gemm_f16x2_splitk_workspace(M, N, batch, slabs))
    work = torch.empty(max(floats, 4), dtype=torch.float32, device=out.device)
    tag = {'flops': 2.0 * M * N * K * batch, 'shape': ('gemm_tail', 0, 0, M, N, K, batch)}
    call('eap_gemm_f16x2_splitk_tail_f32', out, M, N, K, A, lda, B, ldb, sb, out, ldc, sc, batch, abs_a, b_bound[0], int(b_bound[1]), float(b_bound[2]),
         slabs, work, floats, ncols, tag=tag)


def matmul_reduce_tail_takes(A, B, out):
    """Would matmul_reduce_tail run?  What matmul_reduce_takes_split asks."""
    return matmul_reduce_takes_split(A, B, out)


def matmul_reduce_tail(A, B, out, ncols):
    """out = sum_z A_z[:, :ncols[z]] B_z[:ncols[z], :] on the three-plane kernel (eap_gemm_bf16x3_reduce_tail_f32): nothing past ncols[z] is read."""
    if not matmul_reduce_tail_takes(A, B, out):
        raise RuntimeError('matmul_reduce_tail: the operands do not qualify for the split kernel (matmul_reduce_tail_takes)')
    ta, tb, M, N, K, lda, sa, ldb, sb, ldc, _, batch = _product(A, B, out, reduce=True)
    ws = torch.empty(max(int(abi.eap_gemm_bf16x3_reduce_workspace(M, N, K, batch)), 4), dtype=torch.float32, device=out.device)
    tag = {'flops': 2.0 * M * N * K * batch, 'shape': ('gemm_reduce_tail', 0, 1, M, N, K, batch)}
    call('eap_gemm_bf16x3_reduce_tail_f32', out, M, N, K, A, lda, sa, B, ldb, sb, out, ldc, batch, ncols, ws, tag=tag)


def so3_dense_gplanes_bound(W3, fc4, ks):
    """-> bound float32 [b,na,o] = max_{c,r} |fc4| x (max_k sum_c |W3| x 1.0001), fc4 [b,c,rp,na], W3 [o ks, c]"""
    check_input(W3, fc4)
    b, c, rp, na = fc4.shape
    o = W3.shape[0] // ks
    dev = fc4.device
    fpart = torch.empty(b, c, na, dtype=torch.float32, device=dev)
    wsum = torch.empty(o, dtype=torch.float32, device=dev)
    bound = torch.empty(b, na, o, dtype=torch.float32, device=dev)
    call('eap_so3_dense_gplanes_bound_f32', fc4, b, o, c, na, int(ks), rp, W3, fc4, fpart, wsum, bound)
    return bound


def so3_dense_point_order(order, memb, q_xyz):
    """order int64 [b,p] (the indices of a sort), memb int32 [b,p,16 or 32], q_xyz float32 [b,3,p] -> (order as int32, memb and q_xyz gathered
    through it, pivot_pos int32 [1]: the column of cloud 0 that is point 0)"""
    check_input(order, memb, q_xyz)
    b, p = order.shape
    order32 = torch.empty(b, p, dtype=torch.int32, device=order.device)
    memb_out, xyz_out = torch.empty_like(memb), torch.empty_like(q_xyz)
    pivot_pos = torch.empty(1, dtype=torch.int32, device=order.device)
    call('eap_so3_dense_point_order', order, b, p, memb.shape[2], order, memb, q_xyz, order32, memb_out, xyz_out, pivot_pos)
    return order32, memb_out, xyz_out, pivot_pos


def so3_dense_fwd(g, geo, p, c=0, ldg=None, out=None, col_map=None, operand=None, o=None):
    """g [b,o,ks,ldg] (rows hold [rp,na]: W . F over the referenced rows, F with c channels; ldg >= rp*na, default equal) -> y [b,o,p,na];
    or operand = (scale, planes) of so3_dense_gplanes with g None (then o = the output width).
    (c only prices the launch for bench.py: the reference's grouping einsum + contraction, minus the small GEMM that made g.)
    out [b,o,p_dst,na] with col_map int32 [b,p]: the p columns are the points col_map[b, :] of `out` (negative: padding) -- the launch
    of one rigid part of posed clouds; returns out."""
    yt = _dense_fwd_yt(g, geo, p, c, ldg, operand, o)
    b, na, o = yt.shape[0], geo.na, yt.shape[2]
    if col_map is not None:
        if out is None or col_map.dtype != torch.int32 or tuple(col_map.shape) != (b, p) or not col_map.is_contiguous() or not out.is_contiguous():
            raise RuntimeError('so3_dense_fwd: col_map must be a contiguous int32 [b,p] and come with a contiguous out')
        call('eap_so3_dense_untranspose_map_f32', yt, b, o, p, na, out.shape[2], geo.columns(col_map), yt, out)
        return out
    y = torch.empty(b, o, p, na, dtype=torch.float32, device=yt.device)
    # the re-ordering pass also leaves the channel moments a BatchNorm right behind this layer starts with (its own pass otherwise)
    chunks = (p + 63) // 64
    ps = torch.empty(o, b * chunks, dtype=torch.float32, device=yt.device)
    pq = torch.empty_like(ps)
    if geo.order is not None:                                     # columns in the geometry's point order: written through it
        call('eap_so3_dense_untranspose_map_stats_f32', yt, b, o, p, na, p, geo.order, geo.pivot_pos, yt, y, ps, pq)
    else:
        call('eap_so3_dense_untranspose_f32', yt, b, o, p, na, yt, y, ps, pq)
    leave_stats_hint(y, (ps, pq))
    return y


def _dense_fwd_yt(g, geo, p, c, ldg, operand, o):
    """the forward product alone -> Yt [b,na,o,p] (columns in the geometry's point order)"""
    na = geo.na
    if operand is None:
        b, o = g.shape[:2]
        ldg = geo.rp * na if ldg is None else int(ldg)
        scale, planes = so3_dense_split(g, seg=geo.rp, seg_pitch=ldg, shape=(b, o, geo.ks * geo.rp, na), mapped=True, n_rows=geo.n_rows)
    else:
        scale, planes = operand
        b = geo.b
    yt = torch.empty(b, na, o, p, dtype=torch.float32, device=planes.device)
    return _dense_product(1, geo, b, o, p, 0, scale, planes, yt, 2.0 * b * c * geo.ks * na * (p * geo.nn + o * p - o * geo.rp))


def so3_dense_fwd_bnact(g, geo, p, c, ldg, norm_moments, operand=None, o=None, affine=None, partials=False):
    """The dense forward with the training-mode BatchNorm + leaky_relu behind it applied by the re-ordering pass (the conv + BatchNorm
    node of vgtk/so3conv/functional.py): product -> Yt; statistics pass over Yt; norm_moments(s1, s2, pivot, count) -> (scale, shift, slope)
    per channel (float32 [o]); y' = leaky(scale y + shift) written through the geometry's point order.  affine = (scale, shift, slope)
    instead of norm_moments: an inference-mode norm folded into one per-channel map (FoldedEpilogue), no statistics pass.  partials:
    norm_moments takes the partial sums float32 [o, parts] and the pivot as a float32 view of Yt (eap_norm_fold_train_f32 sums them).  -> y' [b,o,p,na]"""
    yt = _dense_fwd_yt(g, geo, p, c, ldg, operand, o)
    b, na, o = yt.shape[0], geo.na, yt.shape[2]
    if affine is not None:
        bn_scale, bn_shift, slope = affine[0].contiguous(), affine[1].contiguous(), float(affine[2])
    else:
        # moments of every channel over (cloud, anchor, point): Yt is [b na][o][p] for the statistics kernel; the pivot is its own first element
        ps, pq = _partials(yt, b * na, o, p)
        call('eap_bn_stats_f32', yt, b * na, o, p, yt, ps, pq)
        if partials:
            bn_scale, bn_shift, slope = norm_moments(ps, pq, yt[0, 0, :, 0], b * na * p)
        else:
            bn_scale, bn_shift, slope = norm_moments(ps.sum(1, dtype=torch.float64), pq.sum(1, dtype=torch.float64), yt[0, 0, :, 0].double(), b * na * p)
    y = torch.empty(b, o, p, na, dtype=torch.float32, device=yt.device)
    call('eap_so3_dense_untranspose_bnact_f32', yt, b, o, p, na, p, geo.order, yt, bn_scale, bn_shift, slope, y)
    return y


def bn_act_bwd_reduce_fromy(gy, y, beta, inv_gamma, slope, partials=False):
    """gy, y [b,c,p,na] (y = the layer's activated output) -> (sum g, sum g xhat) float64 [c] and the per-row maxima gmax, xmax float32 [b,c,na]
    (csrc/bn_act.hip bn_act_bwd_reduce_fromy_kernel).  partials: the two sums as the kernel leaves them, float32 [c, parts], for norm_fold_bwd."""
    b, c, p, na = y.shape
    n = p * na
    nblk = int(abi.eap_bn_act_fromy_blocks(n, na))
    pg = torch.empty(c, b * nblk, dtype=torch.float32, device=y.device)
    pgx = torch.empty_like(pg)
    gmax = torch.empty(b, c, na, dtype=torch.int32, device=y.device)
    xmax = torch.empty_like(gmax)
    call('eap_bn_act_bwd_reduce_fromy_f32', y, b, c, n, na, slope, gy, y, beta, inv_gamma, pg, pgx, gmax, xmax)
    if partials:
        return pg, pgx, gmax.view(torch.float32), xmax.view(torch.float32)
    return pg.sum(1, dtype=torch.float64), pgx.sum(1, dtype=torch.float64), gmax.view(torch.float32), xmax.view(torch.float32)


def so3_dense_bwd_bn(gy, yact, geo, ldz, coef, rowbound, slope, packed=False):
    """so3_dense_bwd for the gradient BEHIND a training-mode BatchNorm + leaky_relu, formed while it is split into the product's planes
    (eap_so3_dense_split_bn_f32): gy = dL/dy', yact = y' [b,o,p,na], coef float32 [5,o] = k1, k2, k3, beta, 1/gamma, rowbound float32 [b,o,na] >=
    max |gx| of every row.  -> Z as so3_dense_bwd; packed: with every cloud's columns (a, r) at a * live16 + r (see dense_live16), nothing zeroed."""
    b, o, p, na = gy.shape
    ldz = na * geo.rp if ldz is None else int(ldz)
    colmap = geo.columns(None)
    l = p if colmap is None else colmap.shape[1]
    scale = torch.empty(2, b, na, o, dtype=torch.float32, device=gy.device)
    planes = torch.empty(b * na * o * ((l + 31) // 32 * 32), dtype=torch.int32, device=gy.device)
    call('eap_so3_dense_split_bn_f32', gy, b, o, l, p, na, rowbound.view(torch.int32), colmap, gy, yact, coef, slope, scale, planes)
    z = torch.empty(b, o, geo.ks, ldz, dtype=torch.float32, device=gy.device)
    return _dense_product(0, geo, b, o, l, ldz, scale, planes, z, 2.0 * b * o * l * na * geo.ks * geo.nn, packed=packed)


def _partials(x, b, c, n):
    nseg = int(abi.eap_bn_act_segments(n))
    return (torch.empty(c, b * nseg, dtype=torch.float32, device=x.device),
            torch.empty(c, b * nseg, dtype=torch.float32, device=x.device))


# Channel moments of a tensor, handed from the kernel that WROTE it (the dense forward's re-ordering pass) to the BatchNorm behind
# it: one entry, keyed like the row-maximum hint below (tensor object + version + shape)
_STATS_HINT = [None]
STATS_HINTS_TAKEN = 0


def _leave_hint(slot, t, payload):
    slot[0] = (weakref.ref(t), t._version, tuple(t.shape), payload)


def _take_hint(slot, t):
    """the slot's payload if it was left for exactly this tensor (object, version, shape), else None; the slot is empty afterwards"""
    h, slot[0] = slot[0], None
    if not USE_ROWMAX_HINT or h is None or h[0]() is not t or h[1] != t._version or h[2] != tuple(t.shape):
        return None
    return h[3]


def leave_stats_hint(t, partials):
    _leave_hint(_STATS_HINT, t, partials)


def take_stats_hint(t):
    global STATS_HINTS_TAKEN
    partials = _take_hint(_STATS_HINT, t)
    STATS_HINTS_TAKEN += partials is not None
    return partials


def bn_stats(x, b, c, n):
    """-> (sum, sumsq) of x - pivot per channel, float64 [c] (pivot = x[0, c, 0])."""
    hint = take_stats_hint(x)
    if hint is not None and hint[0].shape[0] == c:
        return hint[0].sum(1, dtype=torch.float64), hint[1].sum(1, dtype=torch.float64)
    ps, pq = _partials(x, b, c, n)
    call('eap_bn_stats_f32', x, b, c, n, x, ps, pq)
    return ps.sum(1, dtype=torch.float64), pq.sum(1, dtype=torch.float64)


def bn_act_fwd(x, b, c, n, scale, shift, slope, residual=None):
    y = torch.empty_like(x)
    if residual is None:
        call('eap_bn_act_fwd_f32', x, b, c, n, slope, x, scale, shift, y)
    else:
        call('eap_bn_act_add_fwd_f32', x, b, c, n, slope, x, scale, shift, residual, y)
    return y


def bn_act_bwd_reduce(gy, x, b, c, n, scale, shift, mean, invstd, slope):
    pg, pgx = _partials(x, b, c, n)
    call('eap_bn_act_bwd_reduce_f32', x, b, c, n, slope, gy, x, scale, shift, mean, invstd, pg, pgx)
    return pg.sum(1, dtype=torch.float64), pgx.sum(1, dtype=torch.float64)


# Row maxima of a gradient tensor, handed from the kernel that WROTE it (the BatchNorm backward) to the one that splits it into
# fp16 planes (the dense backward product's stored operand): one entry, keyed on the tensor OBJECT (a weak reference: autograd
# hands the same tensor to the next node when nothing is accumulated into it) and its version counter.  Anything else -- another
# tensor, a tensor modified in between, no entry -- and the split finds the maxima itself.
_ROWMAX_HINT = [None]
USE_ROWMAX_HINT = True        # False: the split always finds its maxima itself (A/B runs, tests)
ROWMAX_HINTS_TAKEN = 0        # how often a hint was accepted (tests)


def leave_rowmax_hint(t, rowmax):
    _leave_hint(_ROWMAX_HINT, t, rowmax)


def take_rowmax_hint(t):
    global ROWMAX_HINTS_TAKEN
    rowmax = _take_hint(_ROWMAX_HINT, t)
    ROWMAX_HINTS_TAKEN += rowmax is not None
    return rowmax


def bn_act_bwd_apply(gy, x, b, c, n, scale, shift, mean, invstd, k2, k3, slope):
    gx = torch.empty_like(x)
    if x.dim() == 4 and x.shape[3] % 4 == 0 and x.shape[3] <= 64 and n == x.shape[2] * x.shape[3] and c % 128 == 0 and gx.data_ptr() % 16 == 0 \
            and gy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0:
        # [b, c, points, anchors] at a width the dense backward product takes: the same pass also leaves the row maxima its
        # stored-operand split needs (csrc/bn_act.hip bn_act_bwd_apply_rowmax_kernel)
        rowmax = torch.empty(b, c, x.shape[3], dtype=torch.int32, device=x.device)
        call('eap_bn_act_bwd_apply_rowmax_f32', x, b, c, n, int(x.shape[3]), slope, gy, x, scale, shift, mean, invstd, k2, k3, gx, rowmax)
        leave_rowmax_hint(gx, rowmax)
        return gx
    call('eap_bn_act_bwd_apply_f32', x, b, c, n, slope, gy, x, scale, shift, mean, invstd, k2, k3, gx)
    return gx


# ---- the first inter conv layer with its norm, without the conv output (csrc/narrow_conv.hip) -------------------
# W [o, ck] and the grouped input x [b, ck, n] in the reference layout, ck = C*K <= 32; the conv output is recomputed in every pass

NARROW_CONV_MAX_CK = 32


def narrow_conv_takes(o, ck, n):
    return 1 <= ck <= NARROW_CONV_MAX_CK and o >= 32 and o % 32 == 0 and n % 4 == 0 and n < (1 << 25)


def _narrow_partials(x, b, o, n):
    nseg = int(abi.eap_narrow_conv_segments(n))
    return (torch.empty(o, b * nseg, dtype=torch.float32, device=x.device),
            torch.empty(o, b * nseg, dtype=torch.float32, device=x.device))


def narrow_conv_stats(W, x, partials=False):
    """-> (sum, sumsq) of y - pivot per channel (float64 [o]) and pivot (float64 [o]) for y = W x, which is not written; partials: the sums as
    the kernel leaves them, float32 [o, parts], and the pivot in float32, for norm_fold_train"""
    check_input(W, x)
    b, ck, n = x.shape
    o = W.shape[0]
    ps, pq = _narrow_partials(x, b, o, n)
    pivot = torch.empty(o, dtype=torch.float32, device=x.device)
    call('eap_narrow_conv_stats_f32', x, b, o, ck, n, W, x, pivot, ps, pq)
    if partials:
        return ps, pq, pivot
    return ps.sum(1, dtype=torch.float64), pq.sum(1, dtype=torch.float64), pivot.double()


def narrow_conv_bnact_fwd(W, x, scale, shift, slope):
    """-> y' [b, o, n] = leaky_relu(scale (W x) + shift)"""
    check_input(W, x, scale, shift)
    b, ck, n = x.shape
    o = W.shape[0]
    y = torch.empty(b, o, n, dtype=torch.float32, device=x.device)
    call('eap_narrow_conv_bnact_fwd_f32', x, b, o, ck, n, slope, W, x, scale, shift, y)
    return y


def narrow_conv_bwd_reduce(gy, x, W, scale, shift, mean, invstd, slope, partials=False):
    """-> sum(g), sum(g xhat) per channel, float64 [o]; partials: as the kernel leaves them, float32 [o, parts], for norm_fold_bwd"""
    check_input(gy, x, W, scale, shift, mean, invstd)
    b, ck, n = x.shape
    o = W.shape[0]
    pg, pgx = _narrow_partials(x, b, o, n)
    call('eap_narrow_conv_bwd_reduce_f32', x, b, o, ck, n, slope, gy, x, W, scale, shift, mean, invstd, pg, pgx)
    if partials:
        return pg, pgx
    return pg.sum(1, dtype=torch.float64), pgx.sum(1, dtype=torch.float64)


def narrow_conv_bwd_dw(gy, x, W, scale, shift, mean, invstd, k2, k3, slope):
    """-> dW [o, ck] = sum gx x^T with gx = scale g - k2 - xhat k3 never written"""
    check_input(gy, x, W, scale, shift, mean, invstd, k2, k3)
    b, ck, n = x.shape
    o = W.shape[0]
    nseg = int(abi.eap_narrow_conv_segments(n))
    partial = torch.empty(b * nseg, o, ck, dtype=torch.float32, device=x.device)
    dW = torch.empty(o, ck, dtype=torch.float32, device=x.device)
    call('eap_narrow_conv_bwd_dw_f32', x, b, o, ck, n, slope, gy, x, W, scale, shift, mean, invstd, k2, k3, partial, dW)
    return dW


# per-cloud statistics over a point subset (the pose heads' batched per-cloud calls); scale .. k3 are [b, c]

def bn_stats_masked(x, b, c, n, na, mask):
    """-> (sum, sumsq) of mask * (x - pivot) per (cloud, channel), float64 [b, c] (pivot = x[0, c, 0])."""
    ps, pq = _partials(x, b, c, n)
    call('eap_bn_stats_masked_f32', x, b, c, n, na, x, mask, ps, pq)
    return ps.view(c, b, -1).sum(2, dtype=torch.float64).t(), pq.view(c, b, -1).sum(2, dtype=torch.float64).t()


def bn_act_cloud_fwd(x, b, c, n, scale, shift, slope):
    y = torch.empty_like(x)
    call('eap_bn_act_cloud_fwd_f32', x, b, c, n, slope, x, scale, shift, y)
    return y


def bn_act_cloud_bwd_reduce(gy, x, b, c, n, scale, shift, mean, invstd, slope):
    pg, pgx = _partials(x, b, c, n)
    call('eap_bn_act_cloud_bwd_reduce_f32', x, b, c, n, slope, gy, x, scale, shift, mean, invstd, pg, pgx)
    return pg.view(c, b, -1).sum(2, dtype=torch.float64).t(), pgx.view(c, b, -1).sum(2, dtype=torch.float64).t()


def bn_act_cloud_bwd_apply(gy, x, b, c, n, na, scale, shift, mean, invstd, k2, k3, mask, slope):
    gx = torch.empty_like(x)
    call('eap_bn_act_cloud_bwd_apply_f32', x, b, c, n, na, slope, gy, x, scale, shift, mean, invstd, k2, k3, mask, gx)
    return gx


# the same layer with the weighted point mean behind it (csrc/heads.hip): x [b,c,p,na] the raw contraction output, w [b,p] point
# weights, inv_den [b]; the activated map and its gradient are never written.  Anchor rows of at most 64 floats take the
# eap_bn_act_cloud_mean_* entries (16 lanes per row), longer ones of at most 256 (the 240 of a `use_2d` map) their _wide twins (a
# wavefront per row)

def _cloud_mean_entries(na):
    return 'eap_bn_act_cloud_mean_wide' if na > 64 else 'eap_bn_act_cloud_mean'


def bn_act_cloud_mean_fwd(x, scale, shift, w, inv_den, slope):
    """-> [b, c, na] = inv_den sum_p w leaky(x scale + shift)"""
    b, c, p, na = x.shape
    out = torch.empty(b, c, na, dtype=torch.float32, device=x.device)
    call(_cloud_mean_entries(na) + '_fwd_f32', x, b, c, p, na, slope, x, scale, shift, w, inv_den, out)
    return out


def bn_act_cloud_mean_bwd_reduce(g, x, scale, shift, mean, invstd, w, inv_den, slope):
    """-> sum(gg), sum(gg xhat) per (cloud, channel), float64 [b, c]"""
    b, c, p, na = x.shape
    parts = int(getattr(abi, _cloud_mean_entries(na) + '_parts')(p))
    pg = torch.empty(b, c, parts, dtype=torch.float32, device=x.device)
    pgx = torch.empty_like(pg)
    call(_cloud_mean_entries(na) + '_bwd_reduce_f32', x, b, c, p, na, slope, g, x, scale, shift, mean, invstd, w, inv_den, pg, pgx)
    return pg.sum(2, dtype=torch.float64), pgx.sum(2, dtype=torch.float64)


def bn_act_cloud_mean_bwd_apply(g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, stat_mask, slope):
    b, c, p, na = x.shape
    gx = torch.empty_like(x)
    call(_cloud_mean_entries(na) + '_bwd_apply_f32', x, b, c, p, na, slope, g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, stat_mask, gx)
    return gx


# SlotAttention's per-point passes (csrc/slot_attention.hip, the eap_slot_attn_* entries): x [b,d,n] channel-major, mean / rstd [b,n] the
# LayerNorm statistics of a point, z = (x - mean) rstd never written; u, gmsum [b,s,d]; c0, gwsum [b,s]; attn, w, gdots [b,s,n]

def _slot_f32(*tensors):
    check_input(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f'slot attention kernels take float32 tensors, not {t.dtype}')


def slot_attn_stats(x, ln_eps):
    """-> mean, rstd [b, n] over the d channels of every point"""
    _slot_f32(x)
    b, d, n = x.shape
    mean = torch.empty(b, n, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    call('eap_slot_attn_stats_f32', x, b, d, n, ln_eps, x, mean, rstd)
    return mean, rstd


def slot_attn_scores_fwd(x, mean, rstd, u, c0, eps):
    """-> attn [b, s, n] = softmax_s(z . u_s + c0_s) + eps"""
    _slot_f32(x, mean, rstd, u, c0)
    (b, d, n), s = x.shape, u.shape[1]
    attn = torch.empty(b, s, n, dtype=torch.float32, device=x.device)
    call('eap_slot_attn_scores_fwd_f32', x, b, s, d, n, eps, x, mean, rstd, u, c0, attn)
    return attn


def slot_attn_pool(x, mean, rstd, w):
    """-> msum [b, s, d] = sum_n w[s,n] z[n], wsum [b, s] = sum_n w[s,n]: float32 partials per 1024 points added in float64"""
    _slot_f32(x, mean, rstd, w)
    (b, d, n), s = x.shape, w.shape[1]
    parts = int(abi.eap_slot_attn_pool_parts(n))
    psum = torch.empty(b, parts, s, d + 1, dtype=torch.float32, device=x.device)
    call('eap_slot_attn_pool_f32', x, b, s, d, n, x, mean, rstd, w, psum)
    total = psum[:, 0] if parts == 1 else psum.sum(1, dtype=torch.float64).float()
    return total[..., :d], total[..., d]


def slot_attn_scores_bwd(x, mean, rstd, attn, gmsum, gwsum, gattn, eps):
    """-> gdots [b, s, n], the gradient of the scores, from the gradients of msum, wsum and (None allowed) attn"""
    _slot_f32(x, mean, rstd, attn, gmsum, gwsum, gattn)
    (b, d, n), s = x.shape, attn.shape[1]
    gdots = torch.empty_like(attn)
    call('eap_slot_attn_scores_bwd_f32', x, b, s, d, n, eps, x, mean, rstd, attn, gmsum, gwsum, gattn, gdots)
    return gdots


def slot_attn_input_grad(x, mean, rstd, rows, vecs):
    """-> gx [b, d, n] of gz[n] = sum_j rows[j,n] vecs[j] through the LayerNorm statistics; rows [b,j,n], vecs [b,j,d], j <= 16"""
    _slot_f32(x, mean, rstd, rows, vecs)
    (b, d, n), j = x.shape, rows.shape[1]
    gx = torch.empty_like(x)
    call('eap_slot_attn_input_grad_f32', x, b, j, d, n, x, mean, rstd, rows, vecs, gx)
    return gx


def so3_intra_conv(feats, W, intra_idx32):
    """Implicit-GEMM intra conv forward: feats [b,c,p,na], W [o, c*nt], intra_idx int32 [na,nt] -> [b,o,p,na]."""
    b, c, p, na = feats.shape
    o, nt = W.shape[0], intra_idx32.shape[1]
    out = torch.empty(b, o, p, na, dtype=torch.float32, device=feats.device)
    split = SPLIT_BF16_CONTRACTION and W.data_ptr() % 16 == 0 and abi.eap_so3_intra_conv_bf16x3_f32_supported(b, o, c, p, na, nt)
    tag = {'flops': 2.0 * b * o * c * nt * p * na, 'shape': ('intra_conv', b, o, c, p, na, nt)}
    if split and SPLIT_PLANES == 2 and feats.data_ptr() % 16 == 0:
        abs_w = absmax_rows(W, 1, o, c * nt, c * nt, 0)
        abs_f = absmax_colgroups(feats, b, c, p * na, p * na, c * p * na, na) if na % 4 == 0 else None
        if abs_w is not None and abs_f is not None:
            call('eap_so3_intra_conv_f16x2_f32', out, b, o, c, p, na, nt, W, feats, intra_idx32, out, abs_w, abs_f, tag=tag)
            return out
    call('eap_so3_intra_conv_bf16x3_f32' if split else 'eap_so3_intra_conv_f32', out, b, o, c, p, na, nt, W, feats, intra_idx32, out, tag=tag)
    return out


def so3_intra_conv2d(feats, W, intra_idx32):
    """so3_intra_conv on the (na, nr) anchor axis of IntraSO3Conv2D, the residual innermost: feats [b,c,p,na*nr], W [o, c*nt], intra_idx
    int32 [na,nt] -> [b,o,p,na*nr] = sum_{c,t} W[o, c*nt + t] feats[b,c,p,intra_idx[a,t],r]."""
    b, c, p, tot = feats.shape
    na, nt = intra_idx32.shape
    o, nr = W.shape[0], _residuals(tot, na)
    out = torch.empty(b, o, p, tot, dtype=torch.float32, device=feats.device)
    split = SPLIT_BF16_CONTRACTION and W.data_ptr() % 16 == 0 and abi.eap_so3_intra_conv2d_split_supported(b, o, c, p, na, nr, nt)
    tag = {'flops': 2.0 * b * o * c * nt * p * tot, 'shape': ('intra_conv2d', b, o, c, p, na, nr, nt)}
    if split and SPLIT_PLANES == 2 and feats.data_ptr() % 16 == 0:
        abs_w = absmax_rows(W, 1, o, c * nt, c * nt, 0)
        abs_f = absmax_colgroups(feats, b, c, p * tot, p * tot, c * p * tot, tot)
        if abs_w is not None and abs_f is not None:
            call('eap_so3_intra_conv2d_f16x2_f32', out, b, o, c, p, na, nr, nt, W, feats, intra_idx32, out, abs_w, abs_f, tag=tag)
            return out
    call('eap_so3_intra_conv2d_bf16x3_f32' if split else 'eap_so3_intra_conv2d_f32', out, b, o, c, p, na, nr, nt, W, feats, intra_idx32, out, tag=tag)
    return out
