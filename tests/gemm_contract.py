"""Harness of the GEMM operand contract (include/eap_hip.h, "dense contraction"): every entry takes leading dimensions,
batch strides and raw base pointers, so

  * a leading dimension may exceed the logical width,
  * nothing outside the logical elements of an input may influence a result,
  * nothing outside [M, N] of each item of C may be written.

A `Case` is one GEMM call on logical operands A [batchA, M, K] and B [batch, K, N] of non-zero integers in [-4, 4] (float32,
seeded).  Every partial product and partial sum is then an integer below 2^24, so the fp32 kernels, the three-bf16-plane split
(h holds the value, m = l = 0) and the two-fp16-plane split (power-of-two scales, l = 0) all owe the EXACT result: the
reference is the float64 product on the CPU (exact for these integers) and the comparison is torch.equal.

`Case.materialise(device)` embeds each operand in a larger buffer by a layout variant

    variant   row pitch                            item stride          base
    tight     width                                rows * width         0
    padded    roundup4(width) + 4 / 8 / 12 (A/B/C) rows * pitch + 20    12 floats
    odd       width + 1 / 3 / 5                    odd                  1 float

(`padded` rounds the width up to whole 16-byte pieces first, so that a ragged width such as K = 4099 still gives the pitch the
16-byte kernels accept; for a width that is a multiple of 4 this is width + 4 / 8 / 12), with a guard band of 256 floats on
both sides.  Everything in an input buffer outside the logical elements is NaN; C, the residual's padding and the workspaces
are pre-filled with one NaN bit pattern.  `Call.check()` requires the logical region of C to equal the reference and every
other word of the C buffer (and the workspace guards) to still hold that pattern, compared as int32 bits.

The module is device-agnostic: tests/test_gemm_contract_host.py runs it against entries emulated in torch on the CPU (with
planted faults, each of which must be caught), tests/test_gpu_gemm_contract.py against the HIP entries.
"""
import functools
import os

import torch

GUARD = 256
FILL_BITS = 0x7FC0BEEF                    # a quiet NaN with a recognisable payload
_PAD = {'A': (4, 1), 'B': (8, 3), 'C': (12, 5), 'R': (12, 5)}       # (padded, odd) extra floats per row
VARIANTS = ('tight', 'padded', 'odd')

RECORDS = []                              # one line per case that ran: entry | kernel | variant | shape | seconds


class ContractViolation(AssertionError):
    pass


def record(call, kernel, seconds):
    c = call.case
    line = (f'{c.entry} | {kernel or "-"} | {c.variant_name()} | ta={c.transA} tb={c.transB} M={c.M} N={c.N} K={c.K} batch={c.batch} '
            f'strideA={"0" if c.shared_a else "item"}{" ep" if c.epilogue else ""}{" res" if c.epilogue == "res" else ""} | {seconds:.4f}')
    RECORDS.append(line)
    print(line)
    log = os.environ.get('EAP_GEMM_CONTRACT_LOG')
    if log:
        with open(log, 'a') as f:
            f.write(line + '\n')
    return line


def _up4(x):
    return (x + 3) // 4 * 4


class Operand:
    """A [nb][rows][cols] matrix stack inside a flat float32 buffer: element (z, r, c) at off + z * stride + r * ld + c.
    `stride` is what the entry is told (0 for an operand shared by the batch)."""

    def __init__(self, role, rows, cols, nb, variant, shared=False, ld=None, stride_extra=0, base_extra=0):
        assert variant in VARIANTS, variant
        self.role, self.rows, self.cols, self.nb, self.variant, self.shared = role, rows, cols, nb, variant, shared
        pad4, podd = _PAD[role]
        if variant == 'tight':
            self.ld, gap, base = cols, 0, 0
        elif variant == 'padded':
            self.ld, gap, base = _up4(cols) + pad4, 20, 12
        else:
            self.ld, gap, base = cols + podd, 20, 1
        if ld is not None:                # a residual takes C's pitch
            self.ld = ld
        self.item_stride = rows * self.ld + gap + stride_extra
        if variant == 'odd' and self.item_stride % 2 == 0:
            self.item_stride += 1
        self.stride = 0 if shared else self.item_stride
        self.off = GUARD + base + base_extra
        self.size = self.off + (nb - 1) * self.item_stride + rows * self.ld + GUARD
        self.buf = None

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return torch.as_strided(buf, (self.nb, self.rows, self.cols), (self.item_stride, self.ld, 1), self.off)

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def tensor(self):
        """a 1-D view that starts at the operand's base (for the dispatcher, which takes tensors)"""
        return self.buf[self.off:]


class Blocked:
    """B stored blocked by 4 (include/eap_hip.h, eap_gemm_f32_xb): element (row r of `brows`, position x) of an item at
    (x >> 2) * brows * 4 + r * 4 + (x & 3); the items `stride` apart."""

    def __init__(self, brows, xlen, nb, variant):
        assert xlen % 4 == 0
        self.brows, self.xlen, self.nb, self.variant, self.shared = brows, xlen, nb, variant, False
        gap, base = (0, 0) if variant == 'tight' else (20, 12)
        self.ld = 4
        self.item_stride = self.stride = brows * xlen + gap
        self.off = GUARD + base
        self.size = self.off + (nb - 1) * self.item_stride + brows * xlen + GUARD
        self.buf = None

    def view(self, buf=None):
        """-> the logical elements as stored: [nb][xlen / 4][brows][4]"""
        buf = self.buf if buf is None else buf
        return torch.as_strided(buf, (self.nb, self.xlen // 4, self.brows, 4), (self.item_stride, self.brows * 4, 4, 1), self.off)

    def logical(self):
        """-> [nb][brows][xlen]"""
        return self.view().permute(0, 2, 1, 3).reshape(self.nb, self.brows, self.xlen)

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off


def _nan_buffer(n):
    return torch.full((n,), float('nan'), dtype=torch.float32)


def fill_buffer(n, device):
    return torch.full((n,), FILL_BITS, dtype=torch.int32, device=device).view(torch.float32)


@functools.lru_cache(maxsize=3)
def problem(M, N, K, batch, batch_a, seed):
    """-> logical A [batch_a, M, K], B [batch, K, N] (float32, non-zero integers in [-4, 4]) and the float64 products
    [batch, M, N].  Cached: the variants of one shape share it; nobody writes to it."""
    gen = torch.Generator().manual_seed(1000003 * seed + 31 * M + 17 * N + 7 * K + batch + 3 * batch_a)

    def draw(*shape):
        v = torch.randint(1, 5, shape, generator=gen)
        return (v * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()

    A, B = draw(batch_a, M, K), draw(batch, K, N)
    return A, B, torch.matmul(A.double(), B.double())


class Case:
    """entry: the C-ABI name (for the record).  variants: one name for all operands, or a dict role -> name.  shared_a: A has one
    item and strideA = 0.  reduce: C[M, N] = the sum over the items.  epilogue: None, 'ep' (scale, shift, slope) or 'res' (+ residual).
    b_blocked: B blocked by 4 (eap_gemm_f32_xb)."""

    def __init__(self, entry, M, N, K, batch, transA=0, transB=0, variants='tight', shared_a=False, reduce=False, epilogue=None,
                 b_blocked=False, seed=0, c_base_extra=0):
        self.entry, self.M, self.N, self.K, self.batch = entry, M, N, K, batch
        self.transA, self.transB = int(transA), int(transB)
        self.variants = dict.fromkeys('ABC', variants) if isinstance(variants, str) else dict(variants)
        self.shared_a, self.reduce, self.epilogue, self.b_blocked, self.seed = shared_a, reduce, epilogue, b_blocked, seed
        self.c_base_extra = c_base_extra           # floats added to C's base offset (a view that starts inside its storage)

    def variant_name(self):
        v = self.variants
        return v['A'] if v['A'] == v['B'] == v['C'] else f"A:{v['A']},B:{v['B']},C:{v['C']}"

    def reference(self):
        A, B, prod = problem(self.M, self.N, self.K, self.batch, 1 if self.shared_a else self.batch, self.seed)
        return A, B, (prod.sum(0, keepdim=True) if self.reduce else prod)

    def epilogue_terms(self):
        gen = torch.Generator().manual_seed(77 + self.seed + self.M)
        scale = torch.pow(2.0, torch.randint(-2, 3, (self.M,), generator=gen).float()) * (torch.randint(0, 2, (self.M,), generator=gen) * 2 - 1).float()
        shift = torch.randint(-8, 9, (self.M,), generator=gen).float()
        res = torch.randint(-4, 5, (self.batch, self.M, self.N), generator=gen).float()
        return scale, shift, 0.25, res

    def materialise(self, device):
        return Call(self, device)


class Call:
    def __init__(self, case, device):
        self.case, self.device = case, device
        c = case
        A, B, ref = c.reference()
        self.A = Operand('A', *((c.K, c.M) if c.transA else (c.M, c.K)), A.shape[0], c.variants['A'], shared=c.shared_a)
        buf = _nan_buffer(self.A.size)
        self.A.view(buf).copy_(A.transpose(1, 2) if c.transA else A)
        self.A.buf = buf.to(device)
        if c.b_blocked:
            self.B = Blocked(c.N if c.transB else c.K, c.K if c.transB else c.N, c.batch, c.variants['B'])
            buf = _nan_buffer(self.B.size)
            lay = B.transpose(1, 2) if c.transB else B                      # [batch][brows][xlen]
            self.B.view(buf).copy_(lay.reshape(c.batch, self.B.brows, self.B.xlen // 4, 4).permute(0, 2, 1, 3))
        else:
            self.B = Operand('B', *((c.N, c.K) if c.transB else (c.K, c.N)), c.batch, c.variants['B'])
            buf = _nan_buffer(self.B.size)
            self.B.view(buf).copy_(B.transpose(1, 2) if c.transB else B)
        self.B.buf = buf.to(device)
        self.C = Operand('C', c.M, c.N, 1 if c.reduce else c.batch, c.variants['C'], base_extra=c.c_base_extra)
        self.C.buf = fill_buffer(self.C.size, device)
        self.expected = ref
        self.scale = self.shift = self.R = None
        self.slope = 0.0
        if c.epilogue:
            scale, shift, self.slope, res = c.epilogue_terms()
            v = ref * scale.double()[None, :, None] + shift.double()[None, :, None]
            v = torch.where(v >= 0, v, v * self.slope)
            self.scale, self.shift = scale.to(device), shift.to(device)
            if c.epilogue == 'res':
                # laid out like C (its pitch is ldc), its own item stride, its padding holds the fill pattern
                self.R = Operand('R', c.M, c.N, c.batch, c.variants['C'], ld=self.C.ld, stride_extra=0 if c.variants['C'] == 'tight' else 8)
                buf = fill_buffer(self.R.size, 'cpu')
                self.R.view(buf).copy_(res)
                self.R.buf = buf.to(device)
                v = v + res.double()
            self.expected = v
        self._ws = []

    def workspace(self, words):
        """-> a float32 tensor of `words` words (16-byte aligned) between two guard bands, everything pre-filled"""
        buf = fill_buffer(GUARD + max(int(words), 1) + GUARD, self.device)
        self._ws.append((buf, int(words)))
        return buf[GUARD:GUARD + max(int(words), 1)]

    def check(self):
        """the logical region of C equals the reference; every other word of the C buffer and of the workspace guards still holds
        the fill pattern"""
        c = self.case
        got = self.C.view()
        want = self.expected.float()
        assert torch.equal(want.double(), self.expected), 'harness: the reference is not representable in float32'
        want = want.to(self.device)
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            z, r, col = [int(x) for x in bad.nonzero()[0]]
            raise ContractViolation(f'{c.entry} [{c.variant_name()}] C differs from the exact product at {int(bad.sum())} of {bad.numel()} elements, '
                                    f'first at item {z} row {r} col {col}: got {got[z, r, col].item()!r}, want {want[z, r, col].item()!r}')
        rest = self.C.buf.view(torch.int32).clone()
        self.C.view(rest).fill_(FILL_BITS)
        if not bool((rest == FILL_BITS).all()):
            at = int((rest != FILL_BITS).nonzero()[0])
            rel = at - self.C.off
            z, rem = divmod(rel, self.C.item_stride) if rel >= 0 else (-1, rel)
            raise ContractViolation(f'{c.entry} [{c.variant_name()}] wrote outside [M, N] of C: {int((rest != FILL_BITS).sum())} words, first at '
                                    f'buffer word {at} (item {z}, row {rem // self.C.ld}, col {rem % self.C.ld}; M={c.M} N={c.N} ldc={self.C.ld})')
        for buf, words in self._ws:
            w = buf.view(torch.int32)
            if not bool((w[:GUARD] == FILL_BITS).all() and (w[GUARD + max(words, 1):] == FILL_BITS).all()):
                raise ContractViolation(f'{c.entry} [{c.variant_name()}] wrote outside its workspace of {words} words')
        if self.R is not None:
            rest = self.R.buf.view(torch.int32).clone()
            self.R.view(rest).fill_(FILL_BITS)
            assert bool((rest == FILL_BITS).all()), 'the residual was written to'


def absmax_reference(op, grp=None):
    """the words eap_absmax_rows_f32 (grp None: [nb, rows]) / eap_absmax_colgroups_f32 ([nb, cols // grp]) owe for an operand:
    bit patterns of the largest magnitudes of the LOGICAL elements"""
    v = op.view().abs()
    m = v.amax(2) if grp is None else v.amax(1).view(op.nb, op.cols // grp, grp).amax(2)
    return m.contiguous().view(torch.int32)


def check_absmax(words, op, grp=None, what='absmax'):
    want = absmax_reference(op, grp)
    if not torch.equal(words.view(torch.int32).reshape(want.shape), want):
        raise ContractViolation(f'{what}: the magnitudes differ from those of the logical elements (padding read?)')
