// csrc/device_prims.h -- the device-side primitives the gfx950 kernels share: vector types, the global -> LDS DMA
// loads, the power-of-two row scale of the two-fp16-plane products, the XCD block remap.  One definition each.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- global -> LDS DMA ----------------------------------------------------------------------------------------------
// One wave-wide load whose data goes straight to LDS: lane l's 16 (glds16*) or 4 (glds4*) bytes land at
// lds_dst + 16*l / 4*l, lds_dst wave-uniform (it travels in M0).  glds16 / glds4 take a 64-bit address per lane;
// the `s` forms take a wave-uniform 64-bit base in SGPRs and a 32-bit byte offset per lane: no 64-bit VALU add per request.
// Inline asm on purpose, not the builtin: hipcc tracks the builtin as an LDS store and drains vmcnt before every
// later ds_read, which would serialise the next chunk's rows behind this chunk's operand reads; an asm load is
// invisible to its waitcnt bookkeeping.  So THE CALLER OWNS THE WAIT: dma_wait() (or a counted s_waitcnt of its own)
// before the barrier that publishes the data.  M0 is saved and restored inside the one statement, so the compiler's
// own uses of M0 around it are undisturbed; the s_nop covers the M0 write -> DMA load hazard.
// A change to one of these sequences is a change to every kernel that stages through LDS: re-run their tests.

// LDS byte address of a __shared__ object (what M0 takes for the LDS-DMA loads)
__device__ inline unsigned lds_addr(const void *ptr) {
    return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)ptr;
}
__device__ inline void glds16(const void *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ inline void glds16s(const void *sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ inline void glds4(const void *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ inline void glds4s(const void *sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ inline void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- two-fp16-plane products ----------------------------------------------------------------------------------------
// The scale 2^(14 - e) of a row (or tensor) whose largest magnitude, or a bound on it, is v in [2^e, 2^(e+1)); 1 for 0,
// inf, nan.  The split GEMMs (csrc/gemm_bf16x3.hip, PL = 2) and the dense product (csrc/so3_dense.hip) must agree on it
// to the bit: their error bounds assume the same rule.
__device__ __forceinline__ float pow2_scale(float v) {
    const unsigned b = __float_as_uint(v) & 0x7fffffffu;
    const int e = (int)(b >> 23) - 127;
    if (b == 0u || e == 128) return 1.0f;
    const int se = max(-120, min(120, 14 - max(e, -126)));
    return __uint_as_float((unsigned)(se + 127) << 23);
}

// ---- uniform base + per-lane byte offset ----------------------------------------------------------------------------
// uniform 64-bit base + 32-bit byte offset per lane: hipcc then uses the SGPR-base addressing form and no 64-bit
// vector arithmetic (the first version of csrc/zpconv_bwd.hip spent 260 v_lshl_add_u64 per unit and, under the register
// pressure they caused, waited for every single load)
template <typename V>
__device__ __forceinline__ V ld_off(const void *ubase, unsigned voff) {
    return *reinterpret_cast<const V *>(reinterpret_cast<const char *>(ubase) + voff);
}
template <typename V>
__device__ __forceinline__ void st_off(void *ubase, unsigned voff, V v) {
    *reinterpret_cast<V *>(reinterpret_cast<char *>(ubase) + voff) = v;
}

// ---- block -> XCD ---------------------------------------------------------------------------------------------------
// Consecutive points must land on the SAME XCD: each (channel, k) output row of a point is only
// 4*na bytes, so neighbouring points share cache lines; with the default round-robin dispatch
// (block b -> XCD b % 8) they would sit half-written in eight different L2s and reach HBM as
// partial lines (measured: X written at ~1 TB/s).  Remap so that XCD x gets a contiguous range
// of points (bijective for any P).
__device__ __forceinline__ int xcd_point(int bx, int p) {
    const int q = p >> 3, r = p & 7, xcd = bx & 7, j = bx >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
#endif
