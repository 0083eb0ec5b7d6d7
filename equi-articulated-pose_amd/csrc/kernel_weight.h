// csrc/kernel_weight.h -- the interpolation weight of the inter convolution's grouping, as the four fp32-MFMA kernels
// evaluate it (csrc/so3_inter_lists.hip, so3_inter_lists2.hip, so3_inter_inv.hip, so3_inter_mfma.hip).  One definition.
//
//   w(p,a,k,n) = relu(1 - |g(p,n) - A_a kappa_k|^2 / sigma) = clamp(base_e + kc + g . k')
//     base_e = 1 - |g|^2/sigma     once per entry (entry_base)
//     k'     = 2 A_a kappa_k / sigma,   kc = -|kappa_k|^2/sigma     per-lane constants (load), lane <-> kernel point k
//
// The weights are the MFMA's B operand and never exist in memory: lane (k = l & 31, e = l >> 5) evaluates its own in
// registers right before the matrix instruction that consumes it.  On this part the fp32 MFMA and the vector ALU share
// their multipliers (vector fp32 peak = matrix fp32 peak; tools/microbench/mfma_waves.hip: every VALU instruction between
// MFMAs costs its 4 cycles of matrix time at ANY occupancy -- the first k-loop spent 150 VALU instructions per 16 MFMAs
// and sat at 95 % of the resulting 63 % ceiling), so the weight is evaluated with as few VALU instructions as it takes:
// everything goes through packed operations on two anchors at a time -- the per-entry term joins kc in one add, then
// three packed FMAs, and the relu is the clamp modifier of the last one (weights never exceed 1): 2 instructions per
// weight instead of 5.  The last FMA is inline assembly for the sake of that modifier.  Its s_nop 1: a register written
// by a VALU instruction needs two wait states before an MFMA reads it as an operand, and hipcc pads only the instructions
// it emits itself, so the wait states of a write inside an asm string have to be inside the string.
// kernel_weight_exact (csrc/so3_inter.hip) and the weight tables of csrc/so3_dense.hip are deliberately other evaluations.
#pragma once
#include "device_prims.h"
#ifdef __HIPCC__

namespace kernel_weight {

// what kc of a kernel-point column past ks, and the per-entry term of a dead entry, are set to: the weight clamps to 0
constexpr float DEAD = -1e30f;
// relative tolerance of Constants::uniform()
constexpr float UNIFORM_TOL = 1e-6f;

// the per-entry term
__device__ __forceinline__ float entry_base(const float4 g, float inv_sigma) {
    return 1.0f - inv_sigma * (g.x * g.x + g.y * g.y + g.z * g.z);
}

// the per-lane constants of a wave's APW anchors (k = lane & 31), packed in anchor pairs
template <int APW>
struct Constants {
    f32x2 kx[APW / 2], ky[APW / 2], kz[APW / 2], kc[APW / 2];

    // anchor_of(ai): memory index of the wave's ai-th anchor (always a valid one)
    template <typename AnchorOf>
    __device__ __forceinline__ void load(const float *rk, int ks, int lk, float inv_sigma, AnchorOf anchor_of) {
        const int lkc = min(lk, ks - 1);
#pragma unroll
        for (int ai = 0; ai < APW; ++ai) {
            const float *r3 = rk + ((size_t)anchor_of(ai) * ks + lkc) * 3;
            const float x = r3[0], y = r3[1], z = r3[2];
            kx[ai >> 1][ai & 1] = 2.f * inv_sigma * x;
            ky[ai >> 1][ai & 1] = 2.f * inv_sigma * y;
            kz[ai >> 1][ai & 1] = 2.f * inv_sigma * z;
            kc[ai >> 1][ai & 1] = lk < ks ? -inv_sigma * (x * x + y * y + z * z) : DEAD;
        }
    }

    // Kernel points rotated by the anchors all have the norm of the unrotated point, so kc is normally the same for the
    // wave's anchors (to rounding): it then joins the per-entry term with ONE plain add per k-step instead of a packed one
    // per anchor pair (a packed instruction costs the matrix pipe twice a plain one, tools/microbench/mfma_riders.hip):
    // eval<true>.  Arbitrary rk tables (norms that differ) keep the general form.  Wave-uniform.
    __device__ __forceinline__ bool uniform() const {
        const float kcl = kc[0][0];
        static_assert(APW == 4, "written for two anchor pairs");
        return __all(fabsf(kc[0][1] - kcl) <= UNIFORM_TOL * fabsf(kcl) && fabsf(kc[1][0] - kcl) <= UNIFORM_TOL * fabsf(kcl) &&
                     fabsf(kc[1][1] - kcl) <= UNIFORM_TOL * fabsf(kcl)) != 0;
    }

    // the weights of one entry (offset vector g, per-entry term base) for the wave's anchors; KCU: uniform() held
    template <bool KCU>
    __device__ __forceinline__ void eval(const float4 g, float base, f32x2 (&wv)[APW / 2]) const {
        const float bkc = base + kc[0][0];
#pragma unroll
        for (int j = 0; j < APW / 2; ++j) {
            f32x2 x = __builtin_elementwise_fma((f32x2){g.x, g.x}, kx[j], KCU ? (f32x2){bkc, bkc} : kc[j] + (f32x2){base, base});
            x = __builtin_elementwise_fma((f32x2){g.y, g.y}, ky[j], x);
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] clamp\n\ts_nop 1" : "=v"(wv[j]) : "v"((f32x2){g.z, g.w}), "v"(kz[j]), "v"(x));
        }
    }
};

}  // namespace kernel_weight
#endif
