// csrc/heads.hip -- the anchor-axis reductions of the heads that read the backbone's [B,C,N,A] feature map
// (SURVEY.md section 8(f) rows 2 and 3): one pass over the map instead of the reference's 3-4 torch passes.
//
//   anchor attention pooling   InvPPOutBlockOurs.forward, SPConvNets/utils/base_so3conv.py:L905-912 (InvPPOutBlock2DOurs, L921-1008):
//        conf[b,n,a] = softmax_a(logit[b,n,a] * T);   out[b,c,n] = sum_a x[b,c,n,a] conf[b,n,a]
//   slot-masked point mean     the pose head's masked averages over the points of every slot at once
//        (SPConvNets/models/model_utils.py:L470-472 + L484 / L549-552, called once per slot by
//        ...pn_38_multi_stage.py:L695-1015):   out[b,s,c,a] = sum_n m[b,s,n] x[b,c,n,a] / max(sum_n m[b,s,n], 1e-8)
//   masked point max           the pose head's 'max' pooling on a point subset (model_utils.py:L79-80, L470-484)
//   norm + act + point mean    the last unary layer of InvOutBlockOursWithMask and the point average behind it
//        (SPConvNets/utils/base_so3conv.py:L1076-1107):   out[b,c,a] = inv_den[b] sum_p w[b,p] leaky(x[b,c,p,a] scale[b,c] + shift[b,c])
//
// Mapping: Q lanes of a wavefront hold one point's anchor row, one 16-byte quad per lane, so a wave takes G = 64 / Q consecutive
// points with one load instruction and a 256-thread block walks CHAINS = 4 G point chains.  Every kernel is written once and
// compiled for both Q:
//   Q = 16   rows of at most 64 floats (15 quads of a 60-anchor row + one idle lane): 4 points per wave, 16 chains per block, a row
//            reduction is 4 shuffle steps.  The entries without a suffix.
//   Q = 64   rows of at most 256 floats (the 60 x 4 = 240 anchors of a `use_2d` map, lanes 60-63 idle): one point per wave, 4
//            chains per block, 6 shuffle steps.  The _wide entries.  What a wave reads per POINT (a mask weight, a channel's gradient)
//            has a wave-uniform address here and comes through the scalar cache.
// HBM-bound: x is read once forward; the backward reads x or g once and writes dx once.  No atomics; every sum has a fixed order
// (a chain ascends over its points, the chains are folded through LDS in chain order), so results are bit-identical run to run.
#include <initializer_list>

#include "common.h"

namespace {

// the wave's index in its block as a value the compiler knows to be the same in every lane
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// a thread's place in the mapping: its quad of the row, and the point chain it walks (first point `chain` = wave * G + lane / Q, step
// CHAINS; also its row of the LDS partials).  At Q = 64 the chain is the wave, taken through wave_index() so that what is read per point
// becomes scalar loads; at Q = 16 it differs within the wave, and the uniform wave index only cost time there (2 % of the masked max
// forward at 4 x 256 x 2048 x 60, profiles/heads_one_source.txt)
template <int Q>
struct Lanes {
    static_assert(Q == 16 || Q == 64, "a row takes a quarter of a wavefront or all of it");
    static constexpr int G = 64 / Q, CHAINS = 4 * G;
    // loop trips a chain keeps in flight where the trips are independent: at Q = 64 what a trip reads per point sits in scalar registers
    // and four trips cost little; at Q = 16 it is per lane, and unrolling would pay for the loads in flight with occupancy
    static constexpr int ROWS = Q == 64 ? 4 : 1;
    int quad, chain;
    __device__ Lanes() : quad(threadIdx.x % Q), chain(Q == 64 ? wave_index() : (int)(threadIdx.x / Q)) {}
};

// over the Q lanes of a row, widest step first
template <int Q>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int d = Q / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
template <int Q>
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
    for (int d = Q / 2; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

// block = CHAINS consecutive points of one cloud; every row's lanes walk all channels of their point.  A point past n re-reads point
// n - 1 and an idle lane the last quad; neither stores.
template <int Q, bool BWD>
__global__ __launch_bounds__(256) void anchor_attn_pool_kernel(int c, int n, int na, float temperature,
                                                              const float *__restrict__ x, const float *__restrict__ logits,
                                                              const float *__restrict__ g, float *__restrict__ out,
                                                              float *__restrict__ conf_out, float *__restrict__ dx,
                                                              float *__restrict__ dlogits) {
    const Lanes<Q> ln;
    const int bi = blockIdx.y, pt = blockIdx.x * ln.CHAINS + ln.chain, nq = na >> 2;
    if constexpr (Q == 64) {
        if (pt >= n) return;                                 // the whole wave: no block-wide barrier below
    }
    const bool live = ln.quad < nq, on = pt < n && live;
    const size_t at = (size_t)min(pt, n - 1) * na + 4 * min(ln.quad, nq - 1), row = (size_t)bi * n * na + at;
    // softmax over the anchors of this point
    float4 l = *reinterpret_cast<const float4 *>(logits + row);
    l.x *= temperature; l.y *= temperature; l.z *= temperature; l.w *= temperature;
    if (!live) l = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    const float m = row_max<Q>(fmaxf(fmaxf(l.x, l.y), fmaxf(l.z, l.w)));
    float4 e = make_float4(__expf(l.x - m), __expf(l.y - m), __expf(l.z - m), __expf(l.w - m));
    if (!live) e = make_float4(0.f, 0.f, 0.f, 0.f);
    const float inv = 1.0f / row_sum<Q>(e.x + e.y + e.z + e.w);
    const float4 cf = make_float4(e.x * inv, e.y * inv, e.z * inv, e.w * inv);
    if (!BWD && on && conf_out) *reinterpret_cast<float4 *>(conf_out + row) = cf;
    const size_t cs = (size_t)n * na;                        // channel stride of x
    const float *xp = x + (size_t)bi * c * cs + at;
    if (!BWD) {
        float *op = out + (size_t)bi * c * n + min(pt, n - 1);
        auto dot = [&](const float4 v) { return live ? v.x * cf.x + v.y * cf.y + v.z * cf.z + v.w * cf.w : 0.f; };
        int ci = 0;
        for (; ci + 4 <= c; ci += 4) {                       // 4 channel rows in flight; every channel's sum in the same order
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(xp + (size_t)(ci + u) * cs);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float s = row_sum<Q>(dot(v[u]));
                if (on && ln.quad == 0) op[(size_t)(ci + u) * n] = s;
            }
        }
        for (; ci < c; ++ci) {
            const float s = row_sum<Q>(dot(*reinterpret_cast<const float4 *>(xp + (size_t)ci * cs)));
            if (on && ln.quad == 0) op[(size_t)ci * n] = s;
        }
    } else {
        const float *gp = g + (size_t)bi * c * n + min(pt, n - 1);
        float *dxp = dx + (size_t)bi * c * cs + at;
        float4 dc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll Lanes<Q>::ROWS
        for (int ci = 0; ci < c; ++ci) {
            const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)ci * cs);
            const float gv = gp[(size_t)ci * n];
            dc.x = fmaf(gv, v.x, dc.x); dc.y = fmaf(gv, v.y, dc.y); dc.z = fmaf(gv, v.z, dc.z); dc.w = fmaf(gv, v.w, dc.w);
            if (on) *reinterpret_cast<float4 *>(dxp + (size_t)ci * cs) = make_float4(gv * cf.x, gv * cf.y, gv * cf.z, gv * cf.w);
        }
        // softmax backward: dlogit = T conf (dconf - sum_a conf dconf)
        const float s = row_sum<Q>(live ? cf.x * dc.x + cf.y * dc.y + cf.z * dc.z + cf.w * dc.w : 0.f);
        if (on) *reinterpret_cast<float4 *>(dlogits + row) = make_float4(temperature * cf.x * (dc.x - s), temperature * cf.y * (dc.y - s),
                                                                         temperature * cf.z * (dc.z - s), temperature * cf.w * (dc.w - s));
    }
}

constexpr int MAXS = 8;     // slots per launch

// Both slot kernels are compiled for NS = 1, 2, 4 and 8 slots and run at the smallest NS >= ns.  A point's NS weights are fetched
// unconditionally (slots past ns re-read slot ns - 1), so the loads of an iteration go out together; a load behind an `if (s < ns)`
// would wait for the one before it.

// forward: block = (channel, cloud); a chain takes its points in ascending order, one row per iteration; per slot one float4
// accumulator per lane (those past ns gather values nobody reads); the chains' partials are folded through LDS in chain order
template <int Q, int NS>
__global__ __launch_bounds__(256) void slot_mean_fwd_kernel(int c, int n, int na, int ns, const float *__restrict__ x,
                                                            const float *__restrict__ m, const float *__restrict__ inv_den,
                                                            float *__restrict__ out) {
    constexpr int CHAINS = Lanes<Q>::CHAINS;
    __shared__ float4 s_part[NS][CHAINS][Q];                  // [slot][chain][quad], 4 KB per slot
    const Lanes<Q> ln;
    const int ci = blockIdx.x, bi = blockIdx.y, nq = na >> 2;
    float4 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *xp = x + ((size_t)bi * c + ci) * n * na + 4 * min(ln.quad, nq - 1);
    const float *mp = m + (size_t)bi * ns * n;
#pragma unroll Lanes<Q>::ROWS
    for (int p0 = ln.chain; p0 < n; p0 += CHAINS) {
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p0 * na);
        float w[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) w[s] = mp[(size_t)min(s, ns - 1) * n + p0];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            acc[s].x = fmaf(w[s], v.x, acc[s].x); acc[s].y = fmaf(w[s], v.y, acc[s].y);
            acc[s].z = fmaf(w[s], v.z, acc[s].z); acc[s].w = fmaf(w[s], v.w, acc[s].w);
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (s < ns) s_part[s][ln.chain][ln.quad] = acc[s];
    __syncthreads();
    for (int e = threadIdx.x; e < ns * nq; e += 256) {
        const int s = e / nq, q = e - s * nq;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < CHAINS; ++j) { const float4 u = s_part[s][j][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float d = inv_den[(size_t)bi * ns + s];
        *reinterpret_cast<float4 *>(out + (((size_t)bi * ns + s) * c + ci) * na + 4 * q) = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
    }
}

// backward w.r.t. x: dx[b,c,n,a] = sum_s g[b,s,c,a] m[b,s,n] inv_den[b,s]; a slot past ns is the term 0 * 0, which leaves the sum as it is
template <int Q, int NS>
__global__ __launch_bounds__(256) void slot_mean_bwd_kernel(int c, int n, int na, int ns, const float *__restrict__ g,
                                                            const float *__restrict__ m, const float *__restrict__ inv_den,
                                                            float *__restrict__ dx) {
    const Lanes<Q> ln;
    const int ci = blockIdx.x, bi = blockIdx.y, nq = na >> 2;
    if (ln.quad >= nq) return;
    float4 gv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        gv[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < ns) {
            const float d = inv_den[(size_t)bi * ns + s];
            const float4 t = *reinterpret_cast<const float4 *>(g + (((size_t)bi * ns + s) * c + ci) * na + 4 * ln.quad);
            gv[s] = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
        }
    }
    float *dp = dx + ((size_t)bi * c + ci) * n * na + 4 * ln.quad;
    const float *mp = m + (size_t)bi * ns * n;
#pragma unroll Lanes<Q>::ROWS
    for (int p0 = ln.chain; p0 < n; p0 += Lanes<Q>::CHAINS) {
        float w[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float ws = mp[(size_t)min(s, ns - 1) * n + p0];
            w[s] = s < ns ? ws : 0.f;
        }
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            t.x = fmaf(w[s], gv[s].x, t.x); t.y = fmaf(w[s], gv[s].y, t.y); t.z = fmaf(w[s], gv[s].z, t.z); t.w = fmaf(w[s], gv[s].w, t.w);
        }
        *reinterpret_cast<float4 *>(dp + (size_t)p0 * na) = t;
    }
}

// masked max over the points, the pose head's 'max' pooling on a point subset (`(x * mask).max(2)`: SO3OutBlockRWithMask /
// SO3OutBlockRTWithMaskSep with pooling_method = 'max', SPConvNets/models/model_utils.py:L79-80, L470-484): out[b,c,a] = max_p
// mask[b,p] * x[b,c,p,a] and the point that attains it (the lowest index among equals: deterministic).  One pass over x.
// A product that is NaN (a NaN or mask 0 times an infinity in x, whatever the mask) is the result, as torch's max gives it, and arg the
// lowest point with such a product: a diverged map must not pool to a finite number.  -0.0 and +0.0 are equals.
__device__ __forceinline__ bool max_takes(float a, float best) {          // within a lane's ascending chain: larger, or the first NaN
    return a > best || (a != a && best == best);
}
__device__ __forceinline__ bool max_takes(float u, int k, float best, int at) {      // between chains: ... or equal at a lower point
    const bool un = u != u, bn = best != best;
    return (un || bn) ? (un && (!bn || k < at)) : (u > best || (u == best && k < at));
}

// block = (channel, cloud); a chain takes its points in ascending order; the chains are folded through LDS in chain order
template <int Q>
__global__ __launch_bounds__(256) void masked_max_fwd_kernel(int c, int n, int na, const float *__restrict__ x, const float *__restrict__ m,
                                                             float *__restrict__ out, int32_t *__restrict__ arg) {
    constexpr int CHAINS = Lanes<Q>::CHAINS;
    __shared__ float4 s_val[CHAINS][Q];
    __shared__ int4 s_idx[CHAINS][Q];
    const Lanes<Q> ln;
    const int ci = blockIdx.x, bi = blockIdx.y, nq = na >> 2;
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int4 at = make_int4(0, 0, 0, 0);
    const float *xp = x + ((size_t)bi * c + ci) * n * na + 4 * min(ln.quad, nq - 1);
    const float *mp = m + (size_t)bi * n;
#pragma unroll Lanes<Q>::ROWS
    for (int p0 = ln.chain; p0 < n; p0 += CHAINS) {                        // ascending within a lane: ">" keeps the first of equals
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p0 * na);
        const float w = mp[p0];
        const float a0 = w * v.x, a1 = w * v.y, a2 = w * v.z, a3 = w * v.w;
        if (max_takes(a0, best.x)) { best.x = a0; at.x = p0; }
        if (max_takes(a1, best.y)) { best.y = a1; at.y = p0; }
        if (max_takes(a2, best.z)) { best.z = a2; at.z = p0; }
        if (max_takes(a3, best.w)) { best.w = a3; at.w = p0; }
    }
    s_val[ln.chain][ln.quad] = best;
    s_idx[ln.chain][ln.quad] = at;
    __syncthreads();
    if (threadIdx.x < nq) {
        const int q = threadIdx.x;
        float4 bv = s_val[0][q];
        int4 bi4 = s_idx[0][q];
        for (int j = 1; j < CHAINS; ++j) {
            const float4 u = s_val[j][q];
            const int4 k = s_idx[j][q];
            if (max_takes(u.x, k.x, bv.x, bi4.x)) { bv.x = u.x; bi4.x = k.x; }
            if (max_takes(u.y, k.y, bv.y, bi4.y)) { bv.y = u.y; bi4.y = k.y; }
            if (max_takes(u.z, k.z, bv.z, bi4.z)) { bv.z = u.z; bi4.z = k.z; }
            if (max_takes(u.w, k.w, bv.w, bi4.w)) { bv.w = u.w; bi4.w = k.w; }
        }
        *reinterpret_cast<float4 *>(out + ((size_t)bi * c + ci) * na + 4 * q) = bv;
        *reinterpret_cast<int4 *>(arg + ((size_t)bi * c + ci) * na + 4 * q) = bi4;
    }
}

// dx[b,c,p,a] = (p == arg[b,c,a]) * mask[b,p] * g[b,c,a], written for every point (no memset + scatter)
template <int Q>
__global__ __launch_bounds__(256) void masked_max_bwd_kernel(int c, int n, int na, const float *__restrict__ g, const int32_t *__restrict__ arg,
                                                             const float *__restrict__ m, float *__restrict__ dx) {
    const Lanes<Q> ln;
    const int ci = blockIdx.x, bi = blockIdx.y, nq = na >> 2;
    if (ln.quad >= nq) return;
    const float4 gv = *reinterpret_cast<const float4 *>(g + ((size_t)bi * c + ci) * na + 4 * ln.quad);
    const int4 at = *reinterpret_cast<const int4 *>(arg + ((size_t)bi * c + ci) * na + 4 * ln.quad);
    float *dp = dx + ((size_t)bi * c + ci) * n * na + 4 * ln.quad;
    const float *mp = m + (size_t)bi * n;
#pragma unroll Lanes<Q>::ROWS
    for (int p0 = ln.chain; p0 < n; p0 += Lanes<Q>::CHAINS) {
        const float w = mp[p0];
        *reinterpret_cast<float4 *>(dp + (size_t)p0 * na) =
            make_float4(p0 == at.x ? w * gv.x : 0.f, p0 == at.y ? w * gv.y : 0.f, p0 == at.z ? w * gv.z : 0.f, p0 == at.w ? w * gv.w : 0.f);
    }
}

// ---- BatchNorm2d + leaky_relu + weighted point mean in one pass: the last unary layer of InvOutBlockOursWithMask and the point
// average behind it (SPConvNets/utils/base_so3conv.py:L1076-1107; between that ReLU and the average the reference's pointnet stage
// is linear, so the average moves in front of it and the activated [b,c,n,a] map is never needed; on a `use_2d` map
// PointnetSO3ConvOurs keeps tot_anchors [240,3,3] for it, L1173-1176, L1196):
//     out[b,c,a] = inv_den[b] sum_p w[b,p] leaky(x[b,c,p,a] scale[b,c] + shift[b,c])
// block = (channel, cloud); a chain takes its points in ascending order, PM_UNROLL rows per loop trip into as many accumulators
// (independent loads in flight, fp32 chains of n / 64 terms); accumulators (a tree) and chains (through LDS, in chain order) are
// folded in a fixed order: bit-identical run to run.  Points past n re-read point n - 1 with weight 0.
constexpr int PM_UNROLL = 4;
constexpr int PM_APPLY_PTS = 512;       // points per block of the backward apply

__device__ __forceinline__ float leaky(float pre, float slope) { return pre > 0.f ? pre : pre * slope; }

template <int Q>
__global__ __launch_bounds__(256) void bn_act_mean_fwd_kernel(int c, int n, int na, float slope, const float *__restrict__ x,
                                                              const float *__restrict__ scale, const float *__restrict__ shift,
                                                              const float *__restrict__ w, const float *__restrict__ inv_den,
                                                              float *__restrict__ out) {
    constexpr int CHAINS = Lanes<Q>::CHAINS;
    __shared__ float4 s_part[CHAINS][Q];                      // [chain][quad]
    const Lanes<Q> ln;
    const int ci = blockIdx.x, bi = blockIdx.y, nq = na >> 2;
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si];
    const float *xp = x + si * n * na + 4 * min(ln.quad, nq - 1);     // an idle lane re-reads the last quad
    const float *wp = w + (size_t)bi * n;
    float4 acc[PM_UNROLL];
#pragma unroll
    for (int u = 0; u < PM_UNROLL; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p0 = ln.chain; p0 < n; p0 += CHAINS * PM_UNROLL) {
        float4 v[PM_UNROLL];
        float wv[PM_UNROLL];
#pragma unroll
        for (int u = 0; u < PM_UNROLL; ++u) {
            const int p = p0 + CHAINS * u, pc = min(p, n - 1);
            v[u] = *reinterpret_cast<const float4 *>(xp + (size_t)pc * na);
            wv[u] = p < n ? wp[pc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PM_UNROLL; ++u) {
            acc[u].x = fmaf(wv[u], leaky(fmaf(v[u].x, sc, sh), slope), acc[u].x);
            acc[u].y = fmaf(wv[u], leaky(fmaf(v[u].y, sc, sh), slope), acc[u].y);
            acc[u].z = fmaf(wv[u], leaky(fmaf(v[u].z, sc, sh), slope), acc[u].z);
            acc[u].w = fmaf(wv[u], leaky(fmaf(v[u].w, sc, sh), slope), acc[u].w);
        }
    }
    s_part[ln.chain][ln.quad] = make_float4((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y),
                                            (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z), (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w));
    __syncthreads();
    if (threadIdx.x < nq) {
        const int q = threadIdx.x;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < CHAINS; ++j) { const float4 u = s_part[j][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float d = inv_den[bi];
        *reinterpret_cast<float4 *>(out + si * na + 4 * q) = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
    }
}

// backward, reduction pass: with gg = (pre > 0 ? 1 : slope) w[b,p] inv_den[b] g[b,c,a] (the gradient the unfused composition would
// broadcast to [b,c,n,a] and read back) formed in registers, the sums of gg and gg xhat over the points and anchors of a (cloud, channel)
// row as CHAINS partials [b][c][chain], for the caller to add in float64: per trip a lane adds its four anchors (a tree) to the row's
// accumulator; behind the loop the accumulators are folded (a tree) and the row's lanes summed
template <int Q>
__global__ __launch_bounds__(256) void bn_act_mean_bwd_reduce_kernel(int c, int n, int na, float slope, const float *__restrict__ g,
                                                                     const float *__restrict__ x, const float *__restrict__ scale,
                                                                     const float *__restrict__ shift, const float *__restrict__ mean,
                                                                     const float *__restrict__ invstd, const float *__restrict__ w,
                                                                     const float *__restrict__ inv_den, float *__restrict__ pg,
                                                                     float *__restrict__ pgx) {
    constexpr int CHAINS = Lanes<Q>::CHAINS;
    const Lanes<Q> ln;
    const int ci = blockIdx.x, bi = blockIdx.y, nq = na >> 2, quad = min(ln.quad, nq - 1);
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si], mu = mean[si], is = invstd[si], d = inv_den[bi];
    float4 gq = *reinterpret_cast<const float4 *>(g + si * na + 4 * quad);
    gq = make_float4(gq.x * d, gq.y * d, gq.z * d, gq.w * d);
    const float *xp = x + si * n * na + 4 * quad;
    const float *wp = w + (size_t)bi * n;
    float s[PM_UNROLL], q[PM_UNROLL];
#pragma unroll
    for (int u = 0; u < PM_UNROLL; ++u) s[u] = q[u] = 0.f;
    for (int p0 = ln.chain; p0 < n; p0 += CHAINS * PM_UNROLL) {
        float4 v[PM_UNROLL];
        float wv[PM_UNROLL];
#pragma unroll
        for (int u = 0; u < PM_UNROLL; ++u) {
            const int p = p0 + CHAINS * u, pc = min(p, n - 1);
            v[u] = *reinterpret_cast<const float4 *>(xp + (size_t)pc * na);
            wv[u] = p < n ? wp[pc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PM_UNROLL; ++u) {
            const float g0 = (fmaf(v[u].x, sc, sh) > 0.f ? gq.x : gq.x * slope) * wv[u], g1 = (fmaf(v[u].y, sc, sh) > 0.f ? gq.y : gq.y * slope) * wv[u];
            const float g2 = (fmaf(v[u].z, sc, sh) > 0.f ? gq.z : gq.z * slope) * wv[u], g3 = (fmaf(v[u].w, sc, sh) > 0.f ? gq.w : gq.w * slope) * wv[u];
            s[u] += (g0 + g1) + (g2 + g3);
            q[u] += (g0 * ((v[u].x - mu) * is) + g1 * ((v[u].y - mu) * is)) + (g2 * ((v[u].z - mu) * is) + g3 * ((v[u].w - mu) * is));
        }
    }
    const bool live = ln.quad < nq;                           // an idle lane re-read the last quad
    const float ts = row_sum<Q>(live ? (s[0] + s[1]) + (s[2] + s[3]) : 0.f), tq = row_sum<Q>(live ? (q[0] + q[1]) + (q[2] + q[3]) : 0.f);
    if (ln.quad == 0) {
        pg[si * CHAINS + ln.chain] = ts;
        pgx[si * CHAINS + ln.chain] = tq;
    }
}

// backward, apply pass: gx = scale gg - stat_mask (k2 + xhat k3), the formula of bn_act_bwd_apply_kernel<CLOUD> (csrc/bn_act.hip) on the gradient
// formed in registers.  block = (channel, cloud, PM_APPLY_PTS points); no reduction
template <int Q>
__global__ __launch_bounds__(256) void bn_act_mean_bwd_apply_kernel(int c, int n, int na, float slope, const float *__restrict__ g,
                                                                    const float *__restrict__ x, const float *__restrict__ scale,
                                                                    const float *__restrict__ shift, const float *__restrict__ mean,
                                                                    const float *__restrict__ invstd, const float *__restrict__ k2,
                                                                    const float *__restrict__ k3, const float *__restrict__ w,
                                                                    const float *__restrict__ inv_den, const float *__restrict__ stat_mask,
                                                                    float *__restrict__ gx) {
    const Lanes<Q> ln;
    const int ci = blockIdx.x, bi = blockIdx.y, nq = na >> 2;
    if (ln.quad >= nq) return;
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si], mu = mean[si], is = invstd[si], c2 = k2[si], c3 = k3[si], d = inv_den[bi];
    float4 gq = *reinterpret_cast<const float4 *>(g + si * na + 4 * ln.quad);
    gq = make_float4(gq.x * d, gq.y * d, gq.z * d, gq.w * d);
    const float *xp = x + si * n * na + 4 * ln.quad;
    float *op = gx + si * n * na + 4 * ln.quad;
    const float *wp = w + (size_t)bi * n;
    const float *mp = stat_mask ? stat_mask + (size_t)bi * n : nullptr;
    const int first = blockIdx.z * PM_APPLY_PTS, last = min(n, first + PM_APPLY_PTS);
    auto one = [&](float gv, float xv, float wv, float m) {
        const float gg = (fmaf(xv, sc, sh) > 0.f ? gv : gv * slope) * wv;
        return fmaf(-m, fmaf((xv - mu) * is, c3, c2), gg * sc);
    };
#pragma unroll Lanes<Q>::ROWS
    for (int p = first + ln.chain; p < last; p += Lanes<Q>::CHAINS) {
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p * na);
        const float wv = wp[p], m = mp ? mp[p] : 1.f;
        *reinterpret_cast<float4 *>(op + (size_t)p * na) = make_float4(one(gq.x, v.x, wv, m), one(gq.y, v.y, wv, m), one(gq.z, v.z, wv, m), one(gq.w, v.w, wv, m));
    }
}

// ---- host side: the checks and launches of an entry, shared by its two instantiations (`who` is the entry's name in messages) ----

// anchor rows of 1 to Q 16-byte words (and at most MAXS slots), every tensor a kernel reads or writes by float4 / int4 on a 16-byte
// boundary (`which` names them in the message)
inline int head_args(const char *who, int na, int max_na, int ns, const char *which, const void *p0, const void *p1, const void *p2 = nullptr,
                     const void *p3 = nullptr) {
    char buf[240];
    if (na <= 0 || na > max_na || (na & 3) != 0 || ns > MAXS) {
        snprintf(buf, sizeof(buf), "%s: anchors must be a multiple of 4, at most %d%s", who, max_na, ns > 0 ? "; at most 8 slots" : "");
        return eap::bad_arg(buf);
    }
    if (!eap::aligned16(p0, p1, p2, p3)) {
        snprintf(buf, sizeof(buf), "%s: %s must be 16-byte aligned", who, which);
        return eap::bad_arg(buf);
    }
    return 0;
}

// the fused norm + point mean: the anchor rule, then the operands every kernel of the entry reads (`required`: one of them null is named
// a refusal, not a fault), then the 16-byte rule on the [b,c,n,na] and [b,c,na] tensors
inline int mean_args(const char *who, int na, int max_na, std::initializer_list<const void *> required, const void *p0, const void *p1,
                     const void *p2) {
    char buf[240];
    if (na <= 0 || na > max_na || (na & 3) != 0) {
        snprintf(buf, sizeof(buf), "%s: anchors must be a multiple of 4, at most %d", who, max_na);
        return eap::bad_arg(buf);
    }
    for (const void *p : required)
        if (!p) {
            snprintf(buf, sizeof(buf), "%s: a required pointer is null", who);
            return eap::bad_arg(buf);
        }
    if (!eap::aligned16(p0, p1, p2)) {
        snprintf(buf, sizeof(buf), "%s: the [b,c,n,na] and [b,c,na] tensors must be 16-byte aligned", who);
        return eap::bad_arg(buf);
    }
    return 0;
}

inline int no_points(const char *who) {                       // a maximum or a mean over nothing is no value
    char buf[96];
    snprintf(buf, sizeof(buf), "%s: no points", who);
    return eap::bad_arg(buf);
}

template <int Q, bool BWD>
int attn_pool(const char *who, int b, int c, int n, int na, float temperature, const float *x, const float *logits, const float *g, float *out,
              float *conf, float *dx, float *dlogits, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = head_args(who, na, 4 * Q, 0, BWD ? "x, logits, dx and dlogits" : "x, logits and conf", x, logits, BWD ? dx : conf, dlogits)) return e;
    return eap::run_kernel(who, anchor_attn_pool_kernel<Q, BWD>, eap::cdiv(n, Lanes<Q>::CHAINS), b, 1, dim3(256), 0, eap::S(stream), c, n, na,
                           temperature, x, logits, g, out, conf, dx, dlogits);
}

// forward (in = x, res = out) or backward (in = g, res = dx), on the kernel of the smallest compiled slot count that holds ns
template <int Q, bool BWD>
int slot_mean(const char *who, int b, int ns, int c, int n, int na, const float *in, const float *mask, const float *inv_den, float *res,
              eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0 || ns <= 0) return 0;
    if (int e = head_args(who, na, 4 * Q, ns, BWD ? "g and dx" : "x and out", in, res)) return e;
    auto go = [&](auto fwd_k, auto bwd_k) {
        return eap::run_kernel(who, BWD ? bwd_k : fwd_k, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, ns, in, mask, inv_den, res);
    };
    if (ns <= 1) return go(slot_mean_fwd_kernel<Q, 1>, slot_mean_bwd_kernel<Q, 1>);
    if (ns <= 2) return go(slot_mean_fwd_kernel<Q, 2>, slot_mean_bwd_kernel<Q, 2>);
    if (ns <= 4) return go(slot_mean_fwd_kernel<Q, 4>, slot_mean_bwd_kernel<Q, 4>);
    return go(slot_mean_fwd_kernel<Q, MAXS>, slot_mean_bwd_kernel<Q, MAXS>);
}

template <int Q>
int masked_max_fwd(const char *who, int b, int c, int n, int na, const float *x, const float *mask, float *out, int32_t *arg, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return no_points(who);
    if (int e = head_args(who, na, 4 * Q, 0, "x, out and arg", x, out, arg)) return e;
    return eap::run_kernel(who, masked_max_fwd_kernel<Q>, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, x, mask, out, arg);
}

template <int Q>
int masked_max_bwd(const char *who, int b, int c, int n, int na, const float *g, const int32_t *arg, const float *mask, float *dx,
                   eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = head_args(who, na, 4 * Q, 0, "g, arg and dx", g, arg, dx)) return e;
    return eap::run_kernel(who, masked_max_bwd_kernel<Q>, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, g, arg, mask, dx);
}

template <int Q>
int mean_fwd(const char *who, int b, int c, int n, int na, float slope, const float *x, const float *scale, const float *shift, const float *w,
             const float *inv_den, float *out, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return no_points(who);
    if (int e = mean_args(who, na, 4 * Q, {x, scale, shift, w, inv_den, out}, x, out, nullptr)) return e;
    return eap::run_kernel(who, bn_act_mean_fwd_kernel<Q>, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, slope, x, scale, shift, w, inv_den, out);
}

template <int Q>
int mean_bwd_reduce(const char *who, int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                    const float *shift, const float *mean, const float *invstd, const float *w, const float *inv_den, float *pg, float *pgx,
                    eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return no_points(who);
    if (int e = mean_args(who, na, 4 * Q, {g, x, scale, shift, mean, invstd, w, inv_den, pg, pgx}, x, g, nullptr)) return e;
    return eap::run_kernel(who, bn_act_mean_bwd_reduce_kernel<Q>, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, slope, g, x, scale, shift, mean,
                           invstd, w, inv_den, pg, pgx);
}

template <int Q>
int mean_bwd_apply(const char *who, int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                   const float *shift, const float *mean, const float *invstd, const float *k2, const float *k3, const float *w,
                   const float *inv_den, const float *stat_mask, float *gx, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return no_points(who);
    if (int e = mean_args(who, na, 4 * Q, {g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, gx}, x, g, gx)) return e;
    return eap::run_kernel(who, bn_act_mean_bwd_apply_kernel<Q>, c, b, eap::cdiv(n, PM_APPLY_PTS), dim3(256), 0, eap::S(stream), c, n, na, slope, g,
                           x, scale, shift, mean, invstd, k2, k3, w, inv_den, stat_mask, gx);
}

}  // namespace

// ---- the C ABI (include/eap_hip.h): the entries without a suffix run Q = 16 on rows of at most 64 floats, the _wide entries Q = 64 on
// every row of at most 256 ----
extern "C" int eap_anchor_attn_pool_fwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                            float *out, float *conf, eap_stream_t stream) {
    return attn_pool<16, false>("anchor_attn_pool_fwd", b, c, n, na, temperature, x, logits, nullptr, out, conf, nullptr, nullptr, stream);
}
extern "C" int eap_anchor_attn_pool_wide_fwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                                 float *out, float *conf, eap_stream_t stream) {
    return attn_pool<64, false>("anchor_attn_pool_wide_fwd", b, c, n, na, temperature, x, logits, nullptr, out, conf, nullptr, nullptr, stream);
}

extern "C" int eap_anchor_attn_pool_bwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                            const float *g, float *dx, float *dlogits, eap_stream_t stream) {
    return attn_pool<16, true>("anchor_attn_pool_bwd", b, c, n, na, temperature, x, logits, g, nullptr, nullptr, dx, dlogits, stream);
}
extern "C" int eap_anchor_attn_pool_wide_bwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                                 const float *g, float *dx, float *dlogits, eap_stream_t stream) {
    return attn_pool<64, true>("anchor_attn_pool_wide_bwd", b, c, n, na, temperature, x, logits, g, nullptr, nullptr, dx, dlogits, stream);
}

extern "C" int eap_slot_masked_mean_fwd_f32(int b, int ns, int c, int n, int na, const float *x, const float *mask,
                                            const float *inv_den, float *out, eap_stream_t stream) {
    return slot_mean<16, false>("slot_masked_mean_fwd", b, ns, c, n, na, x, mask, inv_den, out, stream);
}
extern "C" int eap_slot_masked_mean_wide_fwd_f32(int b, int ns, int c, int n, int na, const float *x, const float *mask,
                                                 const float *inv_den, float *out, eap_stream_t stream) {
    return slot_mean<64, false>("slot_masked_mean_wide_fwd", b, ns, c, n, na, x, mask, inv_den, out, stream);
}

extern "C" int eap_slot_masked_mean_bwd_f32(int b, int ns, int c, int n, int na, const float *g, const float *mask,
                                            const float *inv_den, float *dx, eap_stream_t stream) {
    return slot_mean<16, true>("slot_masked_mean_bwd", b, ns, c, n, na, g, mask, inv_den, dx, stream);
}
extern "C" int eap_slot_masked_mean_wide_bwd_f32(int b, int ns, int c, int n, int na, const float *g, const float *mask,
                                                 const float *inv_den, float *dx, eap_stream_t stream) {
    return slot_mean<64, true>("slot_masked_mean_wide_bwd", b, ns, c, n, na, g, mask, inv_den, dx, stream);
}

extern "C" int eap_masked_max_fwd_f32(int b, int c, int n, int na, const float *x, const float *mask, float *out, int32_t *arg,
                                      eap_stream_t stream) {
    return masked_max_fwd<16>("masked_max_fwd", b, c, n, na, x, mask, out, arg, stream);
}
extern "C" int eap_masked_max_wide_fwd_f32(int b, int c, int n, int na, const float *x, const float *mask, float *out, int32_t *arg,
                                           eap_stream_t stream) {
    return masked_max_fwd<64>("masked_max_wide_fwd", b, c, n, na, x, mask, out, arg, stream);
}

extern "C" int eap_masked_max_bwd_f32(int b, int c, int n, int na, const float *g, const int32_t *arg, const float *mask, float *dx,
                                      eap_stream_t stream) {
    return masked_max_bwd<16>("masked_max_bwd", b, c, n, na, g, arg, mask, dx, stream);
}
extern "C" int eap_masked_max_wide_bwd_f32(int b, int c, int n, int na, const float *g, const int32_t *arg, const float *mask, float *dx,
                                           eap_stream_t stream) {
    return masked_max_bwd<64>("masked_max_wide_bwd", b, c, n, na, g, arg, mask, dx, stream);
}

// ---- BatchNorm2d + leaky_relu + weighted point mean (InvOutBlockOursWithMask, SPConvNets/utils/base_so3conv.py:L1076-1107) ----
// partial sums per (cloud, channel) the backward reduction leaves: one per chain
extern "C" int eap_bn_act_cloud_mean_parts(int n) { return n > 0 ? Lanes<16>::CHAINS : 0; }
extern "C" int eap_bn_act_cloud_mean_wide_parts(int n) { return n > 0 ? Lanes<64>::CHAINS : 0; }

extern "C" int eap_bn_act_cloud_mean_fwd_f32(int b, int c, int n, int na, float slope, const float *x, const float *scale, const float *shift,
                                             const float *w, const float *inv_den, float *out, eap_stream_t stream) {
    return mean_fwd<16>("bn_act_cloud_mean_fwd", b, c, n, na, slope, x, scale, shift, w, inv_den, out, stream);
}
extern "C" int eap_bn_act_cloud_mean_wide_fwd_f32(int b, int c, int n, int na, float slope, const float *x, const float *scale, const float *shift,
                                                  const float *w, const float *inv_den, float *out, eap_stream_t stream) {
    return mean_fwd<64>("bn_act_cloud_mean_wide_fwd", b, c, n, na, slope, x, scale, shift, w, inv_den, out, stream);
}

extern "C" int eap_bn_act_cloud_mean_bwd_reduce_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                    const float *shift, const float *mean, const float *invstd, const float *w,
                                                    const float *inv_den, float *pg, float *pgx, eap_stream_t stream) {
    return mean_bwd_reduce<16>("bn_act_cloud_mean_bwd_reduce", b, c, n, na, slope, g, x, scale, shift, mean, invstd, w, inv_den, pg, pgx, stream);
}
extern "C" int eap_bn_act_cloud_mean_wide_bwd_reduce_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                         const float *shift, const float *mean, const float *invstd, const float *w,
                                                         const float *inv_den, float *pg, float *pgx, eap_stream_t stream) {
    return mean_bwd_reduce<64>("bn_act_cloud_mean_wide_bwd_reduce", b, c, n, na, slope, g, x, scale, shift, mean, invstd, w, inv_den, pg, pgx, stream);
}

extern "C" int eap_bn_act_cloud_mean_bwd_apply_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                   const float *shift, const float *mean, const float *invstd, const float *k2, const float *k3,
                                                   const float *w, const float *inv_den, const float *stat_mask, float *gx, eap_stream_t stream) {
    return mean_bwd_apply<16>("bn_act_cloud_mean_bwd_apply", b, c, n, na, slope, g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, stat_mask, gx,
                              stream);
}
extern "C" int eap_bn_act_cloud_mean_wide_bwd_apply_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                        const float *shift, const float *mean, const float *invstd, const float *k2, const float *k3,
                                                        const float *w, const float *inv_den, const float *stat_mask, float *gx,
                                                        eap_stream_t stream) {
    return mean_bwd_apply<64>("bn_act_cloud_mean_wide_bwd_apply", b, c, n, na, slope, g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, stat_mask,
                              gx, stream);
}
