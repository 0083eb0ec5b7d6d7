// csrc/heads_wide.hip -- the three oldest kernel pairs of csrc/heads.hip (anchor attention pooling, slot-masked point mean, masked
// point max; the definitions are given there and in include/eap_hip.h) for anchor rows of up to 256 floats: the [B,C,N,240] map a
// `use_2d` backbone (60 space anchors x 4 plane anchors) hands to InvPPOutBlockOurs / InvPPOutBlock2DOurs
// (SPConvNets/utils/base_so3conv.py:L842-917, L921-1008) and to the poolings of SO3OutBlockRTWithMaskSep
// (SPConvNets/models/model_utils.py:L470-484, L549-552).  heads.hip keeps a point's anchors in 16 lanes and stops at 64 anchors.
//
// Mapping: ONE WAVEFRONT owns one point's anchor row; lane l holds the 16-byte quad l of up to 64 (at 240 anchors lanes 60-63
// idle): one load instruction covers the row's 960 contiguous bytes.  Reductions over the anchors are 6 shuffle steps over the
// wave.  HBM-bound: x is read once forward; the backward reads x or g once and writes dx once.  No atomics; every sum has a fixed
// order, so results are bit-identical run to run.  Behind them the wide twin of the fused BatchNorm + leaky_relu + point mean of
// csrc/heads.hip (eap_bn_act_cloud_mean_wide_*), on the same mapping.
#include <initializer_list>

#include "common.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
    v += __shfl_xor(v, 32); v += __shfl_xor(v, 16); v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 32)); v = fmaxf(v, __shfl_xor(v, 16)); v = fmaxf(v, __shfl_xor(v, 8));
    v = fmaxf(v, __shfl_xor(v, 4)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 1));
    return v;
}

constexpr int WAVES = 4;    // per block, every kernel here

// the wave's index in its block as a value the compiler knows to be the same in every lane: what a wave reads per POINT (a mask weight, a
// channel's gradient) then comes through the scalar cache instead of 64 lanes fetching one address
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// block = 4 waves = 4 consecutive points of one cloud; every wave walks all channels of its point
template <bool BWD>
__global__ __launch_bounds__(256) void anchor_attn_pool_wide_kernel(int c, int n, int na, float temperature,
                                                                   const float *__restrict__ x, const float *__restrict__ logits,
                                                                   const float *__restrict__ g, float *__restrict__ out,
                                                                   float *__restrict__ conf_out, float *__restrict__ dx,
                                                                   float *__restrict__ dlogits) {
    const int bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index();
    const int pt = blockIdx.x * WAVES + wave, nq = na >> 2;
    if (pt >= n) return;                                     // the whole wave: no block-wide barrier below
    const bool live = lane < nq;
    const int quad = min(lane, nq - 1);                      // an idle lane re-reads the last quad
    const size_t row = ((size_t)bi * n + pt) * na + 4 * quad;
    // softmax over the anchors of this point
    float4 l = *reinterpret_cast<const float4 *>(logits + row);
    l.x *= temperature; l.y *= temperature; l.z *= temperature; l.w *= temperature;
    if (!live) l = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    const float m = wave_max(fmaxf(fmaxf(l.x, l.y), fmaxf(l.z, l.w)));
    float4 e = make_float4(__expf(l.x - m), __expf(l.y - m), __expf(l.z - m), __expf(l.w - m));
    if (!live) e = make_float4(0.f, 0.f, 0.f, 0.f);
    const float inv = 1.0f / wave_sum(e.x + e.y + e.z + e.w);
    const float4 cf = make_float4(e.x * inv, e.y * inv, e.z * inv, e.w * inv);
    if (!BWD && live && conf_out) *reinterpret_cast<float4 *>(conf_out + row) = cf;
    const size_t cs = (size_t)n * na;                        // channel stride of x
    const float *xp = x + (size_t)bi * c * cs + ((size_t)pt * na + 4 * quad);
    if (!BWD) {
        float *op = out + (size_t)bi * c * n + pt;
        auto dot = [&](const float4 v) { return live ? v.x * cf.x + v.y * cf.y + v.z * cf.z + v.w * cf.w : 0.f; };
        int ci = 0;
        for (; ci + 4 <= c; ci += 4) {                       // 4 rows in flight per wave; every channel's sum in the same order
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(xp + (size_t)(ci + u) * cs);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float s = wave_sum(dot(v[u]));
                if (lane == 0) op[(size_t)(ci + u) * n] = s;
            }
        }
        for (; ci < c; ++ci) {
            const float s = wave_sum(dot(*reinterpret_cast<const float4 *>(xp + (size_t)ci * cs)));
            if (lane == 0) op[(size_t)ci * n] = s;
        }
    } else {
        const float *gp = g + (size_t)bi * c * n + pt;
        float *dxp = dx + (size_t)bi * c * cs + ((size_t)pt * na + 4 * quad);
        float4 dc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int ci = 0; ci < c; ++ci) {
            const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)ci * cs);
            const float gv = gp[(size_t)ci * n];
            dc.x = fmaf(gv, v.x, dc.x); dc.y = fmaf(gv, v.y, dc.y); dc.z = fmaf(gv, v.z, dc.z); dc.w = fmaf(gv, v.w, dc.w);
            if (live) *reinterpret_cast<float4 *>(dxp + (size_t)ci * cs) = make_float4(gv * cf.x, gv * cf.y, gv * cf.z, gv * cf.w);
        }
        // softmax backward: dlogit = T conf (dconf - sum_a conf dconf)
        const float s = wave_sum(live ? cf.x * dc.x + cf.y * dc.y + cf.z * dc.z + cf.w * dc.w : 0.f);
        if (live) *reinterpret_cast<float4 *>(dlogits + row) = make_float4(temperature * cf.x * (dc.x - s), temperature * cf.y * (dc.y - s),
                                                                          temperature * cf.z * (dc.z - s), temperature * cf.w * (dc.w - s));
    }
}

constexpr int MAXS = 8;     // slots per launch

// Both slot kernels are compiled for NS = 1, 2, 4 and 8 slots and run at the smallest NS >= ns.  A point's NS weights are fetched
// unconditionally (slots past ns re-read slot ns - 1), so the scalar loads of an iteration go out together; a load behind an `if (s < ns)`
// would wait for the one before it.

// forward: block = (channel, cloud); wave w takes the points w, w + 4, ..., one row per iteration; per slot one float4 accumulator
// per lane (those past ns gather values nobody reads); the 4 waves' partials are folded through LDS in wave order
template <int NS>
__global__ __launch_bounds__(256) void slot_mean_wide_fwd_kernel(int c, int n, int na, int ns, const float *__restrict__ x,
                                                                 const float *__restrict__ m, const float *__restrict__ inv_den,
                                                                 float *__restrict__ out) {
    __shared__ float4 s_part[NS][WAVES][64];                  // [slot][wave][quad], 4 KB per slot
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index(), nq = na >> 2;
    float4 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *xp = x + ((size_t)bi * c + ci) * n * na + 4 * min(lane, nq - 1);
    const float *mp = m + (size_t)bi * ns * n;
#pragma unroll 4
    for (int p0 = wave; p0 < n; p0 += WAVES) {
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
        if (s < ns) s_part[s][wave][lane] = acc[s];
    __syncthreads();
    for (int e = threadIdx.x; e < ns * nq; e += 256) {
        const int s = e / nq, q = e - s * nq;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < WAVES; ++j) { const float4 u = s_part[s][j][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float d = inv_den[(size_t)bi * ns + s];
        *reinterpret_cast<float4 *>(out + (((size_t)bi * ns + s) * c + ci) * na + 4 * q) = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
    }
}

// backward w.r.t. x: dx[b,c,n,a] = sum_s g[b,s,c,a] m[b,s,n] inv_den[b,s]; a slot past ns is the term 0 * 0, which leaves the sum as it is
template <int NS>
__global__ __launch_bounds__(256) void slot_mean_wide_bwd_kernel(int c, int n, int na, int ns, const float *__restrict__ g,
                                                                 const float *__restrict__ m, const float *__restrict__ inv_den,
                                                                 float *__restrict__ dx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index(), nq = na >> 2;
    if (lane >= nq) return;
    float4 gv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        gv[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < ns) {
            const float d = inv_den[(size_t)bi * ns + s];
            const float4 t = *reinterpret_cast<const float4 *>(g + (((size_t)bi * ns + s) * c + ci) * na + 4 * lane);
            gv[s] = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
        }
    }
    float *dp = dx + ((size_t)bi * c + ci) * n * na + 4 * lane;
    const float *mp = m + (size_t)bi * ns * n;
#pragma unroll 4
    for (int p0 = wave; p0 < n; p0 += WAVES) {
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

// the kernel of the smallest compiled slot count that holds ns
template <typename... A>
int run_slot_kernel(bool bwd, const char *what, int ns, long long gx, long long gy, hipStream_t s, A... a) {
    auto go = [&](auto fwd_k, auto bwd_k) { return eap::run_kernel(what, bwd ? bwd_k : fwd_k, gx, gy, 1, dim3(256), 0, s, a...); };
    if (ns <= 1) return go(slot_mean_wide_fwd_kernel<1>, slot_mean_wide_bwd_kernel<1>);
    if (ns <= 2) return go(slot_mean_wide_fwd_kernel<2>, slot_mean_wide_bwd_kernel<2>);
    if (ns <= 4) return go(slot_mean_wide_fwd_kernel<4>, slot_mean_wide_bwd_kernel<4>);
    return go(slot_mean_wide_fwd_kernel<MAXS>, slot_mean_wide_bwd_kernel<MAXS>);
}

// the tie and NaN rules of masked_max_fwd_kernel (csrc/heads.hip)
__device__ __forceinline__ bool max_takes(float a, float best) {          // within a lane's ascending chain: larger, or the first NaN
    return a > best || (a != a && best == best);
}
__device__ __forceinline__ bool max_takes(float u, int k, float best, int at) {      // between chains: ... or equal at a lower point
    const bool un = u != u, bn = best != best;
    return (un || bn) ? (un && (!bn || k < at)) : (u > best || (u == best && k < at));
}

// block = (channel, cloud); wave w takes the points w, w + 4, ... in ascending order; the 4 waves are folded through LDS in wave order
__global__ __launch_bounds__(256) void masked_max_wide_fwd_kernel(int c, int n, int na, const float *__restrict__ x, const float *__restrict__ m,
                                                                  float *__restrict__ out, int32_t *__restrict__ arg) {
    __shared__ float4 s_val[WAVES][64];
    __shared__ int4 s_idx[WAVES][64];
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index(), nq = na >> 2;
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int4 at = make_int4(0, 0, 0, 0);
    const float *xp = x + ((size_t)bi * c + ci) * n * na + 4 * min(lane, nq - 1);
    const float *mp = m + (size_t)bi * n;
#pragma unroll 4
    for (int p0 = wave; p0 < n; p0 += WAVES) {                             // ascending within a lane: ">" keeps the first of equals
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p0 * na);
        const float w = mp[p0];
        const float a0 = w * v.x, a1 = w * v.y, a2 = w * v.z, a3 = w * v.w;
        if (max_takes(a0, best.x)) { best.x = a0; at.x = p0; }
        if (max_takes(a1, best.y)) { best.y = a1; at.y = p0; }
        if (max_takes(a2, best.z)) { best.z = a2; at.z = p0; }
        if (max_takes(a3, best.w)) { best.w = a3; at.w = p0; }
    }
    s_val[wave][lane] = best;
    s_idx[wave][lane] = at;
    __syncthreads();
    if (threadIdx.x < nq) {
        const int q = threadIdx.x;
        float4 bv = s_val[0][q];
        int4 bi4 = s_idx[0][q];
        for (int j = 1; j < WAVES; ++j) {
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
__global__ __launch_bounds__(256) void masked_max_wide_bwd_kernel(int c, int n, int na, const float *__restrict__ g, const int32_t *__restrict__ arg,
                                                                  const float *__restrict__ m, float *__restrict__ dx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index(), nq = na >> 2;
    if (lane >= nq) return;
    const float4 gv = *reinterpret_cast<const float4 *>(g + ((size_t)bi * c + ci) * na + 4 * lane);
    const int4 at = *reinterpret_cast<const int4 *>(arg + ((size_t)bi * c + ci) * na + 4 * lane);
    float *dp = dx + ((size_t)bi * c + ci) * n * na + 4 * lane;
    const float *mp = m + (size_t)bi * n;
#pragma unroll 4
    for (int p0 = wave; p0 < n; p0 += WAVES) {
        const float w = mp[p0];
        *reinterpret_cast<float4 *>(dp + (size_t)p0 * na) =
            make_float4(p0 == at.x ? w * gv.x : 0.f, p0 == at.y ? w * gv.y : 0.f, p0 == at.z ? w * gv.z : 0.f, p0 == at.w ? w * gv.w : 0.f);
    }
}

// ---- BatchNorm2d + leaky_relu + weighted point mean in one pass (bn_act_mean_*_kernel of csrc/heads.hip, whose lanes are (point group of
// 4, anchor quad of 16) and stop at 64 anchors): the last unary layer of InvOutBlockOursWithMask and the point average behind it on a
// `use_2d` map (SPConvNets/utils/base_so3conv.py:L1076-1107; PointnetSO3ConvOurs keeps tot_anchors [240,3,3] for it, L1173-1176, L1196):
//     out[b,c,a] = inv_den[b] sum_p w[b,p] leaky(x[b,c,p,a] scale[b,c] + shift[b,c])
// block = (channel, cloud); wave w takes the points w, w + 4, ... in ascending order, PMW_ROWS rows per loop trip into as many accumulators
// (independent loads in flight, fp32 chains of ceil(n / 16) terms); accumulators (a tree) and waves (through LDS, in wave order) are folded
// in a fixed order: bit-identical run to run.  Points past n re-read point n - 1 with weight 0.  What a wave reads per point (w, stat_mask)
// and per block (scale ... inv_den) has a wave-uniform address and comes through the scalar cache.
constexpr int PMW_ROWS = 4;
constexpr int PMW_PARTS = WAVES;        // partial sums per (cloud, channel) the backward reduction leaves: one per wave
constexpr int PMW_APPLY_PTS = 512;      // points per block of the backward apply

__device__ __forceinline__ float leaky(float pre, float slope) { return pre > 0.f ? pre : pre * slope; }

__global__ __launch_bounds__(256) void bn_act_mean_wide_fwd_kernel(int c, int n, int na, float slope, const float *__restrict__ x,
                                                                   const float *__restrict__ scale, const float *__restrict__ shift,
                                                                   const float *__restrict__ w, const float *__restrict__ inv_den,
                                                                   float *__restrict__ out) {
    __shared__ float4 s_part[WAVES][64];                      // [wave][quad]
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index(), nq = na >> 2;
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si];
    const float *xp = x + si * n * na + 4 * min(lane, nq - 1);    // an idle lane re-reads the last quad
    const float *wp = w + (size_t)bi * n;
    float4 acc[PMW_ROWS];
#pragma unroll
    for (int u = 0; u < PMW_ROWS; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p0 = wave; p0 < n; p0 += WAVES * PMW_ROWS) {
        float4 v[PMW_ROWS];
        float wv[PMW_ROWS];
#pragma unroll
        for (int u = 0; u < PMW_ROWS; ++u) {
            const int p = p0 + WAVES * u, pc = min(p, n - 1);
            v[u] = *reinterpret_cast<const float4 *>(xp + (size_t)pc * na);
            wv[u] = p < n ? wp[pc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PMW_ROWS; ++u) {
            acc[u].x = fmaf(wv[u], leaky(fmaf(v[u].x, sc, sh), slope), acc[u].x);
            acc[u].y = fmaf(wv[u], leaky(fmaf(v[u].y, sc, sh), slope), acc[u].y);
            acc[u].z = fmaf(wv[u], leaky(fmaf(v[u].z, sc, sh), slope), acc[u].z);
            acc[u].w = fmaf(wv[u], leaky(fmaf(v[u].w, sc, sh), slope), acc[u].w);
        }
    }
    s_part[wave][lane] = make_float4((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y),
                                     (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z), (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w));
    __syncthreads();
    if (threadIdx.x < nq) {
        const int q = threadIdx.x;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < WAVES; ++j) { const float4 u = s_part[j][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float d = inv_den[bi];
        *reinterpret_cast<float4 *>(out + si * na + 4 * q) = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
    }
}

// backward, reduction pass: with gg = (pre > 0 ? 1 : slope) w[b,p] inv_den[b] g[b,c,a] formed in registers, the sums of gg and gg xhat
// over the points and anchors of a (cloud, channel) row as PMW_PARTS partials [b][c][wave], for the caller to add in float64: per trip a
// lane adds its four anchors (a tree) to the row's accumulator; behind the loop the accumulators are folded (a tree) and the wave summed
__global__ __launch_bounds__(256) void bn_act_mean_wide_bwd_reduce_kernel(int c, int n, int na, float slope, const float *__restrict__ g,
                                                                          const float *__restrict__ x, const float *__restrict__ scale,
                                                                          const float *__restrict__ shift, const float *__restrict__ mean,
                                                                          const float *__restrict__ invstd, const float *__restrict__ w,
                                                                          const float *__restrict__ inv_den, float *__restrict__ pg,
                                                                          float *__restrict__ pgx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index(), nq = na >> 2;
    const int quad = min(lane, nq - 1);
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si], mu = mean[si], is = invstd[si], d = inv_den[bi];
    float4 gq = *reinterpret_cast<const float4 *>(g + si * na + 4 * quad);
    gq = make_float4(gq.x * d, gq.y * d, gq.z * d, gq.w * d);
    const float *xp = x + si * n * na + 4 * quad;
    const float *wp = w + (size_t)bi * n;
    float s[PMW_ROWS], q[PMW_ROWS];
#pragma unroll
    for (int u = 0; u < PMW_ROWS; ++u) s[u] = q[u] = 0.f;
    for (int p0 = wave; p0 < n; p0 += WAVES * PMW_ROWS) {
        float4 v[PMW_ROWS];
        float wv[PMW_ROWS];
#pragma unroll
        for (int u = 0; u < PMW_ROWS; ++u) {
            const int p = p0 + WAVES * u, pc = min(p, n - 1);
            v[u] = *reinterpret_cast<const float4 *>(xp + (size_t)pc * na);
            wv[u] = p < n ? wp[pc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PMW_ROWS; ++u) {
            const float g0 = (fmaf(v[u].x, sc, sh) > 0.f ? gq.x : gq.x * slope) * wv[u], g1 = (fmaf(v[u].y, sc, sh) > 0.f ? gq.y : gq.y * slope) * wv[u];
            const float g2 = (fmaf(v[u].z, sc, sh) > 0.f ? gq.z : gq.z * slope) * wv[u], g3 = (fmaf(v[u].w, sc, sh) > 0.f ? gq.w : gq.w * slope) * wv[u];
            s[u] += (g0 + g1) + (g2 + g3);
            q[u] += (g0 * ((v[u].x - mu) * is) + g1 * ((v[u].y - mu) * is)) + (g2 * ((v[u].z - mu) * is) + g3 * ((v[u].w - mu) * is));
        }
    }
    const bool live = lane < nq;                              // an idle lane re-read the last quad
    const float ts = wave_sum(live ? (s[0] + s[1]) + (s[2] + s[3]) : 0.f), tq = wave_sum(live ? (q[0] + q[1]) + (q[2] + q[3]) : 0.f);
    if (lane == 0) {
        pg[si * PMW_PARTS + wave] = ts;
        pgx[si * PMW_PARTS + wave] = tq;
    }
}

// backward, apply pass: gx = scale gg - stat_mask (k2 + xhat k3), the formula of bn_act_mean_bwd_apply_kernel (csrc/heads.hip).
// block = (channel, cloud, PMW_APPLY_PTS points); no reduction
__global__ __launch_bounds__(256) void bn_act_mean_wide_bwd_apply_kernel(int c, int n, int na, float slope, const float *__restrict__ g,
                                                                         const float *__restrict__ x, const float *__restrict__ scale,
                                                                         const float *__restrict__ shift, const float *__restrict__ mean,
                                                                         const float *__restrict__ invstd, const float *__restrict__ k2,
                                                                         const float *__restrict__ k3, const float *__restrict__ w,
                                                                         const float *__restrict__ inv_den, const float *__restrict__ stat_mask,
                                                                         float *__restrict__ gx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_index(), nq = na >> 2;
    if (lane >= nq) return;
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si], mu = mean[si], is = invstd[si], c2 = k2[si], c3 = k3[si], d = inv_den[bi];
    float4 gq = *reinterpret_cast<const float4 *>(g + si * na + 4 * lane);
    gq = make_float4(gq.x * d, gq.y * d, gq.z * d, gq.w * d);
    const float *xp = x + si * n * na + 4 * lane;
    float *op = gx + si * n * na + 4 * lane;
    const float *wp = w + (size_t)bi * n;
    const float *mp = stat_mask ? stat_mask + (size_t)bi * n : nullptr;
    const int first = blockIdx.z * PMW_APPLY_PTS, last = min(n, first + PMW_APPLY_PTS);
    auto one = [&](float gv, float xv, float wv, float m) {
        const float gg = (fmaf(xv, sc, sh) > 0.f ? gv : gv * slope) * wv;
        return fmaf(-m, fmaf((xv - mu) * is, c3, c2), gg * sc);
    };
#pragma unroll 4
    for (int p = first + wave; p < last; p += WAVES) {
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p * na);
        const float wv = wp[p], m = mp ? mp[p] : 1.f;
        *reinterpret_cast<float4 *>(op + (size_t)p * na) = make_float4(one(gq.x, v.x, wv, m), one(gq.y, v.y, wv, m), one(gq.z, v.z, wv, m), one(gq.w, v.w, wv, m));
    }
}

// anchor rows of 1 to 64 16-byte words (and at most MAXS slots), every tensor a kernel reads or writes by float4 / int4 on a 16-byte
// boundary (`which` names them in the message): the message form of head_args (csrc/heads.hip)
inline int wide_args(const char *who, int na, int ns, const char *which, const void *p0, const void *p1, const void *p2 = nullptr,
                     const void *p3 = nullptr) {
    char buf[240];
    if (na <= 0 || na > 256 || (na & 3) != 0 || ns > MAXS) {
        snprintf(buf, sizeof(buf), "%s: anchors must be a multiple of 4, at most 256%s", who, ns > 0 ? "; at most 8 slots" : "");
        return eap::bad_arg(buf);
    }
    if (((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2) | reinterpret_cast<uintptr_t>(p3)) & 15) != 0) {
        snprintf(buf, sizeof(buf), "%s: %s must be 16-byte aligned", who, which);
        return eap::bad_arg(buf);
    }
    return 0;
}

// the fused norm + point mean: the anchor rule, then the operands every kernel of the entry reads (`required`: one of them null is named
// a refusal, not a fault), then the 16-byte rule on the [b,c,n,na] and [b,c,na] tensors
inline int wide_mean_args(const char *who, int na, std::initializer_list<const void *> required, const void *p0, const void *p1, const void *p2) {
    char buf[240];
    if (na <= 0 || na > 256 || (na & 3) != 0) {
        snprintf(buf, sizeof(buf), "%s: anchors must be a multiple of 4, at most 256", who);
        return eap::bad_arg(buf);
    }
    for (const void *p : required)
        if (!p) {
            snprintf(buf, sizeof(buf), "%s: a required pointer is null", who);
            return eap::bad_arg(buf);
        }
    if (((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2)) & 15) != 0) {
        snprintf(buf, sizeof(buf), "%s: the [b,c,n,na] and [b,c,na] tensors must be 16-byte aligned", who);
        return eap::bad_arg(buf);
    }
    return 0;
}

}  // namespace

extern "C" int eap_anchor_attn_pool_wide_fwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                                 float *out, float *conf, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = wide_args("anchor_attn_pool_wide_fwd", na, 0, "x, logits and conf", x, logits, conf)) return e;
    return eap::run_kernel("anchor_attn_pool_wide_fwd", anchor_attn_pool_wide_kernel<false>, eap::cdiv(n, WAVES), b, 1, dim3(256), 0, eap::S(stream), c, n,
                           na, temperature, x, logits, nullptr, out, conf, nullptr, nullptr);
}

extern "C" int eap_anchor_attn_pool_wide_bwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                                 const float *g, float *dx, float *dlogits, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = wide_args("anchor_attn_pool_wide_bwd", na, 0, "x, logits, dx and dlogits", x, logits, dx, dlogits)) return e;
    return eap::run_kernel("anchor_attn_pool_wide_bwd", anchor_attn_pool_wide_kernel<true>, eap::cdiv(n, WAVES), b, 1, dim3(256), 0, eap::S(stream), c, n,
                           na, temperature, x, logits, g, nullptr, nullptr, dx, dlogits);
}

extern "C" int eap_slot_masked_mean_wide_fwd_f32(int b, int ns, int c, int n, int na, const float *x, const float *mask,
                                                 const float *inv_den, float *out, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0 || ns <= 0) return 0;
    if (int e = wide_args("slot_masked_mean_wide_fwd", na, ns, "x and out", x, out)) return e;
    return run_slot_kernel(false, "slot_masked_mean_wide_fwd", ns, c, b, eap::S(stream), c, n, na, ns, x, mask, inv_den, out);
}

extern "C" int eap_slot_masked_mean_wide_bwd_f32(int b, int ns, int c, int n, int na, const float *g, const float *mask,
                                                 const float *inv_den, float *dx, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0 || ns <= 0) return 0;
    if (int e = wide_args("slot_masked_mean_wide_bwd", na, ns, "g and dx", g, dx)) return e;
    return run_slot_kernel(true, "slot_masked_mean_wide_bwd", ns, c, b, eap::S(stream), c, n, na, ns, g, mask, inv_den, dx);
}

extern "C" int eap_masked_max_wide_fwd_f32(int b, int c, int n, int na, const float *x, const float *mask, float *out, int32_t *arg,
                                           eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("masked_max_wide_fwd: no points");        // as masked_max_fwd: a maximum over nothing is no value
    if (int e = wide_args("masked_max_wide_fwd", na, 0, "x, out and arg", x, out, arg)) return e;
    return eap::run_kernel("masked_max_wide_fwd", masked_max_wide_fwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, x, mask, out, arg);
}

extern "C" int eap_masked_max_wide_bwd_f32(int b, int c, int n, int na, const float *g, const int32_t *arg, const float *mask, float *dx,
                                           eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = wide_args("masked_max_wide_bwd", na, 0, "g, arg and dx", g, arg, dx)) return e;
    return eap::run_kernel("masked_max_wide_bwd", masked_max_wide_bwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, g, arg, mask, dx);
}

// ---- BatchNorm2d + leaky_relu + weighted point mean on wide anchor rows (InvOutBlockOursWithMask, SPConvNets/utils/base_so3conv.py:L1076-1107) ----
extern "C" int eap_bn_act_cloud_mean_wide_parts(int n) { return n > 0 ? PMW_PARTS : 0; }

extern "C" int eap_bn_act_cloud_mean_wide_fwd_f32(int b, int c, int n, int na, float slope, const float *x, const float *scale, const float *shift,
                                                  const float *w, const float *inv_den, float *out, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("bn_act_cloud_mean_wide_fwd: no points");
    if (int e = wide_mean_args("bn_act_cloud_mean_wide_fwd", na, {x, scale, shift, w, inv_den, out}, x, out, nullptr)) return e;
    return eap::run_kernel("bn_act_cloud_mean_wide_fwd", bn_act_mean_wide_fwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, slope, x, scale,
                           shift, w, inv_den, out);
}

extern "C" int eap_bn_act_cloud_mean_wide_bwd_reduce_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                         const float *shift, const float *mean, const float *invstd, const float *w,
                                                         const float *inv_den, float *pg, float *pgx, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("bn_act_cloud_mean_wide_bwd_reduce: no points");
    if (int e = wide_mean_args("bn_act_cloud_mean_wide_bwd_reduce", na, {g, x, scale, shift, mean, invstd, w, inv_den, pg, pgx}, x, g, nullptr)) return e;
    return eap::run_kernel("bn_act_cloud_mean_wide_bwd_reduce", bn_act_mean_wide_bwd_reduce_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, slope,
                           g, x, scale, shift, mean, invstd, w, inv_den, pg, pgx);
}

extern "C" int eap_bn_act_cloud_mean_wide_bwd_apply_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                        const float *shift, const float *mean, const float *invstd, const float *k2, const float *k3,
                                                        const float *w, const float *inv_den, const float *stat_mask, float *gx, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("bn_act_cloud_mean_wide_bwd_apply: no points");
    if (int e = wide_mean_args("bn_act_cloud_mean_wide_bwd_apply", na, {g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, gx}, x, g, gx)) return e;
    return eap::run_kernel("bn_act_cloud_mean_wide_bwd_apply", bn_act_mean_wide_bwd_apply_kernel, c, b, eap::cdiv(n, PMW_APPLY_PTS), dim3(256), 0,
                           eap::S(stream), c, n, na, slope, g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, stat_mask, gx);
}
