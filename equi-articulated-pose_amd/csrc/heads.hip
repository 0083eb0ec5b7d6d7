// csrc/heads.hip -- the anchor-axis reductions of the heads that read the backbone's [B,C,N,A] feature map
// (SURVEY.md section 8(f) rows 2 and 3): one pass over the map instead of the reference's 3-4 torch passes.
//
//   anchor attention pooling   InvPPOutBlockOurs.forward, SPConvNets/utils/base_so3conv.py:L905-912:
//        conf[b,n,a] = softmax_a(logit[b,n,a] * T);   out[b,c,n] = sum_a x[b,c,n,a] conf[b,n,a]
//   slot-masked point mean     the pose head's masked averages over the points of every slot at once
//        (SPConvNets/models/model_utils.py:L470-472 + L484 / L549-552, called once per slot by
//        ...pn_38_multi_stage.py:L695-1015):   out[b,s,c,a] = sum_n m[b,s,n] x[b,c,n,a] / max(sum_n m[b,s,n], 1e-8)
//   norm + act + point mean    the last unary layer of InvOutBlockOursWithMask and the point average behind it
//        (SPConvNets/utils/base_so3conv.py:L1076-1107):   out[b,c,a] = inv_den[b] sum_p w[b,p] leaky(x[b,c,p,a] scale[b,c] + shift[b,c])
//
// Mapping: 16 lanes per point (15 anchor quads of a 60-anchor row + one idle lane), 4 consecutive points per
// wave: one 16-byte load per lane covers 960 contiguous bytes of x; reductions over the anchors are 4 shuffle
// steps inside the 16-lane group.  HBM-bound: x is read once (and dx written once in the backward).
#include "common.h"

namespace {

__device__ __forceinline__ float group16_sum(float v) {
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}
__device__ __forceinline__ float group16_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 8)); v = fmaxf(v, __shfl_xor(v, 4)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 1));
    return v;
}

// block = 4 waves = 16 consecutive points of one cloud; every wave walks all channels of its 4 points
template <bool BWD>
__global__ __launch_bounds__(256) void anchor_attn_pool_kernel(int c, int n, int na, float temperature,
                                                              const float *__restrict__ x, const float *__restrict__ logits,
                                                              const float *__restrict__ g, float *__restrict__ out,
                                                              float *__restrict__ conf_out, float *__restrict__ dx,
                                                              float *__restrict__ dlogits) {
    const int bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pt = blockIdx.x * 16 + wave * 4 + (lane >> 4), quad = lane & 15, nq = na >> 2;
    const bool on = pt < n && quad < nq;
    const size_t row = ((size_t)bi * n + min(pt, n - 1)) * na + 4 * min(quad, nq - 1);
    // softmax over the anchors of this point
    float4 l = *reinterpret_cast<const float4 *>(logits + row);
    l.x *= temperature; l.y *= temperature; l.z *= temperature; l.w *= temperature;
    const float neg = -3.0e38f;
    if (quad >= nq) l = make_float4(neg, neg, neg, neg);
    const float m = group16_max(fmaxf(fmaxf(l.x, l.y), fmaxf(l.z, l.w)));
    float4 e = make_float4(__expf(l.x - m), __expf(l.y - m), __expf(l.z - m), __expf(l.w - m));
    if (quad >= nq) e = make_float4(0.f, 0.f, 0.f, 0.f);
    const float inv = 1.0f / group16_sum(e.x + e.y + e.z + e.w);
    const float4 cf = make_float4(e.x * inv, e.y * inv, e.z * inv, e.w * inv);
    if (!BWD && on && conf_out) *reinterpret_cast<float4 *>(conf_out + row) = cf;
    const size_t cs = (size_t)n * na;                        // channel stride of x
    const float *xp = x + (size_t)bi * c * cs + ((size_t)min(pt, n - 1) * na + 4 * min(quad, nq - 1));
    if (!BWD) {
        float *op = out + (size_t)bi * c * n + min(pt, n - 1);
        for (int ci = 0; ci < c; ++ci) {
            const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)ci * cs);
            const float s = group16_sum(quad < nq ? v.x * cf.x + v.y * cf.y + v.z * cf.z + v.w * cf.w : 0.f);
            if (on && quad == 0) op[(size_t)ci * n] = s;
        }
    } else {
        const float *gp = g + (size_t)bi * c * n + min(pt, n - 1);
        float *dxp = dx + (size_t)bi * c * cs + ((size_t)min(pt, n - 1) * na + 4 * min(quad, nq - 1));
        float4 dc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ci = 0; ci < c; ++ci) {
            const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)ci * cs);
            const float gv = gp[(size_t)ci * n];
            dc.x = fmaf(gv, v.x, dc.x); dc.y = fmaf(gv, v.y, dc.y); dc.z = fmaf(gv, v.z, dc.z); dc.w = fmaf(gv, v.w, dc.w);
            if (on) *reinterpret_cast<float4 *>(dxp + (size_t)ci * cs) = make_float4(gv * cf.x, gv * cf.y, gv * cf.z, gv * cf.w);
        }
        // softmax backward: dlogit = T conf (dconf - sum_a conf dconf)
        const float s = group16_sum(quad < nq ? cf.x * dc.x + cf.y * dc.y + cf.z * dc.z + cf.w * dc.w : 0.f);
        if (on) *reinterpret_cast<float4 *>(dlogits + row) = make_float4(temperature * cf.x * (dc.x - s), temperature * cf.y * (dc.y - s),
                                                                         temperature * cf.z * (dc.z - s), temperature * cf.w * (dc.w - s));
    }
}

constexpr int MAXS = 8;     // slots per launch

// forward: block = (channel, cloud); 4 waves stride over the points, 4 points per wave-iteration; per slot one
// float4 accumulator per lane; the 4 point groups and 4 waves are folded through LDS at the end (fixed order)
__global__ __launch_bounds__(256) void slot_mean_fwd_kernel(int c, int n, int na, int ns, const float *__restrict__ x,
                                                            const float *__restrict__ m, const float *__restrict__ inv_den,
                                                            float *__restrict__ out) {
    __shared__ float4 s_part[MAXS][16][16];                   // [slot][wave * 4 + point group][quad]
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, quad = lane & 15, nq = na >> 2;
    float4 acc[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *xp = x + ((size_t)bi * c + ci) * n * na + 4 * min(quad, nq - 1);
    const float *mp = m + (size_t)bi * ns * n;
    for (int p0 = wave * 4 + grp; p0 < n; p0 += 16) {
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p0 * na);
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) {
                const float w = mp[(size_t)s * n + p0];
                acc[s].x = fmaf(w, v.x, acc[s].x); acc[s].y = fmaf(w, v.y, acc[s].y);
                acc[s].z = fmaf(w, v.z, acc[s].z); acc[s].w = fmaf(w, v.w, acc[s].w);
            }
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < ns) s_part[s][wave * 4 + grp][quad] = acc[s];
    __syncthreads();
    for (int e = threadIdx.x; e < ns * nq; e += 256) {
        const int s = e / nq, q = e - s * nq;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < 16; ++j) { const float4 u = s_part[s][j][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float d = inv_den[(size_t)bi * ns + s];
        *reinterpret_cast<float4 *>(out + (((size_t)bi * ns + s) * c + ci) * na + 4 * q) = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
    }
}

// backward w.r.t. x: dx[b,c,n,a] = sum_s g[b,s,c,a] m[b,s,n] inv_den[b,s]
__global__ __launch_bounds__(256) void slot_mean_bwd_kernel(int c, int n, int na, int ns, const float *__restrict__ g,
                                                            const float *__restrict__ m, const float *__restrict__ inv_den,
                                                            float *__restrict__ dx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, quad = lane & 15, nq = na >> 2;
    float4 gv[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        gv[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < ns && quad < nq) {
            const float d = inv_den[(size_t)bi * ns + s];
            const float4 t = *reinterpret_cast<const float4 *>(g + (((size_t)bi * ns + s) * c + ci) * na + 4 * quad);
            gv[s] = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
        }
    }
    float *dp = dx + ((size_t)bi * c + ci) * n * na + 4 * min(quad, nq - 1);
    const float *mp = m + (size_t)bi * ns * n;
    for (int p0 = wave * 4 + grp; p0 < n; p0 += 16) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) {
                const float w = mp[(size_t)s * n + p0];
                t.x = fmaf(w, gv[s].x, t.x); t.y = fmaf(w, gv[s].y, t.y); t.z = fmaf(w, gv[s].z, t.z); t.w = fmaf(w, gv[s].w, t.w);
            }
        if (quad < nq) *reinterpret_cast<float4 *>(dp + (size_t)p0 * na) = t;
    }
}

// masked max over the points, the pose head's 'max' pooling on a point subset (`(x * mask).max(2)`: SO3OutBlockRWithMask /
// SO3OutBlockRTWithMaskSep with pooling_method = 'max', SPConvNets/models/model_utils.py:L79-80, L470-484): out[b,c,a] = max_p
// mask[b,p] * x[b,c,p,a] and the point that attains it (the lowest index among equals: deterministic).  One pass over x.
// A product that is NaN (a NaN or mask 0 times an infinity in x, whatever the mask) is the result, as torch's max gives it, and arg the
// lowest point with such a product: a diverged map must not pool to a finite number.  -0.0 and +0.0 are equals.
// block = (channel, cloud); lane = (point group of 4, anchor quad); groups and waves are folded through LDS in a fixed order
__device__ __forceinline__ bool max_takes(float a, float best) {          // within a lane's ascending chain: larger, or the first NaN
    return a > best || (a != a && best == best);
}
__device__ __forceinline__ bool max_takes(float u, int k, float best, int at) {      // between chains: ... or equal at a lower point
    const bool un = u != u, bn = best != best;
    return (un || bn) ? (un && (!bn || k < at)) : (u > best || (u == best && k < at));
}

__global__ __launch_bounds__(256) void masked_max_fwd_kernel(int c, int n, int na, const float *__restrict__ x, const float *__restrict__ m,
                                                             float *__restrict__ out, int32_t *__restrict__ arg) {
    __shared__ float4 s_val[16][16];
    __shared__ int4 s_idx[16][16];
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, quad = lane & 15, nq = na >> 2;
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int4 at = make_int4(0, 0, 0, 0);
    const float *xp = x + ((size_t)bi * c + ci) * n * na + 4 * min(quad, nq - 1);
    const float *mp = m + (size_t)bi * n;
    for (int p0 = wave * 4 + grp; p0 < n; p0 += 16) {                      // ascending within a lane: ">" keeps the first of equals
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p0 * na);
        const float w = mp[p0];
        const float a0 = w * v.x, a1 = w * v.y, a2 = w * v.z, a3 = w * v.w;
        if (max_takes(a0, best.x)) { best.x = a0; at.x = p0; }
        if (max_takes(a1, best.y)) { best.y = a1; at.y = p0; }
        if (max_takes(a2, best.z)) { best.z = a2; at.z = p0; }
        if (max_takes(a3, best.w)) { best.w = a3; at.w = p0; }
    }
    s_val[wave * 4 + grp][quad] = best;
    s_idx[wave * 4 + grp][quad] = at;
    __syncthreads();
    if (threadIdx.x < nq) {
        const int q = threadIdx.x;
        float4 bv = s_val[0][q];
        int4 bi4 = s_idx[0][q];
        for (int j = 1; j < 16; ++j) {
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
__global__ __launch_bounds__(256) void masked_max_bwd_kernel(int c, int n, int na, const float *__restrict__ g, const int32_t *__restrict__ arg,
                                                             const float *__restrict__ m, float *__restrict__ dx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, quad = lane & 15, nq = na >> 2;
    if (quad >= nq) return;
    const float4 gv = *reinterpret_cast<const float4 *>(g + ((size_t)bi * c + ci) * na + 4 * quad);
    const int4 at = *reinterpret_cast<const int4 *>(arg + ((size_t)bi * c + ci) * na + 4 * quad);
    float *dp = dx + ((size_t)bi * c + ci) * n * na + 4 * quad;
    const float *mp = m + (size_t)bi * n;
    for (int p0 = wave * 4 + grp; p0 < n; p0 += 16) {
        const float w = mp[p0];
        *reinterpret_cast<float4 *>(dp + (size_t)p0 * na) =
            make_float4(p0 == at.x ? w * gv.x : 0.f, p0 == at.y ? w * gv.y : 0.f, p0 == at.z ? w * gv.z : 0.f, p0 == at.w ? w * gv.w : 0.f);
    }
}

// ---- BatchNorm2d + leaky_relu + weighted point mean in one pass: the last unary layer of InvOutBlockOursWithMask and the point
// average behind it (SPConvNets/utils/base_so3conv.py:L1076-1107; between that ReLU and the average the reference's pointnet stage
// is linear, so the average moves in front of it and the activated [b,c,n,a] map is never needed):
//     out[b,c,a] = inv_den[b] sum_p w[b,p] leaky(x[b,c,p,a] scale[b,c] + shift[b,c])
// block = (channel, cloud); lane = (point group of 4, anchor quad) as above.  A lane takes PM_UNROLL points per loop trip into as
// many accumulators (independent loads in flight, fp32 chains of n / 64 terms); accumulators, point groups and waves are folded in a
// fixed order: bit-identical run to run.  Points past n re-read point n - 1 with weight 0.
constexpr int PM_UNROLL = 4;
constexpr int PM_PARTS = 16;            // partial sums per (cloud, channel) the backward reduction leaves: 4 waves x 4 point groups
constexpr int PM_APPLY_PTS = 512;       // points per block of the backward apply

__device__ __forceinline__ float leaky(float pre, float slope) { return pre > 0.f ? pre : pre * slope; }

__global__ __launch_bounds__(256) void bn_act_mean_fwd_kernel(int c, int n, int na, float slope, const float *__restrict__ x,
                                                              const float *__restrict__ scale, const float *__restrict__ shift,
                                                              const float *__restrict__ w, const float *__restrict__ inv_den,
                                                              float *__restrict__ out) {
    __shared__ float4 s_part[16][16];                         // [wave * 4 + point group][quad]
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, quad = lane & 15, nq = na >> 2;
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si];
    const float *xp = x + si * n * na + 4 * min(quad, nq - 1);
    const float *wp = w + (size_t)bi * n;
    float4 acc[PM_UNROLL];
#pragma unroll
    for (int u = 0; u < PM_UNROLL; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p0 = wave * 4 + grp; p0 < n; p0 += 16 * PM_UNROLL) {
        float4 v[PM_UNROLL];
        float wv[PM_UNROLL];
#pragma unroll
        for (int u = 0; u < PM_UNROLL; ++u) {
            const int p = p0 + 16 * u, pc = min(p, n - 1);
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
    s_part[wave * 4 + grp][quad] = make_float4((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y),
                                               (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z), (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w));
    __syncthreads();
    if (threadIdx.x < nq) {
        const int q = threadIdx.x;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < 16; ++j) { const float4 u = s_part[j][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        const float d = inv_den[bi];
        *reinterpret_cast<float4 *>(out + si * na + 4 * q) = make_float4(t.x * d, t.y * d, t.z * d, t.w * d);
    }
}

// backward, reduction pass: with gg = (pre > 0 ? 1 : slope) w[b,p] inv_den[b] g[b,c,a] (the gradient the unfused composition would
// broadcast to [b,c,n,a] and read back), the sums of gg and gg xhat over the points and anchors of a (cloud, channel) row as PM_PARTS
// partials [b][c][wave * 4 + point group], for the caller to add in float64
__global__ __launch_bounds__(256) void bn_act_mean_bwd_reduce_kernel(int c, int n, int na, float slope, const float *__restrict__ g,
                                                                     const float *__restrict__ x, const float *__restrict__ scale,
                                                                     const float *__restrict__ shift, const float *__restrict__ mean,
                                                                     const float *__restrict__ invstd, const float *__restrict__ w,
                                                                     const float *__restrict__ inv_den, float *__restrict__ pg,
                                                                     float *__restrict__ pgx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, quad = lane & 15, nq = na >> 2;
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si], mu = mean[si], is = invstd[si], d = inv_den[bi];
    float4 gq = *reinterpret_cast<const float4 *>(g + si * na + 4 * min(quad, nq - 1));
    gq = make_float4(gq.x * d, gq.y * d, gq.z * d, gq.w * d);
    const float *xp = x + si * n * na + 4 * min(quad, nq - 1);
    const float *wp = w + (size_t)bi * n;
    float s[PM_UNROLL], q[PM_UNROLL];
#pragma unroll
    for (int u = 0; u < PM_UNROLL; ++u) s[u] = q[u] = 0.f;
    for (int p0 = wave * 4 + grp; p0 < n; p0 += 16 * PM_UNROLL) {
        float4 v[PM_UNROLL];
        float wv[PM_UNROLL];
#pragma unroll
        for (int u = 0; u < PM_UNROLL; ++u) {
            const int p = p0 + 16 * u, pc = min(p, n - 1);
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
    const bool live = quad < nq;                              // an idle lane re-read the last quad
    const float ts = group16_sum(live ? (s[0] + s[1]) + (s[2] + s[3]) : 0.f), tq = group16_sum(live ? (q[0] + q[1]) + (q[2] + q[3]) : 0.f);
    if (quad == 0) {
        pg[si * PM_PARTS + wave * 4 + grp] = ts;
        pgx[si * PM_PARTS + wave * 4 + grp] = tq;
    }
}

// backward, apply pass: gx = scale gg - stat_mask (k2 + xhat k3), the formula of bn_act_bwd_apply_kernel<CLOUD> (csrc/bn_act.hip) on the gradient
// formed in registers.  block = (channel, cloud, PM_APPLY_PTS points)
__global__ __launch_bounds__(256) void bn_act_mean_bwd_apply_kernel(int c, int n, int na, float slope, const float *__restrict__ g,
                                                                    const float *__restrict__ x, const float *__restrict__ scale,
                                                                    const float *__restrict__ shift, const float *__restrict__ mean,
                                                                    const float *__restrict__ invstd, const float *__restrict__ k2,
                                                                    const float *__restrict__ k3, const float *__restrict__ w,
                                                                    const float *__restrict__ inv_den, const float *__restrict__ stat_mask,
                                                                    float *__restrict__ gx) {
    const int ci = blockIdx.x, bi = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, quad = lane & 15, nq = na >> 2;
    if (quad >= nq) return;
    const size_t si = (size_t)bi * c + ci;
    const float sc = scale[si], sh = shift[si], mu = mean[si], is = invstd[si], c2 = k2[si], c3 = k3[si], d = inv_den[bi];
    float4 gq = *reinterpret_cast<const float4 *>(g + si * na + 4 * quad);
    gq = make_float4(gq.x * d, gq.y * d, gq.z * d, gq.w * d);
    const float *xp = x + si * n * na + 4 * quad;
    float *op = gx + si * n * na + 4 * quad;
    const float *wp = w + (size_t)bi * n;
    const float *mp = stat_mask ? stat_mask + (size_t)bi * n : nullptr;
    const int first = blockIdx.z * PM_APPLY_PTS, last = min(n, first + PM_APPLY_PTS);
    auto one = [&](float gv, float xv, float wv, float m) {
        const float gg = (fmaf(xv, sc, sh) > 0.f ? gv : gv * slope) * wv;
        return fmaf(-m, fmaf((xv - mu) * is, c3, c2), gg * sc);
    };
    for (int p = first + wave * 4 + grp; p < last; p += 16) {
        const float4 v = *reinterpret_cast<const float4 *>(xp + (size_t)p * na);
        const float wv = wp[p], m = mp ? mp[p] : 1.f;
        *reinterpret_cast<float4 *>(op + (size_t)p * na) = make_float4(one(gq.x, v.x, wv, m), one(gq.y, v.y, wv, m), one(gq.z, v.z, wv, m), one(gq.w, v.w, wv, m));
    }
}

inline int point_mean_dims(const char *who, int na, const void *p0, const void *p1, const void *p2) {
    char buf[200];
    if (na <= 0 || na > 64 || (na & 3) != 0) {
        snprintf(buf, sizeof(buf), "%s: anchors must be a multiple of 4, at most 64", who);
        return eap::bad_arg(buf);
    }
    if (((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2)) & 15) != 0) {
        snprintf(buf, sizeof(buf), "%s: the [b,c,n,na] and [b,c,na] tensors must be 16-byte aligned", who);
        return eap::bad_arg(buf);
    }
    return 0;
}

// the three older pairs: anchor rows of 16-byte words (and at most MAXS slots), every tensor a kernel reads or writes by float4 / int4 on a
// 16-byte boundary (`which` names them in the message)
inline int head_args(const char *who, int na, int ns, const char *which, const void *p0, const void *p1, const void *p2 = nullptr,
                     const void *p3 = nullptr) {
    char buf[240];
    if (na <= 0 || na > 64 || (na & 3) != 0 || ns > MAXS) {
        snprintf(buf, sizeof(buf), "%s: anchors must be a multiple of 4, at most 64%s", who, ns > 0 ? "; at most 8 slots" : "");
        return eap::bad_arg(buf);
    }
    if (((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2) | reinterpret_cast<uintptr_t>(p3)) & 15) != 0) {
        snprintf(buf, sizeof(buf), "%s: %s must be 16-byte aligned", who, which);
        return eap::bad_arg(buf);
    }
    return 0;
}

}  // namespace

extern "C" int eap_anchor_attn_pool_fwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                            float *out, float *conf, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = head_args("anchor_attn_pool_fwd", na, 0, "x, logits and conf", x, logits, conf)) return e;
    return eap::run_kernel("anchor_attn_pool_fwd", anchor_attn_pool_kernel<false>, eap::cdiv(n, 16), b, 1, dim3(256), 0, eap::S(stream), c, n, na, temperature, x,
                           logits, nullptr, out, conf, nullptr, nullptr);
}

extern "C" int eap_anchor_attn_pool_bwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                            const float *g, float *dx, float *dlogits, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = head_args("anchor_attn_pool_bwd", na, 0, "x, logits, dx and dlogits", x, logits, dx, dlogits)) return e;
    return eap::run_kernel("anchor_attn_pool_bwd", anchor_attn_pool_kernel<true>, eap::cdiv(n, 16), b, 1, dim3(256), 0, eap::S(stream), c, n, na, temperature, x,
                           logits, g, nullptr, nullptr, dx, dlogits);
}

extern "C" int eap_slot_masked_mean_fwd_f32(int b, int ns, int c, int n, int na, const float *x, const float *mask,
                                            const float *inv_den, float *out, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0 || ns <= 0) return 0;
    if (int e = head_args("slot_masked_mean_fwd", na, ns, "x and out", x, out)) return e;
    return eap::run_kernel("slot_masked_mean_fwd", slot_mean_fwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, ns, x, mask, inv_den, out);
}

extern "C" int eap_slot_masked_mean_bwd_f32(int b, int ns, int c, int n, int na, const float *g, const float *mask,
                                            const float *inv_den, float *dx, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0 || ns <= 0) return 0;
    if (int e = head_args("slot_masked_mean_bwd", na, ns, "g and dx", g, dx)) return e;
    return eap::run_kernel("slot_masked_mean_bwd", slot_mean_bwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, ns, g, mask, inv_den, dx);
}

extern "C" int eap_masked_max_fwd_f32(int b, int c, int n, int na, const float *x, const float *mask, float *out, int32_t *arg,
                                      eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("masked_max_fwd: no points");
    if (int e = head_args("masked_max_fwd", na, 0, "x, out and arg", x, out, arg)) return e;
    return eap::run_kernel("masked_max_fwd", masked_max_fwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, x, mask, out, arg);
}

extern "C" int eap_masked_max_bwd_f32(int b, int c, int n, int na, const float *g, const int32_t *arg, const float *mask, float *dx,
                                      eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (int e = head_args("masked_max_bwd", na, 0, "g, arg and dx", g, arg, dx)) return e;
    return eap::run_kernel("masked_max_bwd", masked_max_bwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, g, arg, mask, dx);
}

// ---- BatchNorm2d + leaky_relu + weighted point mean (InvOutBlockOursWithMask, SPConvNets/utils/base_so3conv.py:L1076-1107) ----
extern "C" int eap_bn_act_cloud_mean_parts(int n) { return n > 0 ? PM_PARTS : 0; }

extern "C" int eap_bn_act_cloud_mean_fwd_f32(int b, int c, int n, int na, float slope, const float *x, const float *scale, const float *shift,
                                             const float *w, const float *inv_den, float *out, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("bn_act_cloud_mean_fwd: no points");
    if (int e = point_mean_dims("bn_act_cloud_mean_fwd", na, x, out, nullptr)) return e;
    return eap::run_kernel("bn_act_cloud_mean_fwd", bn_act_mean_fwd_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, slope, x, scale, shift, w,
                           inv_den, out);
}

extern "C" int eap_bn_act_cloud_mean_bwd_reduce_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                    const float *shift, const float *mean, const float *invstd, const float *w,
                                                    const float *inv_den, float *pg, float *pgx, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("bn_act_cloud_mean_bwd_reduce: no points");
    if (int e = point_mean_dims("bn_act_cloud_mean_bwd_reduce", na, x, g, nullptr)) return e;
    return eap::run_kernel("bn_act_cloud_mean_bwd_reduce", bn_act_mean_bwd_reduce_kernel, c, b, 1, dim3(256), 0, eap::S(stream), c, n, na, slope, g, x,
                           scale, shift, mean, invstd, w, inv_den, pg, pgx);
}

extern "C" int eap_bn_act_cloud_mean_bwd_apply_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                                   const float *shift, const float *mean, const float *invstd, const float *k2, const float *k3,
                                                   const float *w, const float *inv_den, const float *stat_mask, float *gx, eap_stream_t stream) {
    if (b <= 0 || c <= 0) return 0;
    if (n <= 0) return eap::bad_arg("bn_act_cloud_mean_bwd_apply: no points");
    if (int e = point_mean_dims("bn_act_cloud_mean_bwd_apply", na, x, g, gx)) return e;
    return eap::run_kernel("bn_act_cloud_mean_bwd_apply", bn_act_mean_bwd_apply_kernel, c, b, eap::cdiv(n, PM_APPLY_PTS), dim3(256), 0, eap::S(stream), c,
                           n, na, slope, g, x, scale, shift, mean, invstd, k2, k3, w, inv_den, stat_mask, gx);
}
