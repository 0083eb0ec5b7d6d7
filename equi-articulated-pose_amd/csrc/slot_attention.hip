// csrc/slot_attention.hip -- the per-point passes of SlotAttention (SPConvNets/utils/slot_attention_spec_v2.py:L132-193), the model's
// segmentation step (SPConvNets/models/unsup_seg_so3_pose_conv_pn_38_multi_stage.py:L142, L621), without the per-slot [b,s,n,d] key
// and value tensors the reference writes (L149-154) and reads again in every iteration (L167, L175).
//
// The per-slot LayerNorm (L149), to_k / to_v (L153-154) and the two einsums (L167, L175) are linear in z[n] = (x[n] - mean_n) rstd_n,
// which is the same for every slot:
//     dots[s,n]  = z[n] . u_s + c0_s            u_s = scale g_s o (Wk_s^T q_s),  c0_s = scale q_s . (Wk_s beta_s + bk_s)
//     updates_s  = Wv_s (g_s o m_s + beta_s) + bv_s,   m_s = sum_n attn_ori[s,n] z[n] / sum_n attn_ori[s,n]
// so one iteration is two passes over x (scores, pool) and a few [b,s,d] operations the caller keeps in torch.
//
// x is channel-major [b,d,n] (what InvPPOutBlockOurs returns).  Mapping: lanes run along the points, a lane owns V consecutive points
// (V = 4, one 16-byte word per channel, where n % 4 == 0 and every tensor moved that way is 16-byte aligned; V = 1 otherwise); the
// [b,s,d] operands are indexed by block and loop counters only (wave-uniform reads).  The per-point kernels split the channels over
// the 4 waves of a block and fold the 4 partial sums through LDS in wave order; the pool kernel keeps 8 channels x s slots of
// accumulators per lane and leaves one partial per 1024 points for the caller to add in float64.  No atomics: bit-identical run to run.
#include <initializer_list>

#include "common.h"

namespace {

constexpr int MAXS = 8;                // slots per launch (as csrc/heads.hip)
constexpr int MAXJ = 2 * MAXS;         // outer products per launch of the input-gradient kernel
constexpr int WAVES = 4;
constexpr int POOL_CH = 8;             // channels a pool block keeps accumulators for: a weight is read once and used 8 times
constexpr int POOL_PTS = 1024;         // points per partial of the pool kernel

template <int V>
__device__ __forceinline__ void load_v(const float *p, float (&o)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        o[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_v(float *p, const float (&o)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(o[0], o[1], o[2], o[3]);
    else *p = o[0];
}

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ float wave_sum(float v) {
    v += __shfl_xor(v, 32); v += __shfl_xor(v, 16); v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}

// ---- mean and rstd over the d channels of a point, two passes (slot_attention_spec_v2.py:L149, nn.LayerNorm's statistics) ------
// block = 64 V points of one cloud; wave w takes channels w, w + 4, ...
template <int V>
__global__ __launch_bounds__(256) void slot_stats_kernel(int d, int n, float ln_eps, const float *__restrict__ x, float *__restrict__ mean,
                                                         float *__restrict__ rstd) {
    __shared__ float s_red[WAVES][64 * V];
    const int bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_id();
    const int p0 = (blockIdx.x * 64 + lane) * V, pc = min(p0, n - V);
    const float *xp = x + (size_t)bi * d * n + pc;
    float acc[V], t[V], mu[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll 4
    for (int c = wave; c < d; c += WAVES) {
        load_v<V>(xp + (size_t)c * n, t);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += t[v];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) s_red[wave][lane * V + v] = acc[v];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = lane * V + v;
        mu[v] = (((s_red[0][i] + s_red[1][i]) + s_red[2][i]) + s_red[3][i]) / (float)d;
        acc[v] = 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int c = wave; c < d; c += WAVES) {
        load_v<V>(xp + (size_t)c * n, t);
#pragma unroll
        for (int v = 0; v < V; ++v) { const float e = t[v] - mu[v]; acc[v] = fmaf(e, e, acc[v]); }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) s_red[wave][lane * V + v] = acc[v];
    __syncthreads();
    if (wave == 0 && p0 < n) {
        float r[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int i = lane * V + v;
            r[v] = 1.0f / sqrtf((((s_red[0][i] + s_red[1][i]) + s_red[2][i]) + s_red[3][i]) / (float)d + ln_eps);
        }
        store_v<V>(mean + (size_t)bi * n + p0, mu);
        store_v<V>(rstd + (size_t)bi * n + p0, r);
    }
}

// ---- per point the s products z . vec_s + off_s, then the softmax over the slots (forward, L167-169) or its backward ------------
// forward:  vec = u, off = c0;  attn[s,n] = softmax_s(dots)[s,n] + eps                                        (written)
// backward: vec = gmsum, off = gwsum;  gattn = gattn_in + z . gmsum_s + gwsum_s (the pool's backward, L172-175, folded in),
//           p = attn - eps, gdots[s,n] = p (gattn - sum_s p gattn)                                            (written to `out`)
// block = 64 V points of one cloud; wave w takes channels w, w + 4, ...; the epilogue runs one thread per point
template <int V, bool BWD>
__global__ __launch_bounds__(256) void slot_scores_kernel(int d, int n, int ns, float eps, const float *__restrict__ x,
                                                          const float *__restrict__ mean, const float *__restrict__ rstd,
                                                          const float *__restrict__ vec, const float *__restrict__ off,
                                                          const float *__restrict__ gattn_in, const float *__restrict__ attn_in,
                                                          float *__restrict__ out) {
    __shared__ float s_part[WAVES][MAXS][64 * V];
    const int bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_id();
    const int base = blockIdx.x * 64 * V, p0 = base + lane * V, pc = min(p0, n - V);
    const float *xp = x + (size_t)bi * d * n + pc;
    const float *vp = vec + (size_t)bi * ns * d;
    float mu[V], rs[V], t[V], acc[MAXS][V];
    load_v<V>(mean + (size_t)bi * n + pc, mu);
    load_v<V>(rstd + (size_t)bi * n + pc, rs);
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[s][v] = 0.f;
#pragma unroll 2
    for (int c = wave; c < d; c += WAVES) {
        load_v<V>(xp + (size_t)c * n, t);
#pragma unroll
        for (int v = 0; v < V; ++v) t[v] = (t[v] - mu[v]) * rs[v];
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) {
                const float w = vp[(size_t)s * d + c];
#pragma unroll
                for (int v = 0; v < V; ++v) acc[s][v] = fmaf(t[v], w, acc[s][v]);
            }
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < ns) {
#pragma unroll
            for (int v = 0; v < V; ++v) s_part[wave][s][lane * V + v] = acc[s][v];
        }
    __syncthreads();
    const int i = threadIdx.x, p = base + i;
    if (i >= 64 * V || p >= n) return;
    float val[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        val[s] = s < ns ? (((s_part[0][s][i] + s_part[1][s][i]) + s_part[2][s][i]) + s_part[3][s][i]) + off[(size_t)bi * ns + s] : 0.f;
    const size_t row = (size_t)bi * ns * n + p;
    if (!BWD) {
        float m = val[0];
#pragma unroll
        for (int s = 1; s < MAXS; ++s)
            if (s < ns) m = fmaxf(m, val[s]);
        float den = 0.f;
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) { val[s] = expf(val[s] - m); den += val[s]; }
        const float inv = 1.0f / den;
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) out[row + (size_t)s * n] = val[s] * inv + eps;
    } else {
        float pr[MAXS], dot = 0.f;
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) {
                pr[s] = attn_in[row + (size_t)s * n] - eps;
                if (gattn_in) val[s] += gattn_in[row + (size_t)s * n];
                dot = fmaf(pr[s], val[s], dot);
            }
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) out[row + (size_t)s * n] = pr[s] * (val[s] - dot);
    }
}

// ---- msum[s,c] = sum_n w[s,n] z[n,c], wsum[s] = sum_n w[s,n] as one partial per POOL_PTS points (L172-175; the backward's dL/du, dL/dc0):
// psum[b,part,s,0..d-1] = msum, psum[b,part,s,d] = wsum, one tensor for the caller to add over the parts ----
// block = (POOL_PTS points, POOL_CH channels, cloud); a thread walks its points 256 V apart and keeps ns x POOL_CH accumulators;
// lanes are folded by shuffles, waves through LDS, both in a fixed order
template <int V>
__global__ __launch_bounds__(256) void slot_pool_kernel(int d, int n, int ns, const float *__restrict__ x, const float *__restrict__ mean,
                                                        const float *__restrict__ rstd, const float *__restrict__ w,
                                                        float *__restrict__ psum) {
    __shared__ float s_red[WAVES][MAXS][POOL_CH + 1];
    const int part = blockIdx.x, c0 = blockIdx.y * POOL_CH, bi = blockIdx.z, lane = threadIdx.x & 63, wave = wave_id();
    const int last = min(n, (part + 1) * POOL_PTS);
    const float *xp = x + ((size_t)bi * d + c0) * n;
    const float *wp = w + (size_t)bi * ns * n;
    float acc[MAXS][POOL_CH + 1];                            // [.][POOL_CH]: the sum of the weights
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
#pragma unroll
        for (int k = 0; k <= POOL_CH; ++k) acc[s][k] = 0.f;
    for (int p = part * POOL_PTS + (int)threadIdx.x * V; p < last; p += 256 * V) {
        float mu[V], rs[V], wv[MAXS][V], t[V];
        load_v<V>(mean + (size_t)bi * n + p, mu);
        load_v<V>(rstd + (size_t)bi * n + p, rs);
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < ns) {
                load_v<V>(wp + (size_t)s * n + p, wv[s]);
#pragma unroll
                for (int v = 0; v < V; ++v) acc[s][POOL_CH] += wv[s][v];
            }
#pragma unroll
        for (int k = 0; k < POOL_CH; ++k)
            if (c0 + k < d) {
                load_v<V>(xp + (size_t)k * n + p, t);
#pragma unroll
                for (int v = 0; v < V; ++v) t[v] = (t[v] - mu[v]) * rs[v];
#pragma unroll
                for (int s = 0; s < MAXS; ++s)
                    if (s < ns) {
#pragma unroll
                        for (int v = 0; v < V; ++v) acc[s][k] = fmaf(wv[s][v], t[v], acc[s][k]);
                    }
            }
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < ns) {
#pragma unroll
            for (int k = 0; k <= POOL_CH; ++k) {
                const float r = wave_sum(acc[s][k]);
                if (lane == 0) s_red[wave][s][k] = r;
            }
        }
    __syncthreads();
    const int e = threadIdx.x;
    if (e >= ns * (POOL_CH + 1)) return;
    const int s = e / (POOL_CH + 1), k = e - s * (POOL_CH + 1);
    const float r = ((s_red[0][s][k] + s_red[1][s][k]) + s_red[2][s][k]) + s_red[3][s][k];
    float *row = psum + (((size_t)bi * gridDim.x + part) * ns + s) * (d + 1);
    if (k == POOL_CH) { if (blockIdx.y == 0) row[d] = r; }
    else if (c0 + k < d) row[c0 + k] = r;
}

// ---- the gradient reaching x through z (the LayerNorm statistics' backward, L149) -------------------------------------------------
// gz[n,c] = sum_j rows[j,n] vecs[j,c] (never written);  gx[c,n] = rstd_n (gz[n,c] - mean_c gz[n,.] - z[n,c] mean_c (gz[n,.] z[n,.]))
// block = 64 V points of one cloud; wave w takes channels w, w + 4, ... in both passes
template <int V>
__global__ __launch_bounds__(256) void slot_input_grad_kernel(int d, int n, int nj, const float *__restrict__ x, const float *__restrict__ mean,
                                                              const float *__restrict__ rstd, const float *__restrict__ rows,
                                                              const float *__restrict__ vecs, float *__restrict__ gx) {
    __shared__ float s_red[2][WAVES][64 * V];
    const int bi = blockIdx.y, lane = threadIdx.x & 63, wave = wave_id();
    const int p0 = (blockIdx.x * 64 + lane) * V, pc = min(p0, n - V);
    const float *xp = x + (size_t)bi * d * n + pc;
    const float *vp = vecs + (size_t)bi * nj * d;
    float mu[V], rs[V], r[MAXJ][V], t[V], sa[V], sb[V];
    load_v<V>(mean + (size_t)bi * n + pc, mu);
    load_v<V>(rstd + (size_t)bi * n + pc, rs);
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
        if (j < nj) load_v<V>(rows + ((size_t)bi * nj + j) * n + pc, r[j]);
#pragma unroll
    for (int v = 0; v < V; ++v) sa[v] = sb[v] = 0.f;
    for (int c = wave; c < d; c += WAVES) {
        load_v<V>(xp + (size_t)c * n, t);
        float g[V];
#pragma unroll
        for (int v = 0; v < V; ++v) g[v] = 0.f;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (j < nj) {
                const float w = vp[(size_t)j * d + c];
#pragma unroll
                for (int v = 0; v < V; ++v) g[v] = fmaf(r[j][v], w, g[v]);
            }
#pragma unroll
        for (int v = 0; v < V; ++v) { sa[v] += g[v]; sb[v] = fmaf(g[v], (t[v] - mu[v]) * rs[v], sb[v]); }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) { s_red[0][wave][lane * V + v] = sa[v]; s_red[1][wave][lane * V + v] = sb[v]; }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = lane * V + v;
        sa[v] = (((s_red[0][0][i] + s_red[0][1][i]) + s_red[0][2][i]) + s_red[0][3][i]) / (float)d;
        sb[v] = (((s_red[1][0][i] + s_red[1][1][i]) + s_red[1][2][i]) + s_red[1][3][i]) / (float)d;
    }
    if (p0 >= n) return;
    float *gp = gx + (size_t)bi * d * n + p0;
    for (int c = wave; c < d; c += WAVES) {
        load_v<V>(xp + (size_t)c * n, t);
        float g[V];
#pragma unroll
        for (int v = 0; v < V; ++v) g[v] = 0.f;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (j < nj) {
                const float w = vp[(size_t)j * d + c];
#pragma unroll
                for (int v = 0; v < V; ++v) g[v] = fmaf(r[j][v], w, g[v]);
            }
#pragma unroll
        for (int v = 0; v < V; ++v) g[v] = rs[v] * ((g[v] - sa[v]) - (t[v] - mu[v]) * rs[v] * sb[v]);
        store_v<V>(gp + (size_t)c * n, g);
    }
}

// sizes every entry shares: any n >= 1, d >= 1, 1 <= s <= 8 (hipErrorInvalidValue with the argument named, before any device call)
inline int slot_dims(const char *who, int b, int n, int d, int count, int cap, const char *count_name) {
    char buf[200];
    const char *bad = n < 1 ? "n (points) must be at least 1" : d < 1 ? "d (channels) must be at least 1" : b > 65535 ? "b (clouds) must be at most 65535" : nullptr;
    if (bad) {
        snprintf(buf, sizeof(buf), "%s: %s", who, bad);
        return eap::bad_arg(buf);
    }
    if (count < 1 || count > cap) {
        snprintf(buf, sizeof(buf), "%s: %s must be between 1 and %d, not %d", who, count_name, cap, count);
        return eap::bad_arg(buf);
    }
    return 0;
}

inline int slot_null(const char *who, const char *names, std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (p == nullptr) {
            char buf[240];
            snprintf(buf, sizeof(buf), "%s: a null pointer among %s", who, names);
            return eap::bad_arg(buf);
        }
    return 0;
}

}  // namespace

extern "C" int eap_slot_attn_pool_parts(int n) { return n > 0 ? (int)eap::cdiv(n, POOL_PTS) : 0; }

extern "C" int eap_slot_attn_stats_f32(int b, int d, int n, float ln_eps, const float *x, float *mean, float *rstd, eap_stream_t stream) {
    if (int e = slot_dims("slot_attn_stats", b, n, d, 1, 1, "")) return e;
    if (b <= 0) return 0;
    if (int e = slot_null("slot_attn_stats", "x, mean, rstd", {x, mean, rstd})) return e;
    if (n % 4 == 0 && eap::aligned16(x, mean, rstd))
        return eap::run_kernel("slot_attn_stats", slot_stats_kernel<4>, eap::cdiv(n, 256), b, 1, dim3(256), 0, eap::S(stream), d, n, ln_eps, x, mean, rstd);
    return eap::run_kernel("slot_attn_stats", slot_stats_kernel<1>, eap::cdiv(n, 64), b, 1, dim3(256), 0, eap::S(stream), d, n, ln_eps, x, mean, rstd);
}

extern "C" int eap_slot_attn_scores_fwd_f32(int b, int s, int d, int n, float eps, const float *x, const float *mean, const float *rstd,
                                            const float *u, const float *c0, float *attn, eap_stream_t stream) {
    if (int e = slot_dims("slot_attn_scores_fwd", b, n, d, s, MAXS, "s (slots)")) return e;
    if (b <= 0) return 0;
    if (int e = slot_null("slot_attn_scores_fwd", "x, mean, rstd, u, c0, attn", {x, mean, rstd, u, c0, attn})) return e;
    if (n % 4 == 0 && eap::aligned16(x, mean, rstd))
        return eap::run_kernel("slot_attn_scores_fwd", slot_scores_kernel<4, false>, eap::cdiv(n, 256), b, 1, dim3(256), 0, eap::S(stream), d, n, s, eps, x,
                               mean, rstd, u, c0, nullptr, nullptr, attn);
    return eap::run_kernel("slot_attn_scores_fwd", slot_scores_kernel<1, false>, eap::cdiv(n, 64), b, 1, dim3(256), 0, eap::S(stream), d, n, s, eps, x, mean,
                           rstd, u, c0, nullptr, nullptr, attn);
}

extern "C" int eap_slot_attn_scores_bwd_f32(int b, int s, int d, int n, float eps, const float *x, const float *mean, const float *rstd,
                                            const float *attn, const float *gmsum, const float *gwsum, const float *gattn, float *gdots,
                                            eap_stream_t stream) {
    if (int e = slot_dims("slot_attn_scores_bwd", b, n, d, s, MAXS, "s (slots)")) return e;
    if (b <= 0) return 0;
    if (int e = slot_null("slot_attn_scores_bwd", "x, mean, rstd, attn, gmsum, gwsum, gdots", {x, mean, rstd, attn, gmsum, gwsum, gdots})) return e;
    if (n % 4 == 0 && eap::aligned16(x, mean, rstd))
        return eap::run_kernel("slot_attn_scores_bwd", slot_scores_kernel<4, true>, eap::cdiv(n, 256), b, 1, dim3(256), 0, eap::S(stream), d, n, s, eps, x,
                               mean, rstd, gmsum, gwsum, gattn, attn, gdots);
    return eap::run_kernel("slot_attn_scores_bwd", slot_scores_kernel<1, true>, eap::cdiv(n, 64), b, 1, dim3(256), 0, eap::S(stream), d, n, s, eps, x, mean,
                           rstd, gmsum, gwsum, gattn, attn, gdots);
}

extern "C" int eap_slot_attn_pool_f32(int b, int s, int d, int n, const float *x, const float *mean, const float *rstd, const float *w,
                                      float *psum, eap_stream_t stream) {
    if (int e = slot_dims("slot_attn_pool", b, n, d, s, MAXS, "s (slots)")) return e;
    if (b <= 0) return 0;
    if (int e = slot_null("slot_attn_pool", "x, mean, rstd, w, psum", {x, mean, rstd, w, psum})) return e;
    const long long parts = eap::cdiv(n, POOL_PTS), groups = eap::cdiv(d, POOL_CH);
    if (n % 4 == 0 && eap::aligned16(x, mean, rstd, w))
        return eap::run_kernel("slot_attn_pool", slot_pool_kernel<4>, parts, groups, b, dim3(256), 0, eap::S(stream), d, n, s, x, mean, rstd, w, psum);
    return eap::run_kernel("slot_attn_pool", slot_pool_kernel<1>, parts, groups, b, dim3(256), 0, eap::S(stream), d, n, s, x, mean, rstd, w, psum);
}

extern "C" int eap_slot_attn_input_grad_f32(int b, int j, int d, int n, const float *x, const float *mean, const float *rstd, const float *rows,
                                            const float *vecs, float *gx, eap_stream_t stream) {
    if (int e = slot_dims("slot_attn_input_grad", b, n, d, j, MAXJ, "j (outer products)")) return e;
    if (b <= 0) return 0;
    if (int e = slot_null("slot_attn_input_grad", "x, mean, rstd, rows, vecs, gx", {x, mean, rstd, rows, vecs, gx})) return e;
    if (n % 4 == 0 && eap::aligned16(x, mean, rstd, rows, gx))
        return eap::run_kernel("slot_attn_input_grad", slot_input_grad_kernel<4>, eap::cdiv(n, 256), b, 1, dim3(256), 0, eap::S(stream), d, n, j, x, mean, rstd,
                               rows, vecs, gx);
    return eap::run_kernel("slot_attn_input_grad", slot_input_grad_kernel<1>, eap::cdiv(n, 64), b, 1, dim3(256), 0, eap::S(stream), d, n, j, x, mean, rstd, rows,
                           vecs, gx);
}
