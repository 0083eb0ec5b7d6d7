// csrc/norm_fold.hip -- the per-channel bookkeeping between the big kernels of a conv + BatchNorm + leaky_relu node, one launch (two where a
// second reduction follows the first) instead of the 10 - 35 element-wise and reduction launches on [o], [b, o, na] and [b, p] tensors that
// the same arithmetic takes when it is written as tensor expressions (vgtk/so3conv/functional.py: TrainEpilogue.moments, _backward_dense,
// _backward_narrow; vgtk/_hip.py: so3_dense_gplanes, DenseGeometry).  A few thousand float64 operations per layer: the launches were the cost.
//
// The arithmetic is the tensor expressions' own, operation for operation (this file is built with -ffp-contract=off: a fused multiply-add
// where the expression rounds twice would be a different number); only the order of the float64 sum over the partials differs from the
// library reduction it replaces: lane l of ONE wave adds partials l, l + 64, ... in index order, then a fixed xor tree over the 64 lanes --
// the same bits on every run.  Plain loads and vector stores, no LDS beyond a reduction buffer of at most 1 KB.
#include <math.h>
#include <string.h>

#include "common.h"

namespace {

constexpr int WAVE = 64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

// the sums of two rows of partials [parts] in float64, in every lane
__device__ __forceinline__ void two_row_sums(const float *__restrict__ a, const float *__restrict__ q, int parts, int lane, double &sa, double &sq) {
    sa = 0.0, sq = 0.0;
    for (int i = lane; i < parts; i += WAVE) {
        sa += (double)a[i];
        sq += (double)q[i];
    }
    sa = wave_sum(sa);
    sq = wave_sum(sq);
}

// max that hands a NaN on, as the library reductions do
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

// ---- 1. forward: partial sums -> the affine map, the statistics the backward keeps, the running statistics ------------------
// vgtk/so3conv/blocks.py batch_moments (no exchange), update_running_stats, affine_from_moments; one wave per channel
__global__ __launch_bounds__(WAVE) void norm_fold_train_kernel(int parts, long pivot_stride, double count, double eps, double momentum,
                                                               const float *__restrict__ ps, const float *__restrict__ pq,
                                                               const float *__restrict__ pivot, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, float *__restrict__ running_mean,
                                                               float *__restrict__ running_var, float *__restrict__ scale, float *__restrict__ shift,
                                                               double *__restrict__ mean, double *__restrict__ invstd, float *__restrict__ beta_copy,
                                                               float *__restrict__ inv_gamma) {
    const int ch = blockIdx.x, lane = threadIdx.x;
    double s1, s2;
    two_row_sums(ps + (long)ch * parts, pq + (long)ch * parts, parts, lane, s1, s2);
    if (lane != 0) return;
    const double m = s1 / count;
    const double mu = (double)pivot[(long)ch * pivot_stride] + m;
    double var = s2 / count - m * m;
    var = var < 0.0 ? 0.0 : var;                                      // (clamp_(min = 0): a NaN stays one)
    if (running_mean != nullptr) {
        // float32 tensors updated in place: mul_(1 - momentum), then add_(x, alpha = momentum) = self + alpha * x in one rounding
        const float keep = (float)(1.0 - momentum), alpha = (float)momentum;
        running_mean[ch] = fmaf(alpha, (float)mu, running_mean[ch] * keep);
        running_var[ch] = fmaf(alpha, (float)(var * (count / (count - 1.0))), running_var[ch] * keep);
    }
    const double g = (double)gamma[ch];
    const double is = rsqrt(var + eps);
    const double scale64 = g * is;
    scale[ch] = (float)scale64;
    shift[ch] = (float)((double)beta[ch] - mu * scale64);
    mean[ch] = mu;
    invstd[ch] = is;
    beta_copy[ch] = beta[ch];
    inv_gamma[ch] = g == 0.0 ? 0.f : (float)(1.0 / g);
}

// ---- 2. backward: partial sums -> d gamma, d beta, k2, k3 (+ the dense node's coefficient table and the rows' bounds) ---------------
// one wave per channel; every lane holds the sums, the lanes share the channel's b * na rows of the bound
__global__ __launch_bounds__(WAVE) void norm_fold_bwd_kernel(int o, int parts, int b, int na, double count, const float *__restrict__ pg,
                                                             const float *__restrict__ pgx, const float *__restrict__ k1v,
                                                             const float *__restrict__ beta, const float *__restrict__ inv_gamma,
                                                             const float *__restrict__ gmax, const float *__restrict__ xmax,
                                                             float *__restrict__ dgamma, float *__restrict__ dbeta, float *__restrict__ k2v,
                                                             float *__restrict__ k3v, float *__restrict__ coef, float *__restrict__ bound) {
    const int ch = blockIdx.x, lane = threadIdx.x;
    double tg, tgx;
    two_row_sums(pg + (long)ch * parts, pgx + (long)ch * parts, parts, lane, tg, tgx);
    const float k1 = k1v[ch];
    const float k2 = (float)((double)k1 * tg / count), k3 = (float)((double)k1 * tgx / count);
    if (lane == 0) {
        dgamma[ch] = (float)tgx;
        dbeta[ch] = (float)tg;
        k2v[ch] = k2;
        k3v[ch] = k3;
        if (coef != nullptr) {
            coef[ch] = k1, coef[o + ch] = k2, coef[2 * o + ch] = k3;
            coef[3 * o + ch] = beta[ch], coef[4 * o + ch] = inv_gamma[ch];
        }
    }
    if (bound == nullptr) return;
    const float a1 = fabsf(k1), a2 = fabsf(k2), a3 = fabsf(k3);
    for (int cloud = 0; cloud < b; ++cloud) {
        const long row = ((long)cloud * o + ch) * na;
        for (int a = lane; a < na; a += WAVE) bound[row + a] = (a1 * gmax[row + a] + a2) + a3 * xmax[row + a];
    }
}

// colmax [b, na] = the largest bound over the channels (the bound kernel above has finished: same stream)
// a block takes 16 anchors of one cloud: 16 threads per anchor share the channels, then a fixed order over the 16
__global__ __launch_bounds__(256) void norm_fold_colmax_kernel(int o, int na, const float *__restrict__ bound, float *__restrict__ colmax) {
    __shared__ float red[256];
    const int t = threadIdx.x, a = blockIdx.x * 16 + (t & 15), grp = t >> 4, cloud = blockIdx.y;
    float m = 0.f;                                                    // (the bound is a sum of magnitudes: never below 0)
    if (a < na) {
        const float *src = bound + (long)cloud * o * na + a;
        for (int ch = grp; ch < o; ch += 16) m = nan_max(m, src[(long)ch * na]);
    }
    red[t] = m;
    __syncthreads();
    if (grp == 0 && a < na) {
        for (int g = 1; g < 16; ++g) m = nan_max(m, red[g * 16 + t]);
        colmax[(long)cloud * na + a] = m;
    }
}

// ---- 3. the bound on Z's columns, four (anchor, row) columns to a word ---------------------------------------------------------
__global__ __launch_bounds__(256) void dense_zbound_kernel(int b, int na, int rp, int p, int ldw, long cnt_stride, const float *__restrict__ colmax,
                                                           const int32_t *__restrict__ cnt, const int32_t *__restrict__ n_rows,
                                                           float *__restrict__ words) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x, cloud = blockIdx.y;
    if (w >= ldw) return;
    float v = 0.f;
    if (w < na * rp / 4) {
        const int a = 4 * w / rp, r0 = 4 * w - a * rp, live = n_rows[cloud];
        const float m = colmax[(long)cloud * na + a];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c = r0 + j < live ? cnt[cloud * cnt_stride + r0 + j] : 0;
            c = c < 0 ? 0 : (c > p ? p : c);
            const float t = m * (float)c;
            v = j == 0 ? t : nan_max(v, t);
        }
    }
    words[(long)cloud * ldw + w] = v;
}

// the same words for PACKED Z (eap_so3_dense_product_packed_f32): column (a, r) of a cloud at a live16 + r, live16 = eap::live16(n_rows, rp) -- a
// multiple of 16, so a word's four columns stay with one anchor; the words past the cloud's na live16 columns are zero; ncols[cloud] = na live16
__global__ __launch_bounds__(256) void dense_zbound_packed_kernel(int b, int na, int rp, int p, int ldw, long cnt_stride, const float *__restrict__ colmax,
                                                                  const int32_t *__restrict__ cnt, const int32_t *__restrict__ n_rows,
                                                                  float *__restrict__ words, int32_t *__restrict__ ncols) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x, cloud = blockIdx.y;
    if (w >= ldw) return;
    const int live = n_rows[cloud], pitch = eap::live16(live, rp);
    if (w == 0) ncols[cloud] = na * pitch;
    float v = 0.f;
    if (w < na * pitch / 4) {
        const int a = 4 * w / pitch, r0 = 4 * w - a * pitch;
        const float m = colmax[(long)cloud * na + a];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c = r0 + j < live ? cnt[cloud * cnt_stride + r0 + j] : 0;
            c = c < 0 ? 0 : (c > p ? p : c);
            const float t = m * (float)c;
            v = j == 0 ? t : nan_max(v, t);
        }
    }
    words[(long)cloud * ldw + w] = v;
}

// ---- 4. the bound of the forward's stored operand: max_{c,r} |F| x (max_k sum_c |W| x 1.0001) ---------------------------------
// first launch: blocks [0, b c) take one (cloud, channel) slab of F [rp, na] each -> fpart [b, c, na]; blocks [b c, b c + o) one output channel
// of W3 each -> wsum [o] (the row sums in float64, rounded once: within half an ulp of the exact sum).  4 x na threads: a thread keeps its anchor.
__global__ __launch_bounds__(256) void dense_gbound_parts_kernel(int bc, int c, int rp, int na, int ks, const float *__restrict__ W3,
                                                                 const float *__restrict__ fc4, float *__restrict__ fpart, float *__restrict__ wsum) {
    __shared__ float red[256];
    const int t = threadIdx.x, nt = blockDim.x;
    if ((int)blockIdx.x < bc) {
        const float *src = fc4 + (long)blockIdx.x * rp * na;
        // (nt is a multiple of na: e % na == t % na throughout; four loads in flight per thread)
        const int len = rp * na;
        float m = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
        int e = t;
        for (; e + 3 * nt < len; e += 4 * nt) {
            const float v0 = src[e], v1 = src[e + nt], v2 = src[e + 2 * nt], v3 = src[e + 3 * nt];
            m = nan_max(m, fabsf(v0)), m1 = nan_max(m1, fabsf(v1)), m2 = nan_max(m2, fabsf(v2)), m3 = nan_max(m3, fabsf(v3));
        }
        for (; e < len; e += nt) m = nan_max(m, fabsf(src[e]));
        m = nan_max(nan_max(m, m1), nan_max(m2, m3));
        red[t] = m;
        __syncthreads();
        if (t < na) {
            for (int g = 1; g < nt / na; ++g) m = nan_max(m, red[t + g * na]);
            fpart[(long)blockIdx.x * na + t] = m;
        }
        return;
    }
    const int oc = blockIdx.x - bc, lane = t & (WAVE - 1), wave = t / WAVE, waves = nt / WAVE;      // (whole waves only: 2 to 4 of them)
    float m = 0.f;
    if (wave < waves)
        for (int k = wave; k < ks; k += waves) {
            const float *row = W3 + ((long)oc * ks + k) * c;
            double s = 0.0;
            for (int i = lane; i < c; i += WAVE) s += (double)fabsf(row[i]);
            m = nan_max(m, (float)wave_sum(s));
        }
    if (lane == 0 && wave < waves) red[wave] = m;
    __syncthreads();
    if (t == 0) {
        for (int g = 1; g < waves; ++g) m = nan_max(m, red[g]);
        wsum[oc] = m * 1.0001f;
    }
}

// second launch: one block per (cloud, anchor): the maximum over the channels' parts, then the o products
__global__ __launch_bounds__(256) void dense_gbound_kernel(int c, int na, int o, const float *__restrict__ fpart, const float *__restrict__ wsum,
                                                           float *__restrict__ bound) {
    __shared__ float red[256];
    const int t = threadIdx.x, cloud = blockIdx.x / na, a = blockIdx.x - cloud * na;
    float m = 0.f;
    for (int ch = t; ch < c; ch += 256) m = nan_max(m, fpart[((long)cloud * c + ch) * na + a]);
    red[t] = m;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) red[t] = nan_max(red[t], red[t + s]);
        __syncthreads();
    }
    m = red[0];
    for (int oc = t; oc < o; oc += 256) bound[(long)blockIdx.x * o + oc] = m * wsum[oc];
}

// ---- 5. what follows the sort of a cloud's query points: the int32 order, the tables gathered through it, the pivot's column ------
// one thread per 16 bytes of a point's membership words; the first of a point's threads also moves its order, its coordinates and the pivot
__global__ __launch_bounds__(256) void dense_point_order_kernel(int p, int quads, const int64_t *__restrict__ order, const int4 *__restrict__ memb,
                                                                const float *__restrict__ q_xyz, int32_t *__restrict__ order32,
                                                                int4 *__restrict__ memb_out, float *__restrict__ xyz_out,
                                                                int32_t *__restrict__ pivot_pos) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int cloud = blockIdx.y;
    if (i >= (long)p * quads) return;
    const int j = (int)(i / quads), q = (int)(i - (long)j * quads);
    const int64_t src = order[(long)cloud * p + j];
    if (src < 0 || src >= p) return;                                  // (not a permutation: nothing is read through it)
    memb_out[((long)cloud * p + j) * quads + q] = memb[((long)cloud * p + src) * quads + q];
    if (q != 0) return;
    order32[(long)cloud * p + j] = (int32_t)src;
#pragma unroll
    for (int k = 0; k < 3; ++k) xyz_out[((long)cloud * 3 + k) * p + j] = q_xyz[((long)cloud * 3 + k) * p + src];
    if (cloud == 0 && src == 0) pivot_pos[0] = j;
}

inline double from_bits(int64_t bits) {
    double v;
    memcpy(&v, &bits, sizeof v);
    return v;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int eap_norm_fold_train_f32(int o, int parts, int64_t pivot_stride, int64_t count, int64_t eps_bits, int64_t momentum_bits,
                                       const float *ps, const float *pq, const float *pivot, const float *gamma, const float *beta,
                                       float *running_mean, float *running_var, float *scale, float *shift, double *mean, double *invstd,
                                       float *beta_copy, float *inv_gamma, eap_stream_t stream) {
    if (!ps || !pq || !pivot || !gamma || !beta || !scale || !shift || !mean || !invstd || !beta_copy || !inv_gamma)
        return eap::bad_arg("norm_fold_train: null pointer (only running_mean / running_var may be null, and only together)");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return eap::bad_arg("norm_fold_train: null pointer (only running_mean / running_var may be null, and only together)");
    if (o <= 0 || parts <= 0 || count <= 0 || pivot_stride <= 0) return eap::bad_arg("norm_fold_train: o, parts, count and the pivot stride must be positive");
    return eap::run_kernel("norm_fold_train", norm_fold_train_kernel, o, 1, 1, dim3(WAVE), 0, eap::S(stream), parts, (long)pivot_stride, (double)count,
                           from_bits(eps_bits), from_bits(momentum_bits), ps, pq, pivot, gamma, beta, running_mean, running_var, scale, shift, mean,
                           invstd, beta_copy, inv_gamma);
}

extern "C" int eap_norm_fold_bwd_f32(int o, int parts, int b, int na, int64_t count, const float *pg, const float *pgx, const float *k1,
                                     const float *beta, const float *inv_gamma, const float *gmax, const float *xmax, float *dgamma, float *dbeta,
                                     float *k2, float *k3, float *coef, float *bound, float *colmax, eap_stream_t stream) {
    if (!pg || !pgx || !k1 || !dgamma || !dbeta || !k2 || !k3) return eap::bad_arg("norm_fold_bwd: null pointer");
    const bool dense = beta || inv_gamma || gmax || xmax || coef || bound || colmax;
    if (dense && !(beta && inv_gamma && gmax && xmax && coef && bound && colmax))
        return eap::bad_arg("norm_fold_bwd: null pointer (beta, inv_gamma, gmax, xmax, coef, bound and colmax come together or not at all)");
    if (o <= 0 || parts <= 0 || count <= 0) return eap::bad_arg("norm_fold_bwd: o, parts and count must be positive");
    if (dense && (b <= 0 || na <= 0 || b > 65535)) return eap::bad_arg("norm_fold_bwd: b and na must be positive, b at most 65535 (grid.y)");
    if (int e = eap::run_kernel("norm_fold_bwd", norm_fold_bwd_kernel, o, 1, 1, dim3(WAVE), 0, eap::S(stream), o, parts, b, na, (double)count, pg, pgx, k1,
                                beta, inv_gamma, gmax, xmax, dgamma, dbeta, k2, k3, coef, bound))
        return e;
    if (!dense) return 0;
    return eap::run_kernel("norm_fold_bwd (colmax)", norm_fold_colmax_kernel, eap::cdiv(na, 16), b, 1, dim3(256), 0, eap::S(stream), o, na, (const float *)bound,
                           colmax);
}

extern "C" int eap_so3_dense_zbound_f32(int b, int na, int rp, int p, int ldz, int64_t cnt_stride, const float *colmax, const int32_t *cnt,
                                        const int32_t *n_rows, float *words, eap_stream_t stream) {
    if (!colmax || !cnt || !n_rows || !words) return eap::bad_arg("so3_dense_zbound: null pointer");
    if (b <= 0 || na <= 0 || rp <= 0 || p <= 0 || ldz <= 0) return eap::bad_arg("so3_dense_zbound: b, na, rp, p and ldz must be positive");
    if (rp % 4 != 0 || ldz % 4 != 0 || (long long)na * rp > ldz || cnt_stride < rp)
        return eap::bad_arg("so3_dense_zbound: rp and ldz multiples of 4, ldz >= na * rp, the row stride of cnt >= rp");
    return eap::run_kernel("so3_dense_zbound", dense_zbound_kernel, eap::cdiv(ldz / 4, 256), b, 1, dim3(256), 0, eap::S(stream), b, na, rp, p, ldz / 4,
                           (long)cnt_stride, colmax, cnt, n_rows, words);
}

// eap_so3_dense_zbound_f32 for packed Z: the word of columns 4 w .. 4 w + 3 of cloud i bounds (a, r0 .. r0 + 3) with a = 4 w / live16[i],
// r0 = 4 w % live16[i]; also writes ncols int32 [b] = na live16[i], the live prefix the two tail products take
extern "C" int eap_so3_dense_zbound_packed_f32(int b, int na, int rp, int p, int ldz, int64_t cnt_stride, const float *colmax, const int32_t *cnt,
                                               const int32_t *n_rows, float *words, int32_t *ncols, eap_stream_t stream) {
    if (!colmax || !cnt || !n_rows || !words || !ncols) return eap::bad_arg("so3_dense_zbound_packed: null pointer");
    if (b <= 0 || na <= 0 || rp <= 0 || p <= 0 || ldz <= 0) return eap::bad_arg("so3_dense_zbound_packed: b, na, rp, p and ldz must be positive");
    if (rp % 16 != 0 || ldz % 4 != 0 || (long long)na * rp > ldz || cnt_stride < rp)
        return eap::bad_arg("so3_dense_zbound_packed: rp a multiple of 16, ldz a multiple of 4, ldz >= na * rp, the row stride of cnt >= rp");
    return eap::run_kernel("so3_dense_zbound_packed", dense_zbound_packed_kernel, eap::cdiv(ldz / 4, 256), b, 1, dim3(256), 0, eap::S(stream), b, na, rp, p, ldz / 4,
                           (long)cnt_stride, colmax, cnt, n_rows, words, ncols);
}

extern "C" int eap_so3_dense_gplanes_bound_f32(int b, int o, int c, int na, int ks, int rp, const float *W3, const float *fc4, float *fpart,
                                               float *wsum, float *bound, eap_stream_t stream) {
    if (!W3 || !fc4 || !fpart || !wsum || !bound) return eap::bad_arg("so3_dense_gplanes_bound: null pointer");
    if (b <= 0 || o <= 0 || c <= 0 || na <= 0 || ks <= 0 || rp <= 0) return eap::bad_arg("so3_dense_gplanes_bound: every size must be positive");
    if (na > 128 || (long long)rp * na > 0x7fffffffLL || (long long)b * c > 0x7fffffffLL - o || (long long)b * na > 0x7fffffffLL)
        return eap::bad_arg("so3_dense_gplanes_bound: na <= 128, rp * na, b * c + o and b * na below 2^31");
    const int nt = 256 / na * na;                                     // whole anchor groups: 129 .. 256 threads, at least two whole waves
    if (int e = eap::run_kernel("so3_dense_gplanes_bound (parts)", dense_gbound_parts_kernel, (long long)b * c + o, 1, 1, dim3(nt), 0, eap::S(stream), b * c, c,
                                rp, na, ks, W3, fc4, fpart, wsum))
        return e;
    return eap::run_kernel("so3_dense_gplanes_bound", dense_gbound_kernel, (long long)b * na, 1, 1, dim3(256), 0, eap::S(stream), c, na, o, (const float *)fpart,
                           (const float *)wsum, bound);
}

extern "C" int eap_so3_dense_point_order(int b, int p, int words, const int64_t *order, const uint32_t *memb, const float *q_xyz, int32_t *order32,
                                         uint32_t *memb_out, float *xyz_out, int32_t *pivot_pos, eap_stream_t stream) {
    if (!order || !memb || !q_xyz || !order32 || !memb_out || !xyz_out || !pivot_pos) return eap::bad_arg("so3_dense_point_order: null pointer");
    if (b <= 0 || p <= 0) return eap::bad_arg("so3_dense_point_order: b and p must be positive");
    if (words != 16 && words != 32) return eap::bad_arg("so3_dense_point_order: 16 or 32 membership words per point");
    if (!aligned16(memb) || !aligned16(memb_out)) return eap::bad_arg("so3_dense_point_order: takes 16-byte aligned membership tables");
    const int quads = words / 4;
    return eap::run_kernel("so3_dense_point_order", dense_point_order_kernel, eap::cdiv((long long)p * quads, 256), b, 1, dim3(256), 0, eap::S(stream), p, quads,
                           order, reinterpret_cast<const int4 *>(memb), q_xyz, order32, reinterpret_cast<int4 *>(memb_out), xyz_out, pivot_pos);
}
