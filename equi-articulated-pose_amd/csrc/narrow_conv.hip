// csrc/narrow_conv.hip -- the first inter conv layer (1 -> 64 channels: C*K = 24 contraction indices) with its training-mode
// BatchNorm + leaky_relu as ONE node that never writes the conv output (vgtk/so3conv/functional.py, regime 'narrow input';
// `x = conv(x); feat = relu(norm(x.feats))`, SPConvNets/utils/base_so3poseconv.py:L205-222 + vgtk/vgtk/so3conv/modules.py:L48-55).
//
// With ck = C*K <= 32 the conv output y[b,o,n] = sum_k W[o,k] X[b,k,n] is a 24-term dot product per element: cheaper to
// recompute from the grouped input X [b, ck, n] (n = P*A) than to store and reload (y is 2.7 x the size of X at o = 64).
//   stats       partial (sum, sum of squares) of y - pivot per (channel, cloud, segment)         reads X
//   bnact_fwd   y' = leaky(scale (W X) + shift)                                                  reads X, writes y'
//   bwd_reduce  partial sum(g), sum(g xhat) from dY' and the recomputed pre-activation           reads X, dY'
//   bwd_dw      dW = sum gx X^T, gx = k1 g - k2 - k3 xhat formed in registers                    reads X, dY'
// All reductions leave per-block partials that are summed in a fixed order: bit-reproducible, no float atomics.
//
// y comes off v_mfma_f32_32x32x2_f32 (an exact fp32 fmaf chain) in every pass, so all four see the same bits.  A wave takes
// 128 columns at a time: lane (li = lane & 31, h = lane >> 5) loads float4 X[2 s + h][col0 + 4 li ..] for the ck / 2 steps s
// (16-byte loads, 512 contiguous bytes per row and half-wave); component c of those registers is the operand of the
// 32-column tile {col0 + 4 i + c}.  W[o][2 s + h] sits in registers as the other operand.
//   mfma(W, X): D lane = column quad li, register r = channel (r & 3) + 8 (r >> 2) + 4 h  -> float4 per channel row and lane:
//               the coalesced form (loads of dY', stores of y'); stats, bnact_fwd, bwd_reduce
//   mfma(X, W): D lane = channel li, register r = column quad (r & 3) + 8 (r >> 2) + 4 h  -> gx[o][col] is, as it stands,
//               the A operand of the second product dW[o, k] += gx[o][col] X[k][col] (lane = k, padded to 32); bwd_dw
#include "common.h"
#include "device_prims.h"
#include <type_traits>

namespace {

constexpr int NT = 256, WAVES = 4;
constexpr int TILE = 128;                       // columns per wave and step
constexpr int SEGC = 2048;                      // columns per block
// A block takes `ct` tiles of 32 channels (2 where the channels come in 64s, else 1): wave w works on channel tile w % ct and, with
// the other WAVES / ct - 1 waves of that tile, walks the block's columns in steps of TILE.  (The ct waves of a column range load
// the same X at the same time: one trip to L2.  One tile per wave keeps a wave's registers at two waves per SIMD without scratch.)

__device__ __forceinline__ int drow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// lane (li, h): X[2 s + h][col0 + 4 li .. + 3], zeros past the last row / column.  Addresses are a wave-uniform base (row 2 s,
// column col0) plus the lane's 32-bit byte offset voff = 4 (h n + 4 li): rows are at most 32 and n < 2^25 (checked by the entries)
template <int KS2>
__device__ __forceinline__ void load_x(f32x4 (&xa)[KS2], const float *__restrict__ xb, long n, long col0, unsigned voff, bool ok, int ck, int h) {
#pragma unroll
    for (int s = 0; s < KS2; ++s)
        xa[s] = (ok && 2 * s + h < ck) ? ld_off<f32x4>(xb + (size_t)(2 * s) * n + col0, voff) : (f32x4){0.f, 0.f, 0.f, 0.f};
}

// lane (li, h): W[o0 + li][2 s + h]
template <int KS2>
__device__ __forceinline__ void load_w(float (&wf)[KS2], const float *__restrict__ W, int orow, int ck, int h) {
#pragma unroll
    for (int s = 0; s < KS2; ++s) wf[s] = (2 * s + h < ck) ? W[(size_t)orow * ck + 2 * s + h] : 0.f;
}

// the four 32-column tiles of a wave's 128 columns; T: channels in the lanes (see the head of the file)
template <int KS2, bool T>
__device__ __forceinline__ void conv_tile(f32x16 (&d)[4], const f32x4 (&xa)[KS2], const float (&wf)[KS2]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) d[c][r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
        if (T) {
            d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s].x, wf[s], d[0], 0, 0, 0);
            d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s].y, wf[s], d[1], 0, 0, 0);
            d[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s].z, wf[s], d[2], 0, 0, 0);
            d[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s].w, wf[s], d[3], 0, 0, 0);
        } else {
            d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s], xa[s].x, d[0], 0, 0, 0);
            d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s], xa[s].y, d[1], 0, 0, 0);
            d[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s], xa[s].z, d[2], 0, 0, 0);
            d[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s], xa[s].w, d[3], 0, 0, 0);
        }
    }
}

// the per-lane sums sa / qa [r] (channel drow(r, h) of the wave's tile) of a block -> partial[(channel * nb + cloud) * nseg + seg]:
// the 32 lanes of a half by a fixed butterfly, the waves of a channel tile in order
__device__ __forceinline__ void block_sums(float (&sa)[16], float (&qa)[16], float (*s_red)[2][32], int ct, int o0, int bi, int nb,
                                           int nseg, int seg, float *__restrict__ pa, float *__restrict__ pq) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float a = sa[r], q = qa[r];
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) { a += __shfl_xor(a, d); q += __shfl_xor(q, d); }
        if (li == 0) { s_red[wave][0][drow(r, h)] = a; s_red[wave][1][drow(r, h)] = q; }
    }
    __syncthreads();
    if (t < 32 * ct) {
        float a = 0.f, q = 0.f;
        for (int w = t >> 5; w < WAVES; w += ct) { a += s_red[w][0][t & 31]; q += s_red[w][1][t & 31]; }
        const size_t at = ((size_t)(o0 + t) * nb + bi) * nseg + seg;
        pa[at] = a; pq[at] = q;
    }
}

// where a thread works: block -> (segment of SEGC columns, ct channel tiles from o0, cloud); wave -> (channel tile, column walk)
struct Pos {
    int seg, bi, lane, li, h, ch0, cw, ncw;      // ch0: first channel of the wave's tile; cw of ncw: the wave's place in the column walk
    long beg, end;                               // the block's columns
    unsigned xoff;                               // load_x's lane offset
    __device__ Pos(int ct, long n) {
        seg = blockIdx.x; bi = blockIdx.z;
        const int wave = threadIdx.x >> 6;
        lane = threadIdx.x & 63; li = lane & 31; h = lane >> 5;
        ch0 = (blockIdx.y * ct + wave % ct) * 32; cw = wave / ct; ncw = WAVES / ct;
        beg = (long)seg * SEGC; end = min(n, beg + SEGC);
        xoff = 4u * ((unsigned)h * (unsigned)n + 4u * li);
    }
};

// pivot[o] = y[0, o, 0]: a function of the data alone (bn_stats_kernel's choice), the same bits in every block
template <int KS2>
__global__ __launch_bounds__(NT) void narrow_conv_stats_kernel(int ct, int ck, long n, int nseg, const float *__restrict__ W,
                                                                 const float *__restrict__ x, float *__restrict__ pivot,
                                                                 float *__restrict__ psum, float *__restrict__ psq) {
    __shared__ __attribute__((aligned(16))) float s_piv[64];
    __shared__ float s_red[WAVES][2][32];
    const Pos w(ct, n);
    const int t = threadIdx.x, o0 = blockIdx.y * ct * 32, h = w.h;
    if (t < 32 * ct) {
        float p = 0.f;
        for (int k = 0; k < ck; ++k) p = fmaf(W[(size_t)(o0 + t) * ck + k], x[(size_t)k * n], p);
        s_piv[t] = p;
        if (w.seg == 0 && w.bi == 0) pivot[o0 + t] = p;
    }
    __syncthreads();
    float wf[KS2];
    load_w<KS2>(wf, W, w.ch0 + w.li, ck, h);
    f32x4 pv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) pv[g] = *reinterpret_cast<const f32x4 *>(&s_piv[w.ch0 - o0 + 8 * g + 4 * h]);
    float sa[16], qa[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sa[r] = qa[r] = 0.f;
    const float *xb = x + (size_t)w.bi * ck * n;
#pragma unroll 1
    for (long col0 = w.beg + (long)w.cw * TILE; col0 < w.end; col0 += (long)w.ncw * TILE) {
        const long col = col0 + 4 * w.li;
        const bool ok = col < n;
        f32x4 xa[KS2];
        load_x<KS2>(xa, xb, n, col0, w.xoff, ok, ck, h);
        f32x16 d[4];
        conv_tile<KS2, false>(d, xa, wf);
        if (ok) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float dd = d[c][r] - pv[r >> 2][r & 3];
                    sa[r] += dd;
                    qa[r] = fmaf(dd, dd, qa[r]);
                }
        }
    }
    block_sums(sa, qa, s_red, ct, o0, w.bi, gridDim.z, nseg, w.seg, psum, psq);
}

template <int KS2>
__global__ __launch_bounds__(NT) void narrow_conv_bnact_fwd_kernel(int ct, int o, int ck, long n, float slope, const float *__restrict__ W,
                                                                     const float *__restrict__ x, const float *__restrict__ scale,
                                                                     const float *__restrict__ shift, float *__restrict__ y) {
    const Pos w(ct, n);
    const int h = w.h;
    float wf[KS2];
    load_w<KS2>(wf, W, w.ch0 + w.li, ck, h);
    f32x4 sc[4], sh[4];                                               // channels ch0 + 8 g + 4 h + q (16-byte aligned: multiples of 4 floats)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        sc[g] = *reinterpret_cast<const f32x4 *>(scale + w.ch0 + 8 * g + 4 * h);
        sh[g] = *reinterpret_cast<const f32x4 *>(shift + w.ch0 + 8 * g + 4 * h);
    }
    const float *xb = x + (size_t)w.bi * ck * n;
    float *yb = y + ((size_t)w.bi * o + w.ch0) * n;
    const unsigned roff = 4u * (4u * h * (unsigned)n + 4u * w.li);     // channel row 4 h, column quad li, in bytes
#pragma unroll 1
    for (long col0 = w.beg + (long)w.cw * TILE; col0 < w.end; col0 += (long)w.ncw * TILE) {
        const long col = col0 + 4 * w.li;
        const bool ok = col < n;
        f32x4 xa[KS2];
        load_x<KS2>(xa, xb, n, col0, w.xoff, ok, ck, h);
        f32x16 d[4];
        conv_tile<KS2, false>(d, xa, wf);
        if (ok) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = sc[r >> 2][r & 3], b = sh[r >> 2][r & 3];
                f32x4 v;
                v.x = fmaf(d[0][r], a, b); v.y = fmaf(d[1][r], a, b); v.z = fmaf(d[2][r], a, b); v.w = fmaf(d[3][r], a, b);
                v.x = v.x > 0.f ? v.x : v.x * slope; v.y = v.y > 0.f ? v.y : v.y * slope;
                v.z = v.z > 0.f ? v.z : v.z * slope; v.w = v.w > 0.f ? v.w : v.w * slope;
                st_off<f32x4>(yb + (size_t)(8 * (r >> 2)) * n + col0, roff + 4u * (unsigned)(r & 3) * (unsigned)n, v);
            }
        }
    }
}

// partials of sum(g) and sum(g xhat), laid out and ordered like bn_act_bwd_reduce_kernel (csrc/bn_act.hip):
// g = dY' (pre > 0 ? 1 : slope), pre = scale y + shift, xhat = (y - mean) invstd
template <int KS2>
__global__ __launch_bounds__(NT) void narrow_conv_bwd_reduce_kernel(int ct, int o, int ck, long n, int nseg, float slope,
                                                                      const float *__restrict__ gy, const float *__restrict__ x,
                                                                      const float *__restrict__ W, const float *__restrict__ scale,
                                                                      const float *__restrict__ shift, const float *__restrict__ mean,
                                                                      const float *__restrict__ invstd, float *__restrict__ pg,
                                                                      float *__restrict__ pgx) {
    __shared__ __attribute__((aligned(16))) float s_sc[64], s_sh[64], s_mu[64], s_is[64];
    __shared__ float s_red[WAVES][2][32];
    const Pos w(ct, n);
    const int t = threadIdx.x, o0 = blockIdx.y * ct * 32, h = w.h;
    if (t < 32 * ct) { s_sc[t] = scale[o0 + t]; s_sh[t] = shift[o0 + t]; s_mu[t] = mean[o0 + t]; s_is[t] = invstd[o0 + t]; }
    __syncthreads();
    float wf[KS2];
    load_w<KS2>(wf, W, w.ch0 + w.li, ck, h);
    float sa[16], qa[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sa[r] = qa[r] = 0.f;
    const float *xb = x + (size_t)w.bi * ck * n;
    const float *gb = gy + ((size_t)w.bi * o + w.ch0) * n;
    const unsigned roff = 4u * (4u * h * (unsigned)n + 4u * w.li);     // channel row 4 h, column quad li, in bytes
    const int lc = w.ch0 - o0;
#pragma unroll 1
    for (long col0 = w.beg + (long)w.cw * TILE; col0 < w.end; col0 += (long)w.ncw * TILE) {
        const long col = col0 + 4 * w.li;
        const bool ok = col < n;
        f32x4 xa[KS2];
        load_x<KS2>(xa, xb, n, col0, w.xoff, ok, ck, h);
        f32x16 d[4];
        conv_tile<KS2, false>(d, xa, wf);
        if (ok) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 gv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) gv[q] = ld_off<f32x4>(gb + (size_t)(8 * g) * n + col0, roff + 4u * q * (unsigned)n);
                const f32x4 sc = *reinterpret_cast<const f32x4 *>(&s_sc[lc + 8 * g + 4 * h]), sh = *reinterpret_cast<const f32x4 *>(&s_sh[lc + 8 * g + 4 * h]);
                const f32x4 mu = *reinterpret_cast<const f32x4 *>(&s_mu[lc + 8 * g + 4 * h]), is = *reinterpret_cast<const f32x4 *>(&s_is[lc + 8 * g + 4 * h]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float yv = d[c][4 * g + q];
                        const float pre = fmaf(yv, sc[q], sh[q]);
                        const float gg = pre > 0.f ? gv[q][c] : gv[q][c] * slope;
                        sa[4 * g + q] += gg;
                        qa[4 * g + q] = fmaf(gg, (yv - mu[q]) * is[q], qa[4 * g + q]);
                    }
            }
        }
    }
    block_sums(sa, qa, s_red, ct, o0, w.bi, gridDim.z, nseg, w.seg, pg, pgx);
}

// slab[(cloud * nseg + seg)][o][ck] = sum over the block's columns of gx[o][col] X[k][col],
// gx = scale g - k2 - xhat k3 (bn_act_bwd_apply_kernel's formula), never written
template <int KS2>
__global__ __launch_bounds__(NT) void narrow_conv_bwd_dw_kernel(int ct, int o, int ck, long n, int nseg, float slope,
                                                                  const float *__restrict__ gy, const float *__restrict__ x,
                                                                  const float *__restrict__ W, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, const float *__restrict__ mean,
                                                                  const float *__restrict__ invstd, const float *__restrict__ k2,
                                                                  const float *__restrict__ k3, float *__restrict__ partial) {
    __shared__ float s_part[WAVES][16][64];
    const Pos w(ct, n);
    const int h = w.h, li = w.li, wave = threadIdx.x >> 6;
    const int ch = w.ch0 + li;                                        // this lane's channel
    float wf[KS2];
    load_w<KS2>(wf, W, ch, ck, h);
    const float sc = scale[ch], sh = shift[ch], mu = mean[ch], is = invstd[ch], c2 = k2[ch], c3 = k3[ch];
    const float *gb = gy + ((size_t)w.bi * o + w.ch0) * n;
    const unsigned goff = 4u * ((unsigned)li * (unsigned)n + 16u * h), koff = 4u * ((unsigned)min(li, ck - 1) * (unsigned)n + 16u * h);
    f32x16 dw;
#pragma unroll
    for (int r = 0; r < 16; ++r) dw[r] = 0.f;
    const float *xb = x + (size_t)w.bi * ck * n;
    // (second product: lane = contraction row k of W, zeros past ck; both operands as base + column quad 8 g + q, lane offset row + 4 h quads)
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (long col0 = w.beg + (long)w.cw * TILE; col0 < w.end; col0 += (long)w.ncw * TILE) {
        const long col = col0 + 4 * li;
        f32x4 xa[KS2];
        load_x<KS2>(xa, xb, n, col0, w.xoff, col < n, ck, h);
        f32x16 d[4];
        conv_tile<KS2, true>(d, xa, wf);                              // d[c][r] = y[this lane's channel][col0 + 4 drow(r, h) + c]
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 gv[4], xv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long cq = col0 + 4 * (8 * g + 4 * h + q);
                const bool in = cq < n;                               // (past the end: X = 0 there, so the term vanishes whatever gx is)
                gv[q] = in ? ld_off<f32x4>(gb + col0 + 4 * (8 * g + q), goff) : zero4;
                xv[q] = (in && li < ck) ? ld_off<f32x4>(xb + col0 + 4 * (8 * g + q), koff) : zero4;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float yv = d[c][4 * g + q];
                    const float pre = fmaf(yv, sc, sh);
                    const float gg = pre > 0.f ? gv[q][c] : gv[q][c] * slope;
                    const float gx = fmaf(gg, sc, -c2) - ((yv - mu) * is) * c3;
                    dw = __builtin_amdgcn_mfma_f32_32x32x2f32(gx, xv[q][c], dw, 0, 0, 0);
                }
        }
    }
    // dw: lane (li = k, h), register r = channel ch0 + drow(r, h); the waves of a channel tile through LDS, added in order
#pragma unroll
    for (int r = 0; r < 16; ++r) s_part[wave][r][w.lane] = dw[r];
    __syncthreads();
    if (wave < ct) {
        float *slab = partial + ((size_t)w.bi * nseg + w.seg) * o * ck;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = 0.f;
            for (int u = wave; u < WAVES; u += ct) v += s_part[u][r][w.lane];
            if (li < ck) slab[(size_t)(w.ch0 + drow(r, h)) * ck + li] = v;
        }
    }
}

// one wave per element of dW: lane l adds slabs l, l + 64, ... in order, then a fixed butterfly over the lanes
__global__ __launch_bounds__(256) void narrow_conv_dw_sum_kernel(int mn, int slabs, const float *__restrict__ partial, float *__restrict__ dW) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= mn) return;
    float s = 0.f;
    for (int z = lane; z < slabs; z += 64) s += partial[(size_t)z * mn + e];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) dW[e] = s;
}

inline int nseg_of(long n) { return (int)((n + SEGC - 1) / SEGC); }

inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// what every entry refuses, before any device call
inline int refuse(const char *who, int o, int ck, long n, const void *p0, const void *p1, const void *p2 = nullptr) {
    char buf[200];
    const char *why = nullptr;
    if (ck < 1 || ck > 32) why = "1 to 32 contraction indices (C*K)";
    else if (o < 32 || o % 32 != 0) why = "a multiple of 32 output channels";
    else if (n < 0 || (n & 3) != 0 || n >= (1l << 25)) why = "a row length (P*A) that is a multiple of 4 below 2^25";
    else if (misaligned(p0) || misaligned(p1) || misaligned(p2)) why = "16-byte aligned tensors";
    if (!why) return 0;
    snprintf(buf, sizeof(buf), "%s: takes %s", who, why);
    return eap::bad_arg(buf);
}

inline int tiles_per_block(int o) { return o % 64 == 0 ? 2 : 1; }

// 12 k-steps up to ck = 24, else 16
template <typename F>
int by_depth(int ck, F &&f) {
    return ck <= 24 ? f(std::integral_constant<int, 12>{}) : f(std::integral_constant<int, 16>{});
}

}  // namespace

// segments per (cloud, channel) row: the partial arrays of the two reductions are [o][b * segments], dW's slabs [b * segments][o][ck]
extern "C" int eap_narrow_conv_segments(int64_t n) { return n > 0 ? nseg_of((long)n) : 0; }

extern "C" int eap_narrow_conv_stats_f32(int b, int o, int ck, int64_t n, const float *W, const float *x, float *pivot, float *psum,
                                         float *psq, eap_stream_t stream) {
    if (int e = refuse("narrow_conv_stats", o, ck, (long)n, x, nullptr)) return e;
    if (b <= 0 || n <= 0) return 0;
    const int nseg = nseg_of((long)n), ct = tiles_per_block(o);
    return by_depth(ck, [&](auto ks2) {
        return eap::run_kernel("narrow_conv_stats", narrow_conv_stats_kernel<decltype(ks2)::value>, nseg, o / (32 * ct), b, dim3(NT), 0, eap::S(stream), ct,
                               ck, (long)n, nseg, W, x, pivot, psum, psq);
    });
}

extern "C" int eap_narrow_conv_bnact_fwd_f32(int b, int o, int ck, int64_t n, float slope, const float *W, const float *x, const float *scale,
                                             const float *shift, float *y, eap_stream_t stream) {
    if (int e = refuse("narrow_conv_bnact_fwd", o, ck, (long)n, x, y, scale)) return e;
    if (misaligned(shift)) return eap::bad_arg("narrow_conv_bnact_fwd: takes 16-byte aligned tensors");
    if (b <= 0 || n <= 0) return 0;
    const int ct = tiles_per_block(o);
    return by_depth(ck, [&](auto ks2) {
        return eap::run_kernel("narrow_conv_bnact_fwd", narrow_conv_bnact_fwd_kernel<decltype(ks2)::value>, nseg_of((long)n), o / (32 * ct), b, dim3(NT), 0,
                               eap::S(stream), ct, o, ck, (long)n, slope, W, x, scale, shift, y);
    });
}

extern "C" int eap_narrow_conv_bwd_reduce_f32(int b, int o, int ck, int64_t n, float slope, const float *gy, const float *x, const float *W,
                                              const float *scale, const float *shift, const float *mean, const float *invstd, float *pg,
                                              float *pgx, eap_stream_t stream) {
    if (int e = refuse("narrow_conv_bwd_reduce", o, ck, (long)n, x, gy)) return e;
    if (b <= 0 || n <= 0) return 0;
    const int nseg = nseg_of((long)n), ct = tiles_per_block(o);
    return by_depth(ck, [&](auto ks2) {
        return eap::run_kernel("narrow_conv_bwd_reduce", narrow_conv_bwd_reduce_kernel<decltype(ks2)::value>, nseg, o / (32 * ct), b, dim3(NT), 0, eap::S(stream),
                               ct, o, ck, (long)n, nseg, slope, gy, x, W, scale, shift, mean, invstd, pg, pgx);
    });
}

// partial: b * eap_narrow_conv_segments(n) slabs of [o][ck] floats (scratch); dW [o][ck] = their sum in slab order
extern "C" int eap_narrow_conv_bwd_dw_f32(int b, int o, int ck, int64_t n, float slope, const float *gy, const float *x, const float *W,
                                          const float *scale, const float *shift, const float *mean, const float *invstd, const float *k2,
                                          const float *k3, float *partial, float *dW, eap_stream_t stream) {
    if (int e = refuse("narrow_conv_bwd_dw", o, ck, (long)n, x, gy)) return e;
    if (b <= 0 || n <= 0) return 0;
    const int nseg = nseg_of((long)n), ct = tiles_per_block(o);
    hipStream_t s = eap::S(stream);
    int e = by_depth(ck, [&](auto ks2) {
        return eap::run_kernel("narrow_conv_bwd_dw", narrow_conv_bwd_dw_kernel<decltype(ks2)::value>, nseg, o / (32 * ct), b, dim3(NT), 0, s, ct, o, ck, (long)n,
                               nseg, slope, gy, x, W, scale, shift, mean, invstd, k2, k3, partial);
    });
    if (e) return e;
    const int mn = o * ck;
    return eap::run_kernel("narrow_conv_bwd_dw (sum)", narrow_conv_dw_sum_kernel, eap::cdiv(mn, 4), 1, 1, dim3(256), 0, s, mn, b * nseg, partial, dW);
}
