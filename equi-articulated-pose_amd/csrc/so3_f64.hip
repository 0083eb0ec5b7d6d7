// csrc/so3_f64.hip -- the float64 regime of the SO(3) conv layers on gfx950: one plain kernel per step, chosen by the dtype of
// the tensors (vgtk/so3conv/functional.py, _InterConvF64 / _IntraConvF64 / _ContractF64).
//
// Reference path in float64 (vgtk/vgtk/so3conv/functional.py, L1025-1261 with every tensor .double()):
//   ball_idx, grouped_xyz = ball_query(xyz, xyz, r, nn)          L1061   grouped_xyz is FLOAT32 for any input
//                                                                        (gathering_cuda.cpp:L38-39 allocates a float tensor)
//   R_rel = R_p R_n^T ; g = R_rel (float(x_n) - x_p)             L1065-1078, the subtraction and everything after it in float64
//   w[b,p,a,k,n] = relu(1 - |g - A_a kappa_k|^2 / sigma)         L1112 (L2508-2549)
//   perm[b,p,n,a] = argmax_j tr(R_rel^T A_a A_j^T)               L1199-1204 = mult[argmax_g tr(R_rel A_g)][a], see csrc/so3_inter.hip
//   X[b,c,k,p,a] = sum_n feats[b,c,idx_n,perm_n(a)] w(p,a,k,n)   L1221-1261
//   Y = W X                                                      modules.py:L48-55
//
//   so3_prep_f64          g (three doubles) and the nearest-anchor index per (point, neighbour), the per-cloud flag
//   so3_inter_weights_f64 the materialised inter_w, in the operation order of the torch expression
//   so3_inter_group_fwd   X with w evaluated in registers (lane = anchor, the waves split the kernel points)
//   inv_lists_entries     the second half of the index-only inverse lists of csrc/inv_lists.hip: the ENTRY numbers p * nn + n of
//                         every referenced row, in entry order (any p * nn)
//   so3_inter_group_bwd   the transpose into dF: one workgroup per referenced row walks its entries in that order, one lane per
//                         OUTPUT anchor (the inverse permutation table), sums over k then over the entries: no atomics, one order
//   gemm_f64 (+ _reduce)  v_mfma_f64_16x16x4_f64 over strided views: Y_z = W X_z, dX_z = W^T gY_z, dW = sum_z gY_z X_z^T (every
//                         item's product from zero, then added in index order)
// The intra grouping pair in float64 is csrc/so3_intra.hip's kernels at V = double.
#include <string.h>

#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

inline double from_bits(int64_t bits) {
    double d;
    memcpy(&d, &bits, sizeof d);
    return d;
}

// ---------------------------------------------------------------------------------------------
// prep
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void so3_prep_f64_kernel(
    int p, int n_sup, int nn, int na, const double *__restrict__ q_xyz, const double *__restrict__ s_xyz,
    const int32_t *__restrict__ idx, const double *__restrict__ q_pose, const double *__restrict__ s_pose,
    const double *__restrict__ anchors, int identity_anchor, double *__restrict__ g_out, int32_t *__restrict__ r_out,
    int32_t *__restrict__ nonident) {
    __shared__ double s_anchor[64 * 9];
    for (int i = threadIdx.x; i < na * 9; i += blockDim.x) s_anchor[i] = anchors[i];
    __syncthreads();
    const int bi = blockIdx.y;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)p * nn) return;
    const int pi = (int)(e / nn);
    const int q = idx[(size_t)bi * p * nn + e];
    const double *Q = q_xyz + (size_t)bi * 3 * p;
    const double *X = s_xyz + (size_t)bi * 3 * n_sup;
    // the neighbour's coordinates pass through float32 (group_nd); index n_sup = the shadow point at 1e4 (spconv/functional.py:L83-87)
    const double sx = q < n_sup ? (double)(float)X[q] : 1e4, sy = q < n_sup ? (double)(float)X[n_sup + q] : 1e4,
                 sz = q < n_sup ? (double)(float)X[2 * (size_t)n_sup + q] : 1e4;
    double dx = sx - Q[pi], dy = sy - Q[p + pi], dz = sz - Q[2 * (size_t)p + pi];
    int r = identity_anchor;
    if (q_pose != nullptr) {
        const double *Rp = q_pose + ((size_t)bi * p + pi) * 16;
        const double *Rn = s_pose + ((size_t)bi * n_sup + min(q, n_sup - 1)) * 16;
        double R[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)   // R_rel = R_p R_n^T
                R[i][j] = Rp[i * 4 + 0] * Rn[j * 4 + 0] + Rp[i * 4 + 1] * Rn[j * 4 + 1] + Rp[i * 4 + 2] * Rn[j * 4 + 2];
        const double gx_ = R[0][0] * dx + R[0][1] * dy + R[0][2] * dz;
        const double gy_ = R[1][0] * dx + R[1][1] * dy + R[1][2] * dz;
        const double gz_ = R[2][0] * dx + R[2][1] * dy + R[2][2] * dz;
        dx = gx_; dy = gy_; dz = gz_;
        double best = -1e300;
        for (int g = 0; g < na; ++g) {   // first maximum wins
            const double *A = s_anchor + g * 9;   // tr(R A_g) = sum_ij R[i][j] A[j][i]
            const double t = R[0][0] * A[0] + R[0][1] * A[3] + R[0][2] * A[6] +
                             R[1][0] * A[1] + R[1][1] * A[4] + R[1][2] * A[7] +
                             R[2][0] * A[2] + R[2][1] * A[5] + R[2][2] * A[8];
            if (t > best) { best = t; r = g; }
        }
    }
    double *go = g_out + ((size_t)bi * p * nn + e) * 3;
    go[0] = dx; go[1] = dy; go[2] = dz;
    r_out[(size_t)bi * p * nn + e] = r;
    if (nonident != nullptr && __any(r != identity_anchor) && (threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1)
        atomicOr(nonident + bi, 1);
}

// ---------------------------------------------------------------------------------------------
// materialised kernel weights  w[b,p,a,k,n]
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double kernel_weight_exact(double gx, double gy, double gz, double kx, double ky, double kz, double sigma) {
#pragma clang fp contract(off)
    // the operation order of torch: sum((g - rk)^2), then 1 - d / sigma, one rounding each
    const double dx = gx - kx, dy = gy - ky, dz = gz - kz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return fmax(1.0 - d2 / sigma, 0.0);
}

__global__ __launch_bounds__(256) void so3_inter_weights_f64_kernel(int p, int nn, int na, int ks, double sigma, const double *__restrict__ g,
                                                                    const double *__restrict__ rk, double *__restrict__ w) {
    extern __shared__ double s_g[];      // [nn*3]
    const int pi = blockIdx.x, bi = blockIdx.y;
    const size_t pn = ((size_t)bi * p + pi) * nn;
    for (int i = threadIdx.x; i < nn * 3; i += blockDim.x) s_g[i] = g[pn * 3 + i];
    __syncthreads();
    double *wp = w + pn * na * ks;
    const int total = na * ks * nn;
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int n = e % nn, ak = e / nn;
        const double *k = rk + (size_t)ak * 3;
        wp[e] = kernel_weight_exact(s_g[3 * n], s_g[3 * n + 1], s_g[3 * n + 2], k[0], k[1], k[2], sigma);
    }
}

// the weight as the grouping kernels evaluate it (forward and transpose alike)
__device__ __forceinline__ double kernel_weight(double gx, double gy, double gz, double kx, double ky, double kz, double inv_sigma) {
    const double dx = gx - kx, dy = gy - ky, dz = gz - kz;
    return fmax(1.0 - (dx * dx + dy * dy + dz * dz) * inv_sigma, 0.0);
}

// ---------------------------------------------------------------------------------------------
// fused grouping, forward:  out[b,c,k,p,a] = sum_n feats[b,c,idx_n,perm_n(a)] * w(p,a,k,n)
//   block = one point, 4 waves = 4 groups of KPW kernel points, lane = anchor, CC channels per pass
// ---------------------------------------------------------------------------------------------
constexpr int G_THREADS = 256;

template <int KPW, int CC>
__global__ __launch_bounds__(G_THREADS) void so3_inter_group_fwd_f64_kernel(
    int c, int p, int n_sup, int nn, int na, int ks, double inv_sigma, const double *__restrict__ feats,
    const int32_t *__restrict__ idx, const double *__restrict__ g, const int32_t *__restrict__ rr,
    const double *__restrict__ rk, const uint8_t *__restrict__ mult, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *s_g = reinterpret_cast<double *>(smem);                              // [nn*3]
    int32_t *s_q = reinterpret_cast<int32_t *>(smem + 24 * (size_t)nn);          // [nn]
    int32_t *s_r = s_q + nn;                                                     // [nn]
    uint8_t *s_mult = smem + 32 * (size_t)nn;                                    // [na*na] (only if mult)

    const int pi = blockIdx.x, bi = blockIdx.y;
    const size_t pn = ((size_t)bi * p + pi) * nn;
    for (int i = threadIdx.x; i < nn * 3; i += G_THREADS) s_g[i] = g[pn * 3 + i];
    for (int i = threadIdx.x; i < nn; i += G_THREADS) {
        const int q = idx[pn + i];
        s_q[i] = (q >= 0 && q < n_sup) ? q : -1;   // shadow row (all zeros in the reference) -> skipped
        s_r[i] = rr[pn + i];
    }
    if (mult != nullptr)
        for (int i = threadIdx.x; i < na * na; i += G_THREADS) s_mult[i] = mult[i];
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k0 = wave * KPW;
    if (lane >= na || k0 >= ks) return;

    double kx[KPW], ky[KPW], kz[KPW];
#pragma unroll
    for (int kk = 0; kk < KPW; ++kk) {
        const int k = min(k0 + kk, ks - 1);
        const double *r3 = rk + ((size_t)lane * ks + k) * 3;
        kx[kk] = r3[0]; ky[kk] = r3[1]; kz[kk] = r3[2];
    }
    const double *fb = feats + (size_t)bi * c * n_sup * na;
    const size_t f_cs = (size_t)n_sup * na;
    double *ob = out + (size_t)bi * c * ks * p * na + (size_t)pi * na + lane;
    const size_t o_ks = (size_t)p * na, o_cs = (size_t)ks * p * na;

    for (int c0 = 0; c0 < c; c0 += CC) {
        double acc[CC][KPW];
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
#pragma unroll
            for (int kk = 0; kk < KPW; ++kk) acc[cc][kk] = 0.0;

        for (int n = 0; n < nn; ++n) {
            const int q = s_q[n];
            if (q < 0) continue;   // wave-uniform
            const double gx = s_g[3 * n], gy = s_g[3 * n + 1], gz = s_g[3 * n + 2];
            double wv[KPW];
#pragma unroll
            for (int kk = 0; kk < KPW; ++kk) wv[kk] = kernel_weight(gx, gy, gz, kx[kk], ky[kk], kz[kk], inv_sigma);
            const int a_src = mult != nullptr ? (int)s_mult[s_r[n] * na + lane] : lane;
            const double *f = fb + (size_t)q * na + a_src;
#pragma unroll
            for (int cc = 0; cc < CC; ++cc) {
                const double fv = (c0 + cc < c) ? f[(size_t)(c0 + cc) * f_cs] : 0.0;
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk) acc[cc][kk] = fma(fv, wv[kk], acc[cc][kk]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
            if (c0 + cc < c) {
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk)
                    if (k0 + kk < ks) ob[(size_t)(c0 + cc) * o_cs + (size_t)(k0 + kk) * o_ks] = acc[cc][kk];
            }
    }
}

// ---------------------------------------------------------------------------------------------
// inverse lists, second half: the entry numbers of every referenced row, in entry order
//   one workgroup (4 waves) per (row slot, cloud); wave w scans the w-th quarter of the cloud's entries twice: count, then place
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inv_entries_kernel(int per_cloud, int rld, const int32_t *__restrict__ idx,
                                                          const int32_t *__restrict__ rows, const int32_t *__restrict__ off,
                                                          int32_t *__restrict__ ent) {
    __shared__ int s_wave[4];
    const int r = blockIdx.x, bi = blockIdx.y;
    const int q = rows[(size_t)bi * rld + r];
    if (q < 0) return;                                       // block-uniform
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (per_cloud + 3) / 4;
    const int beg = min(per_cloud, wave * per), end = min(per_cloud, beg + per);
    const int32_t *src = idx + (size_t)bi * per_cloud;
    int mine = 0;
    for (int i = beg + lane; i < end; i += 64) mine += (src[i] == q);
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    int base = off[(size_t)bi * rld + r];
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    int32_t *dst = ent + (size_t)bi * per_cloud;
    for (int i0 = beg; i0 < end; i0 += 64) {                 // wave-uniform trip count
        const int i = i0 + lane;
        const bool m = i < end && src[i] == q;
        const unsigned long long bal = __ballot(m);
        if (bal == 0ull) continue;
        const int pos = base + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
        if (m && pos < per_cloud) dst[pos] = i;
        base += __popcll(bal);
    }
}

// ---------------------------------------------------------------------------------------------
// fused grouping, transpose:  gfeats[b,c,q,a'] = sum over the entries (p,n) of row q, in entry order, of
//                                               sum_k w(p,a,k,n) gout[b,c,k,p,a],   a = the anchor with perm_n(a) = a'
//   block = one referenced row x 4 CW channels (grid.y walks the channels: the lists of a cloud that takes its first nn neighbours in
//   index order are few and long -- ~270 rows of up to 3800 entries at 4096 points -- so the rows alone do not fill the chip); lane = a';
//   wave w owns channels [c0 + w CW, c0 + (w + 1) CW).  The walk along a list is a chain of dependent loads (entry -> g, r -> gout), and the
//   longest list is the kernel's critical path: the block stages 64 entries' numbers in LDS at a time, and the k loop is unrolled in full
//   (KS = 24 or 32) so that the KS x CW loads of an entry are all in flight together.
// ---------------------------------------------------------------------------------------------
constexpr int BWD_STAGE = 64;

template <int KS, int CW>
__global__ __launch_bounds__(G_THREADS) void so3_inter_group_bwd_f64_kernel(
    int c, int p, int n_sup, int nn, int na, int ks, double inv_sigma, const double *__restrict__ gout,
    const int32_t *__restrict__ rows, const int32_t *__restrict__ off, const int32_t *__restrict__ cnt,
    const int32_t *__restrict__ ent, const double *__restrict__ g, const int32_t *__restrict__ rr,
    const double *__restrict__ rk, const uint8_t *__restrict__ multinv, double *__restrict__ gfeats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *s_rk = reinterpret_cast<double *>(smem);                             // [na*ks*3]
    uint8_t *s_minv = smem + 24 * (size_t)na * ks;                               // [na*na] (only if multinv)
    __shared__ double s_g[BWD_STAGE * 3];
    __shared__ int32_t s_e[BWD_STAGE], s_r[BWD_STAGE];
    const int slot = blockIdx.x, bi = blockIdx.z;
    const int q = rows[(size_t)bi * n_sup + slot];
    if (q < 0 || q >= n_sup) return;                                             // block-uniform: an unreferenced slot (gfeats is zeroed)
    for (int i = threadIdx.x; i < na * ks * 3; i += G_THREADS) s_rk[i] = rk[i];
    if (multinv != nullptr)
        for (int i = threadIdx.x; i < na * na; i += G_THREADS) s_minv[i] = multinv[i];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long per_cloud = (long long)p * nn;
    const int beg = off[(size_t)bi * n_sup + slot];
    const int len = min(cnt[(size_t)bi * n_sup + slot], (int)max(0ll, per_cloud - beg));      // block-uniform
    const int32_t *el = ent + (size_t)bi * per_cloud + beg;
    const double *gb = g + (size_t)bi * per_cloud * 3;
    const int32_t *rb = rr + (size_t)bi * per_cloud;
    const double *ob = gout + (size_t)bi * c * ks * p * na;
    const size_t o_ks = (size_t)p * na, o_cs = (size_t)ks * p * na;
    const int c0 = (blockIdx.y * 4 + wave) * CW;
    const bool active = lane < na && c0 < c;

    double acc[CW];
#pragma unroll
    for (int cc = 0; cc < CW; ++cc) acc[cc] = 0.0;
    for (int m0 = 0; m0 < len; m0 += BWD_STAGE) {
        const int staged = min(BWD_STAGE, len - m0);
        __syncthreads();                                                         // (the tables above; the previous stage is consumed)
        if (threadIdx.x < staged) {
            int e = el[m0 + threadIdx.x];
            if (e < 0 || e >= per_cloud) e = -1;
            s_e[threadIdx.x] = e;
            s_r[threadIdx.x] = e < 0 ? 0 : (rb[e] & 63);
            s_g[3 * threadIdx.x] = e < 0 ? 0.0 : gb[3 * (size_t)e];
            s_g[3 * threadIdx.x + 1] = e < 0 ? 0.0 : gb[3 * (size_t)e + 1];
            s_g[3 * threadIdx.x + 2] = e < 0 ? 0.0 : gb[3 * (size_t)e + 2];
        }
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < staged; ++j) {
            const int e = s_e[j];                                                // wave-uniform
            if (e < 0) continue;
            const int pi = e / nn;
            const double gx = s_g[3 * j], gy = s_g[3 * j + 1], gz = s_g[3 * j + 2];
            const int a = multinv != nullptr ? (int)s_minv[s_r[j] * na + lane] : lane;
            const double *k3 = s_rk + (size_t)a * ks * 3;
            const double *o = ob + (size_t)pi * na + a;
            double v[CW][KS];
#pragma unroll
            for (int cc = 0; cc < CW; ++cc)
#pragma unroll
                for (int k = 0; k < KS; ++k) v[cc][k] = (c0 + cc < c && k < ks) ? o[(size_t)(c0 + cc) * o_cs + (size_t)k * o_ks] : 0.0;
            double t[CW];
#pragma unroll
            for (int cc = 0; cc < CW; ++cc) t[cc] = 0.0;
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                if (k < ks) {
                    const double wv = kernel_weight(gx, gy, gz, k3[3 * k], k3[3 * k + 1], k3[3 * k + 2], inv_sigma);
#pragma unroll
                    for (int cc = 0; cc < CW; ++cc) t[cc] = fma(wv, v[cc][k], t[cc]);
                }
            }
#pragma unroll
            for (int cc = 0; cc < CW; ++cc) acc[cc] += t[cc];
        }
    }
    if (active) {
        double *fo = gfeats + ((size_t)bi * c * n_sup + q) * na + lane;
        const size_t f_cs = (size_t)n_sup * na;
#pragma unroll
        for (int cc = 0; cc < CW; ++cc)
            if (c0 + cc < c) fo[(size_t)(c0 + cc) * f_cs] = acc[cc];
    }
}

// ---------------------------------------------------------------------------------------------
// GEMM on v_mfma_f64_16x16x4_f64.  Operands by element strides (rs, cs) = (row, column): a transposed view swaps them.
//   lane l of an MFMA holds A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15]; its four results are
//   C[row = (l >> 4) + 4 reg][col = l & 15]  (NOT the f32 map row = 4 (l >> 4) + reg).
//   block = 4 waves as 2 x 2, a wave owns 32 x 32 of C (2 x 2 MFMA tiles); a k-step of 16: lane group h = l >> 4 owns the four
//   consecutive k = k0 + 4 h + j and feeds them to MFMA j (one order for every run).  Rows, columns and k past the operand are
//   SELECTED as zero, never loaded.
//   REDUCE: C = (C if accumulate else 0) + P_0 + P_1 + ... in item order, every P_z accumulated from zero.
// ---------------------------------------------------------------------------------------------
template <bool REDUCE>
__global__ __launch_bounds__(256) void gemm_f64_kernel(int M, int N, int K, const double *__restrict__ A, long long a_rs, long long a_cs,
                                                       long long strideA, const double *__restrict__ B, long long b_rs, long long b_cs,
                                                       long long strideB, double *__restrict__ C, long long ldc, long long strideC, int batch,
                                                       int accumulate) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, h = lane >> 4;
    const long long m0 = (long long)blockIdx.y * 64 + (wave >> 1) * 32, n0 = (long long)blockIdx.x * 64 + (wave & 1) * 32;
    if (m0 >= M || n0 >= N) return;
    const bool am[2] = {m0 + r < M, m0 + 16 + r < M};
    const bool bn[2] = {n0 + r < N, n0 + 16 + r < N};
    const int z0 = REDUCE ? 0 : blockIdx.z, z1 = REDUCE ? batch : blockIdx.z + 1;
    f64x4 total[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) total[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    if (REDUCE && accumulate) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const long long row = m0 + 16 * i + h + 4 * v, col = n0 + 16 * j + r;
                    if (row < M && col < N) total[i][j][v] = C[row * ldc + col];
                }
    }
    for (int z = z0; z < z1; ++z) {
        const double *Az = A + (long long)z * strideA + (m0 + r) * a_rs;
        const double *Bz = B + (long long)z * strideB + (n0 + r) * b_cs;
        f64x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long kk = k0 + 4 * h + j;
                const bool kin = kk < K;
                const double a0 = (kin && am[0]) ? Az[kk * a_cs] : 0.0;
                const double a1 = (kin && am[1]) ? Az[16 * a_rs + kk * a_cs] : 0.0;
                const double b0 = (kin && bn[0]) ? Bz[kk * b_rs] : 0.0;
                const double b1 = (kin && bn[1]) ? Bz[16 * b_cs + kk * b_rs] : 0.0;
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (REDUCE) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) total[i][j] += acc[i][j];
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) total[i][j] = acc[i][j];
        }
    }
    double *Cz = C + (REDUCE ? 0 : (long long)blockIdx.z * strideC);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const long long row = m0 + 16 * i + h + 4 * v, col = n0 + 16 * j + r;
                if (row < M && col < N) Cz[row * ldc + col] = total[i][j][v];
            }
}

int gemm_f64(bool reduce, int transA, int transB, int M, int N, int K, const double *A, int64_t lda, int64_t strideA, const double *B,
             int64_t ldb, int64_t strideB, double *C, int64_t ldc, int64_t strideC, int batch, int accumulate, hipStream_t s) {
    const char *what = reduce ? "gemm_f64_reduce" : "gemm_f64";
    if (M <= 0 || N <= 0 || (!reduce && batch <= 0)) return 0;
    if (K < 0 || batch < 0) return eap::bad_arg("gemm_f64: negative K or batch");
    if (A == nullptr || B == nullptr || C == nullptr) return eap::bad_arg("gemm_f64: null operand");
    const long long a_rs = transA ? 1 : lda, a_cs = transA ? lda : 1, b_rs = transB ? 1 : ldb, b_cs = transB ? ldb : 1;
    eap::set_kernel(reduce ? "gemm_f64_kernel<true>" : "gemm_f64_kernel<false>");
    if (reduce)
        return eap::run_kernel(what, gemm_f64_kernel<true>, eap::cdiv(N, 64), eap::cdiv(M, 64), 1, dim3(256), 0, s, M, N, K, A, a_rs, a_cs,
                               (long long)strideA, B, b_rs, b_cs, (long long)strideB, C, (long long)ldc, 0ll, batch, accumulate);
    return eap::run_kernel(what, gemm_f64_kernel<false>, eap::cdiv(N, 64), eap::cdiv(M, 64), batch, dim3(256), 0, s, M, N, K, A, a_rs, a_cs,
                           (long long)strideA, B, b_rs, b_cs, (long long)strideB, C, (long long)ldc, (long long)strideC, batch, 0);
}

// the limits the grouping entries share, checked before anything is touched
const char *group_refusal(long long b, long long p, long long nn, int na, int ks) {
    if (na > 64) return "so3 float64: at most 64 anchors";
    if (ks > 32) return "so3 float64: at most 32 kernel points";
    if (b > 65535) return "so3 float64: at most 65535 clouds per call (grid.y)";
    if (p * nn >= (1ll << 31)) return "so3 float64: more than 2^31 entries per cloud";
    return nullptr;
}

}  // namespace

extern "C" int eap_so3_prep_f64(int b, int p, int n, int nn, int na, const double *q_xyz, const double *s_xyz, const int32_t *idx,
                                const double *q_pose, const double *s_pose, const double *anchors, int identity_anchor, double *g,
                                int32_t *r, int32_t *nonident, eap_stream_t stream) {
    if (b <= 0 || p <= 0 || nn <= 0) return 0;
    if (na <= 0) return eap::bad_arg("so3_prep_f64: 1..64 anchors supported");
    if (const char *why = group_refusal(b, p, nn, na, 0)) return eap::bad_arg(why);
    if ((q_pose == nullptr) != (s_pose == nullptr)) return eap::bad_arg("so3_prep_f64: pass both poses or none");
    if (nonident != nullptr) {
        int e = eap::hip_fail(hipMemsetAsync(nonident, 0, sizeof(int32_t) * b, eap::S(stream)), "so3_prep_f64 memset");
        if (e) return e;
    }
    eap::set_kernel("so3_prep_f64_kernel");
    return eap::run_kernel("so3_prep_f64", so3_prep_f64_kernel, eap::cdiv((long long)p * nn, 256), b, 1, dim3(256), 0, eap::S(stream), p, n, nn, na,
                           q_xyz, s_xyz, idx, q_pose, s_pose, anchors, identity_anchor, g, r, nonident);
}

extern "C" int eap_so3_inter_weights_f64(int b, int p, int nn, int na, int ks, int64_t sigma_bits, const double *g, const double *rk,
                                         double *w, eap_stream_t stream) {
    if (b <= 0 || p <= 0 || nn <= 0 || na <= 0 || ks <= 0) return 0;
    if (const char *why = group_refusal(b, p, nn, 0, 0)) return eap::bad_arg(why);
    if ((long long)na * ks * nn >= (1ll << 31)) return eap::bad_arg("so3_inter_weights_f64: more than 2^31 weights per point");
    eap::set_kernel("so3_inter_weights_f64_kernel");
    return eap::run_kernel("so3_inter_weights_f64", so3_inter_weights_f64_kernel, p, b, 1, dim3(256), 24 * (size_t)nn, eap::S(stream), p, nn, na, ks,
                           from_bits(sigma_bits), g, rk, w);
}

extern "C" int eap_so3_inter_group_fwd_f64(int b, int c, int p, int n, int nn, int na, int ks, int64_t sigma_bits, const double *feats,
                                           const int32_t *idx, const double *g, const int32_t *r, const double *rk, const uint8_t *mult,
                                           double *out, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || p <= 0 || na <= 0 || ks <= 0) return 0;
    if (const char *why = group_refusal(b, p, nn, na, ks)) return eap::bad_arg(why);
    hipStream_t s = eap::S(stream);
    if (nn <= 0) return eap::hip_fail(hipMemsetAsync(out, 0, sizeof(double) * (size_t)b * c * ks * p * na, s), "so3_inter_group_fwd_f64 memset");
    const size_t shmem = 32 * (size_t)nn + (mult ? (size_t)na * na : 0);
    const double inv_sigma = 1.0 / from_bits(sigma_bits);
    // KPW kernel points per wave (4 waves: 24 or 32), CC channels per pass (2 for a narrow input: the first layers)
    eap::set_kernel("so3_inter_group_fwd_f64_kernel");
    auto kern = ks <= 24 ? so3_inter_group_fwd_f64_kernel<6, 8> : so3_inter_group_fwd_f64_kernel<8, 8>;
    if (c < 8) kern = ks <= 24 ? so3_inter_group_fwd_f64_kernel<6, 2> : so3_inter_group_fwd_f64_kernel<8, 2>;
    return eap::run_kernel("so3_inter_group_fwd_f64", kern, p, b, 1, dim3(G_THREADS), shmem, s, c, p, n, nn, na, ks, inv_sigma, feats, idx, g, r, rk,
                           mult, out);
}

extern "C" int eap_inv_lists_entries(int b, int p, int n, int nn, const int32_t *idx, const int32_t *rows, const int32_t *off, int32_t *ent,
                                     eap_stream_t stream) {
    if (b <= 0 || p <= 0 || nn <= 0 || n <= 0) return 0;
    if (const char *why = group_refusal(b, p, nn, 0, 0)) return eap::bad_arg(why);
    if (n > 16384) return eap::bad_arg("inv_lists_entries: more than 16384 support points per cloud");
    eap::set_kernel("inv_entries_kernel");
    return eap::run_kernel("inv_lists_entries", inv_entries_kernel, n, b, 1, dim3(256), 0, eap::S(stream), p * nn, n, idx, rows, off, ent);
}

extern "C" int eap_so3_inter_group_bwd_f64(int b, int c, int p, int n, int nn, int na, int ks, int64_t sigma_bits, const double *gout,
                                           const int32_t *rows, const int32_t *off, const int32_t *cnt, const int32_t *ent, const double *g,
                                           const int32_t *r, const double *rk, const uint8_t *multinv, double *gfeats, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || n <= 0 || na <= 0) return 0;
    if (const char *why = group_refusal(b, p, nn, na, ks)) return eap::bad_arg(why);
    if (n > 16384) return eap::bad_arg("so3_inter_group_bwd_f64: more than 16384 support points per cloud (the inverse lists)");
    if (c > 16 * 65535) return eap::bad_arg("so3_inter_group_bwd_f64: more than 16 x 65535 channels (grid.y)");
    hipStream_t s = eap::S(stream);
    int e = eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(double) * (size_t)b * c * n * na, s), "so3_inter_group_bwd_f64 memset");
    if (e || p <= 0 || nn <= 0 || ks <= 0) return e;
    const size_t shmem = 24 * (size_t)na * ks + (multinv ? (size_t)na * na : 0);
    eap::set_kernel(ks <= 24 ? "so3_inter_group_bwd_f64_kernel<24, 4>" : "so3_inter_group_bwd_f64_kernel<32, 4>");
    return eap::run_kernel("so3_inter_group_bwd_f64", ks <= 24 ? so3_inter_group_bwd_f64_kernel<24, 4> : so3_inter_group_bwd_f64_kernel<32, 4>, n, eap::cdiv(c, 16), b,
                           dim3(G_THREADS), shmem, s, c, p, n, nn, na, ks, 1.0 / from_bits(sigma_bits), gout, rows, off, cnt, ent, g, r, rk, multinv, gfeats);
}

extern "C" int eap_gemm_f64(int transA, int transB, int M, int N, int K, const double *A, int64_t lda, int64_t strideA, const double *B,
                            int64_t ldb, int64_t strideB, double *C, int64_t ldc, int64_t strideC, int batch, eap_stream_t stream) {
    return gemm_f64(false, transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, batch, 0, eap::S(stream));
}

extern "C" int eap_gemm_f64_reduce(int transA, int transB, int M, int N, int K, const double *A, int64_t lda, int64_t strideA, const double *B,
                                   int64_t ldb, int64_t strideB, double *C, int64_t ldc, int batch, int accumulate, eap_stream_t stream) {
    return gemm_f64(true, transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, 0, batch, accumulate, eap::S(stream));
}
