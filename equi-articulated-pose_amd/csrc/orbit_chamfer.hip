// csrc/orbit_chamfer.hip -- the reconstruction distances over the orbit on gfx950, float32 and float64
// (reference: SPConvNets/models/unsup_seg_so3_pose_conv_pn_38_multi_stage.py L1341-1361, per slot with its membership mask, and
//  L429-440, the global alignment without one).
//
// G = B * S groups of A posed candidate clouds of M points each, all compared with ONE input cloud of N points per group (the cloud
// of group g is g / S, read planar [B,3,N] as the model holds it), and a per-point membership flag instead of a second, masked copy of
// the cloud.  The loop shape and the arithmetic are csrc/chamfer.hip's: one lane per query, the other side streams through LDS in
// 1024-entry tiles, every squared distance is (dx*dx + dy*dy) + dz*dz with one rounding per operation (built with -ffp-contract=off),
// strict `<` so the first minimum wins -- distances and indices are those of chamfer_nn_kernel on the expanded clouds, bit for bit.
//
//   recon -> ori : one scan keeps two (min, argmin) pairs: over every point, and over the flagged points only, the latter starting at
//                  (99999, -1) so that an empty slot gives the reference's constant and an index that names no point.
//   ori -> recon : one lane per input point, the M points of one candidate cloud in LDS; the masked map is written by the same lane.
//   backward     : a gather in a fixed order like chamfer_grad_ordered_kernel -- no atomics, every element of grecon written once.
#include "common.h"

namespace {

constexpr int OC_THREADS = 256;
constexpr int OC_TILE = 1024;
constexpr double OC_MASKED = 99999.0;      // what the reference writes into the masked entries of its distance tensor

__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }

// |c - q|^2 in chamfer_nn_kernel's order (c the candidate from the tile, q the lane's query)
template <typename T>
__device__ __forceinline__ T dist2(T cx, T cy, T cz, T qx, T qy, T qz) {
    const T dx = sub_rn(cx, qx), dy = sub_rn(cy, qy), dz = sub_rn(cz, qz);
    return add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
}

template <typename T> struct alignas(4 * sizeof(T)) Entry { T x, y, z, w; };   // 16 bytes in float: one broadcast read per candidate

// recon -> ori.  Lane = query (g, j), j in [0, q) with q = A * M; grid (cdiv(q, 256), G).  tile entry = (x, y, z, flag).
// (LDS: 16 KB for float, 32 KB for double)
template <typename T, bool MASKED>
__global__ __launch_bounds__(OC_THREADS) void orbit_recon_to_ori_kernel(
    int q, int n, int s, const T *__restrict__ recon, const T *__restrict__ ori, const uint8_t *__restrict__ member,
    T *__restrict__ d_all, int32_t *__restrict__ i_all, T *__restrict__ d_in, int32_t *__restrict__ i_in) {
    __shared__ Entry<T> tile[OC_TILE];
    const int g = blockIdx.y;
    const int j = blockIdx.x * OC_THREADS + threadIdx.x;
    const T *p = recon + ((size_t)g * q + min(j, q - 1)) * 3;
    const T qx = p[0], qy = p[1], qz = p[2];
    const T *cloud = ori + (size_t)(g / s) * 3 * n;
    const uint8_t *flag = MASKED ? member + (size_t)g * n : nullptr;
    // candidate 0 starts the unmasked pair, whatever its value (as chamfer_nn_kernel's `k == 0 ||`); the scan meets it again and leaves it
    T best = dist2(cloud[0], cloud[n], cloud[2 * (size_t)n], qx, qy, qz);
    int besti = 0;
    T best_in = (T)OC_MASKED;
    int besti_in = -1;
    for (int k0 = 0; k0 < n; k0 += OC_TILE) {
        const int len = min(OC_TILE, n - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < len; t += OC_THREADS) {
            Entry<T> e;
            e.x = cloud[k0 + t];
            e.y = cloud[(size_t)n + k0 + t];
            e.z = cloud[2 * (size_t)n + k0 + t];
            e.w = MASKED ? (T)(flag[k0 + t] != 0) : (T)1;
            tile[t] = e;
        }
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const Entry<T> e = tile[k];
            const T d = dist2(e.x, e.y, e.z, qx, qy, qz);
            if (d < best) { best = d; besti = k0 + k; }
            if (MASKED && e.w != (T)0 && d < best_in) { best_in = d; besti_in = k0 + k; }
        }
    }
    if (j < q) {
        const size_t o = (size_t)g * q + j;
        d_all[o] = best;
        i_all[o] = besti;
        if (MASKED) {
            d_in[o] = best_in;
            i_in[o] = besti_in;
        }
    }
}

// ori -> recon.  Lane = input point i of (g, a); grid (cdiv(N, 256), A, G); the candidate cloud's M points stream through LDS.
// (LDS: 12 KB for float, 24 KB for double)
template <typename T, bool MASKED>
__global__ __launch_bounds__(OC_THREADS) void orbit_ori_to_recon_kernel(
    int m, int n, int s, const T *__restrict__ recon, const T *__restrict__ ori, const uint8_t *__restrict__ member,
    T *__restrict__ d_all, int32_t *__restrict__ index, T *__restrict__ d_in) {
    __shared__ T tile[OC_TILE * 3];
    const int a = blockIdx.y, na = gridDim.y, g = blockIdx.z;
    const int i = blockIdx.x * OC_THREADS + threadIdx.x;
    const T *cloud = ori + (size_t)(g / s) * 3 * n;
    const int ic = min(i, n - 1);
    const T qx = cloud[ic], qy = cloud[(size_t)n + ic], qz = cloud[2 * (size_t)n + ic];
    const T *c = recon + ((size_t)g * na + a) * m * 3;
    T best = 0;
    int besti = 0;
    for (int k0 = 0; k0 < m; k0 += OC_TILE) {
        const int len = min(OC_TILE, m - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < len * 3; t += OC_THREADS) tile[t] = c[(size_t)k0 * 3 + t];
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const T d = dist2(tile[k * 3 + 0], tile[k * 3 + 1], tile[k * 3 + 2], qx, qy, qz);
            if ((k0 + k) == 0 || d < best) { best = d; besti = k0 + k; }
        }
    }
    if (i < n) {
        const size_t o = ((size_t)g * na + a) * n + i;
        d_all[o] = best;
        index[o] = besti;
        if (MASKED) d_in[o] = member[(size_t)g * n + i] != 0 ? best : (T)OC_MASKED;
    }
}

// The ordered backward: lane (g, a, j) owns grecon[g,a,j,:]; grid (cdiv(M, 256), A, G).
//   acc = ((0 + own_all) + own_in) + entries,   own_x = (2 g_r2o_x[g,a,j]) * (recon - ori[idx_x]), skipped where idx_x names no point
//   entries: input points i ascending with idx_o2r[g,a,i] == j:  (2 (g_o2r_all[g,a,i] + member * g_o2r_in[g,a,i])) * (recon - ori[i])
// g_o2r_in / the masked own term are absent when MASKED is false.  An index outside its range is neither matched nor dereferenced.
// (LDS per 1024-entry tile: 4 KB of indices + 16 KB of (2 g, xyz) for float, 32 KB for double.)
template <typename T, bool MASKED>
__global__ __launch_bounds__(OC_THREADS) void orbit_grad_ordered_kernel(
    int m, int n, int s, const T *__restrict__ recon, const T *__restrict__ ori, const uint8_t *__restrict__ member,
    const int32_t *__restrict__ idx_all, const int32_t *__restrict__ idx_in, const int32_t *__restrict__ idx_o2r,
    const T *__restrict__ g_r2o_all, const T *__restrict__ g_r2o_in, const T *__restrict__ g_o2r_all, const T *__restrict__ g_o2r_in,
    T *__restrict__ grecon) {
    __shared__ __align__(16) int32_t tile_idx[OC_TILE];
    __shared__ __align__(16) T tile_v[OC_TILE * 4];                 // (2 g, x, y, z) per entry
    const int a = blockIdx.y, na = gridDim.y, g = blockIdx.z;
    const int j = blockIdx.x * OC_THREADS + threadIdx.x;
    const bool live = j < m;
    const size_t row = ((size_t)g * na + a) * m + (live ? j : m - 1);
    const T *cloud = ori + (size_t)(g / s) * 3 * n;
    const T x[3] = {recon[row * 3 + 0], recon[row * 3 + 1], recon[row * 3 + 2]};
    T acc[3] = {0, 0, 0};
    {
        const int k = idx_all[row];
        if (k >= 0 && k < n) {
            const T w = g_r2o_all[row] * 2;
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[d] += w * (x[d] - cloud[(size_t)d * n + k]);
        }
    }
    if (MASKED) {
        const int k = idx_in[row];
        if (k >= 0 && k < n) {
            const T w = g_r2o_in[row] * 2;
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[d] += w * (x[d] - cloud[(size_t)d * n + k]);
        }
    }
    const int key = live ? j : -1;                    // (a lane past the end matches nothing: it only helps to load the tiles)
    const size_t o0 = ((size_t)g * na + a) * n;
    for (int k0 = 0; k0 < n; k0 += OC_TILE) {
        const int len = min(OC_TILE, n - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < OC_TILE; t += OC_THREADS) {
            if (t >= len) { tile_idx[t] = -2; continue; }           // (the walk below reads whole groups of 8)
            const int i = k0 + t;
            const int32_t to = idx_o2r[o0 + i];
            tile_idx[t] = (to >= 0 && to < m) ? to : -2;
            T w = g_o2r_all[o0 + i];
            if (MASKED && member[(size_t)g * n + i] != 0) w = w + g_o2r_in[o0 + i];
            tile_v[t * 4 + 0] = w * 2;
            tile_v[t * 4 + 1] = cloud[i];
            tile_v[t * 4 + 2] = cloud[(size_t)n + i];
            tile_v[t * 4 + 3] = cloud[2 * (size_t)n + i];
        }
        __syncthreads();
        for (int k = 0; k < len; k += 8) {
            const int4 lo = *reinterpret_cast<const int4 *>(tile_idx + k), hi = *reinterpret_cast<const int4 *>(tile_idx + k + 4);
            const int e[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            bool any = false;
#pragma unroll
            for (int u = 0; u < 8; ++u) any |= e[u] == key;
            if (!any) continue;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (e[u] == key) {
                    const T w = tile_v[(k + u) * 4 + 0];
#pragma unroll
                    for (int d = 0; d < 3; ++d) acc[d] += w * (x[d] - tile_v[(k + u) * 4 + 1 + d]);
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int d = 0; d < 3; ++d) grecon[row * 3 + d] = acc[d];
    }
}

// sizes shared by the two entries: -> 0, or bad_arg.  Every element count an int could index stays below 2^31.
int orbit_sizes(const char *what, int g, int s, int a, int m, int n) {
    char buf[256];
    if (a < 1 || m < 1 || n < 1 || s < 1) {
        snprintf(buf, sizeof(buf), "%s: a, m, n and s must be positive (a %d, m %d, n %d, s %d)", what, a, m, n, s);
        return eap::bad_arg(buf);
    }
    if (g % s != 0) {
        snprintf(buf, sizeof(buf), "%s: g = %d groups are not b clouds x s = %d slots", what, g, s);
        return eap::bad_arg(buf);
    }
    const long long limit = 1LL << 31;
    if ((long long)g * a * m * 3 >= limit || (long long)g * a * n >= limit || (long long)(g / s) * 3 * n >= limit) {
        snprintf(buf, sizeof(buf), "%s: g %d, a %d, m %d, n %d: recon [g,a,m,3], the [g,a,n] maps and ori [g/s,3,n] must each hold fewer than 2^31 elements",
                 what, g, a, m, n);
        return eap::bad_arg(buf);
    }
    return 0;
}

template <typename T>
int orbit_fwd(int g, int s, int a, int m, int n, const T *recon, const T *ori, const uint8_t *member, T *r2o_all, int32_t *r2o_all_idx,
              T *r2o_in, int32_t *r2o_in_idx, T *o2r_all, int32_t *o2r_idx, T *o2r_in, hipStream_t st) {
    const char *what = "orbit_chamfer_forward";
    if (g <= 0) return 0;
    if (int e = orbit_sizes(what, g, s, a, m, n)) return e;
    if (!recon || !ori || !r2o_all || !r2o_all_idx || !o2r_all || !o2r_idx) return eap::bad_arg("orbit_chamfer_forward: null recon, ori or unmasked output");
    if (member && (!r2o_in || !r2o_in_idx || !o2r_in)) return eap::bad_arg("orbit_chamfer_forward: member given without the masked outputs");
    const int q = a * m;
    const dim3 block(OC_THREADS);
    if (member) {
        if (int e = eap::run_kernel(what, orbit_recon_to_ori_kernel<T, true>, eap::cdiv(q, OC_THREADS), g, 1, block, 0, st, q, n, s, recon, ori, member,
                                    r2o_all, r2o_all_idx, r2o_in, r2o_in_idx)) return e;
        return eap::run_kernel(what, orbit_ori_to_recon_kernel<T, true>, eap::cdiv(n, OC_THREADS), a, g, block, 0, st, m, n, s, recon, ori, member, o2r_all,
                               o2r_idx, o2r_in);
    }
    if (int e = eap::run_kernel(what, orbit_recon_to_ori_kernel<T, false>, eap::cdiv(q, OC_THREADS), g, 1, block, 0, st, q, n, s, recon, ori, member,
                                r2o_all, r2o_all_idx, (T *)nullptr, (int32_t *)nullptr)) return e;
    return eap::run_kernel(what, orbit_ori_to_recon_kernel<T, false>, eap::cdiv(n, OC_THREADS), a, g, block, 0, st, m, n, s, recon, ori, member, o2r_all,
                           o2r_idx, (T *)nullptr);
}

template <typename T>
int orbit_bwd(int g, int s, int a, int m, int n, const T *recon, const T *ori, const uint8_t *member, const int32_t *r2o_all_idx,
              const int32_t *r2o_in_idx, const int32_t *o2r_idx, const T *g_r2o_all, const T *g_r2o_in, const T *g_o2r_all, const T *g_o2r_in,
              T *grecon, hipStream_t st) {
    const char *what = "orbit_chamfer_backward";
    if (g <= 0) return 0;
    if (int e = orbit_sizes(what, g, s, a, m, n)) return e;
    if (!recon || !ori || !r2o_all_idx || !o2r_idx || !g_r2o_all || !g_o2r_all || !grecon)
        return eap::bad_arg("orbit_chamfer_backward: null recon, ori, unmasked index, unmasked gradient or output");
    if (member && (!r2o_in_idx || !g_r2o_in || !g_o2r_in)) return eap::bad_arg("orbit_chamfer_backward: member given without the masked index and gradients");
    const dim3 block(OC_THREADS);
    if (member)
        return eap::run_kernel(what, orbit_grad_ordered_kernel<T, true>, eap::cdiv(m, OC_THREADS), a, g, block, 0, st, m, n, s, recon, ori, member,
                               r2o_all_idx, r2o_in_idx, o2r_idx, g_r2o_all, g_r2o_in, g_o2r_all, g_o2r_in, grecon);
    return eap::run_kernel(what, orbit_grad_ordered_kernel<T, false>, eap::cdiv(m, OC_THREADS), a, g, block, 0, st, m, n, s, recon, ori, member,
                           r2o_all_idx, (const int32_t *)nullptr, o2r_idx, g_r2o_all, (const T *)nullptr, g_o2r_all, (const T *)nullptr, grecon);
}

}  // namespace

extern "C" int eap_orbit_chamfer_fwd_f32(int g, int s, int a, int m, int n, const float *recon, const float *ori, const uint8_t *member,
                                         float *r2o_all, int32_t *r2o_all_idx, float *r2o_in, int32_t *r2o_in_idx, float *o2r_all,
                                         int32_t *o2r_idx, float *o2r_in, eap_stream_t stream) {
    return orbit_fwd<float>(g, s, a, m, n, recon, ori, member, r2o_all, r2o_all_idx, r2o_in, r2o_in_idx, o2r_all, o2r_idx, o2r_in, eap::S(stream));
}

extern "C" int eap_orbit_chamfer_fwd_f64(int g, int s, int a, int m, int n, const double *recon, const double *ori, const uint8_t *member,
                                         double *r2o_all, int32_t *r2o_all_idx, double *r2o_in, int32_t *r2o_in_idx, double *o2r_all,
                                         int32_t *o2r_idx, double *o2r_in, eap_stream_t stream) {
    return orbit_fwd<double>(g, s, a, m, n, recon, ori, member, r2o_all, r2o_all_idx, r2o_in, r2o_in_idx, o2r_all, o2r_idx, o2r_in, eap::S(stream));
}

extern "C" int eap_orbit_chamfer_bwd_f32(int g, int s, int a, int m, int n, const float *recon, const float *ori, const uint8_t *member,
                                         const int32_t *r2o_all_idx, const int32_t *r2o_in_idx, const int32_t *o2r_idx, const float *g_r2o_all,
                                         const float *g_r2o_in, const float *g_o2r_all, const float *g_o2r_in, float *grecon,
                                         eap_stream_t stream) {
    return orbit_bwd<float>(g, s, a, m, n, recon, ori, member, r2o_all_idx, r2o_in_idx, o2r_idx, g_r2o_all, g_r2o_in, g_o2r_all, g_o2r_in, grecon,
                            eap::S(stream));
}

extern "C" int eap_orbit_chamfer_bwd_f64(int g, int s, int a, int m, int n, const double *recon, const double *ori, const uint8_t *member,
                                         const int32_t *r2o_all_idx, const int32_t *r2o_in_idx, const int32_t *o2r_idx, const double *g_r2o_all,
                                         const double *g_r2o_in, const double *g_o2r_all, const double *g_o2r_in, double *grecon,
                                         eap_stream_t stream) {
    return orbit_bwd<double>(g, s, a, m, n, recon, ori, member, r2o_all_idx, r2o_in_idx, o2r_idx, g_r2o_all, g_r2o_in, g_o2r_all, g_o2r_in, grecon,
                             eap::S(stream));
}
