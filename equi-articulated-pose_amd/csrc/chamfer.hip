// csrc/chamfer.hip -- chamfer distance forward / backward on gfx950, float32 and float64
// (reference: extensions/chamfer_dist/chamfer.cu L15-145 forward, L173-231 backward;
//  bound as chamfer.forward / chamfer.backward in chamfer_cuda.cpp L22-39).
//
//   forward : dist1[b,i] = min_j |xyz1[b,i] - xyz2[b,j]|^2, idx1 = first arg-min; same with the
//             clouds swapped for dist2 / idx2.
//   backward: gxyz1[b,i] += 2 g1 (x1 - x2[idx1]);  gxyz2[b,idx1] -= the same; and symmetrically.
//
// One lane per query point, the other cloud streams through LDS in 1024-point tiles (every
// candidate is a wave-wide broadcast read).  Squared distances are evaluated with one rounding
// per operation in the reference's source order, so distances and arg-min indices are bit-exact
// against the CPU oracle (first minimum wins, like the reference's strict `<`).
//
// Two backwards.  The scatter (float32 only) is the reference's: float atomicAdd, so a point that several points of the other
// cloud pick gets its sum in an order that differs from run to run.  The ordered one (both widths) is a gather: one lane per
// point of the cloud whose gradient is written, the other cloud's (idx, 2 g, xyz) stream through LDS like the forward's
// candidates, and the lane adds the entries that name its point in ascending index order -- no atomics, every output element
// written once, the same bits every run and the bits of the serial CPU oracle.
#include "common.h"

namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_TILE = 1024;

// one rounding per operation at either width (the file is built with -ffp-contract=off; the intrinsics say so in the source)
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }

// (LDS: 12 KB of tile for float, 24 KB for double)
template <typename T>
__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_kernel(
    int n, int m, const T *__restrict__ xyz1, const T *__restrict__ xyz2,
    T *__restrict__ dist, int32_t *__restrict__ index) {
    __shared__ T tile[CH_TILE * 3];
    const int bi = blockIdx.y;
    const int i = blockIdx.x * CH_THREADS + threadIdx.x;
    const T *p1 = xyz1 + ((size_t)bi * n + min(i, n - 1)) * 3;
    const T x1 = p1[0], y1 = p1[1], z1 = p1[2];
    const T *c2 = xyz2 + (size_t)bi * m * 3;
    T best = 0;
    int besti = 0;
    for (int k0 = 0; k0 < m; k0 += CH_TILE) {
        const int len = min(CH_TILE, m - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < len * 3; t += CH_THREADS) tile[t] = c2[(size_t)k0 * 3 + t];
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const T dx = sub_rn(tile[k * 3 + 0], x1), dy = sub_rn(tile[k * 3 + 1], y1),
                    dz = sub_rn(tile[k * 3 + 2], z1);
            const T d = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
            if ((k0 + k) == 0 || d < best) { best = d; besti = k0 + k; }
        }
    }
    if (i < n) {
        dist[(size_t)bi * n + i] = best;
        index[(size_t)bi * n + i] = besti;
    }
}

__global__ void chamfer_grad_kernel(int n, int m, const float *__restrict__ xyz1,
                                    const float *__restrict__ xyz2, const float *__restrict__ grad_dist1,
                                    const int32_t *__restrict__ idx1, float *__restrict__ gxyz1,
                                    float *__restrict__ gxyz2) {
    const int bi = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o1 = ((size_t)bi * n + i) * 3;
    const int j2 = idx1[(size_t)bi * n + i];
    const size_t o2 = ((size_t)bi * m + j2) * 3;
    const float g = grad_dist1[(size_t)bi * n + i] * 2;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float v = g * (xyz1[o1 + d] - xyz2[o2 + d]);
        atomicAdd(gxyz1 + o1 + d, v);
        atomicAdd(gxyz2 + o2 + d, -v);
    }
}

// The ordered backward of ONE cloud ("mine": n points): lane i owns point i.
//   own term   v[d] = (g_mine[i] * 2) * (mine[i,d] - other[idx_mine[i],d])
//   entries    j ascending over the other cloud (m points) with idx_other[j] == i:  -((g_other[j] * 2) * (other[j,d] - mine[i,d]))
// OWN_FIRST: ((0 + v) + entries...) -- cloud 1; else ((0 + entries...) + v) -- cloud 2: the order in which the serial oracle
// accumulates (direction 1 over all points, then direction 2).  An index outside its range names no point: it is neither
// matched nor dereferenced.  (LDS per 1024-entry tile: 4 KB of indices + 16 KB of (2 g, xyz) for float, 32 KB for double.)
template <typename T, bool OWN_FIRST>
__global__ __launch_bounds__(CH_THREADS) void chamfer_grad_ordered_kernel(
    int n, int m, const T *__restrict__ mine, const T *__restrict__ other, const int32_t *__restrict__ idx_mine,
    const T *__restrict__ g_mine, const int32_t *__restrict__ idx_other, const T *__restrict__ g_other,
    T *__restrict__ gmine) {
    __shared__ __align__(16) int32_t tile_idx[CH_TILE];
    __shared__ __align__(16) T tile_v[CH_TILE * 4];                 // (2 g, x, y, z) per entry
    const int bi = blockIdx.y;
    const int i = blockIdx.x * CH_THREADS + threadIdx.x;
    const bool live = i < n;
    const size_t row = (size_t)bi * n + (live ? i : n - 1);
    const T x[3] = {mine[row * 3 + 0], mine[row * 3 + 1], mine[row * 3 + 2]};
    T own[3] = {0, 0, 0};
    const int j2 = idx_mine[row];
    if (j2 >= 0 && j2 < m) {
        const T g = g_mine[row] * 2;
        const T *p2 = other + ((size_t)bi * m + j2) * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) own[d] = g * (x[d] - p2[d]);
    }
    T acc[3] = {0, 0, 0};
    if (OWN_FIRST) {
#pragma unroll
        for (int d = 0; d < 3; ++d) acc[d] += own[d];
    }
    const int key = live ? i : -1;                    // (a lane past the end matches nothing: it only helps to load the tiles)
    const size_t o0 = (size_t)bi * m;
    for (int k0 = 0; k0 < m; k0 += CH_TILE) {
        const int len = min(CH_TILE, m - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < CH_TILE; t += CH_THREADS) {
            if (t >= len) { tile_idx[t] = -2; continue; }           // (the walk below reads whole groups of 8)
            const size_t j = o0 + k0 + t;
            const int32_t to = idx_other[j];
            tile_idx[t] = (to >= 0 && to < n) ? to : -2;
            tile_v[t * 4 + 0] = g_other[j] * 2;
            tile_v[t * 4 + 1] = other[j * 3 + 0];
            tile_v[t * 4 + 2] = other[j * 3 + 1];
            tile_v[t * 4 + 3] = other[j * 3 + 2];
        }
        __syncthreads();
        // 8 indices per step (two 16-byte broadcast reads); the entries are only visited, in ascending order, where a lane of the wave has a
        // match among them -- with clouds of similar size that is about one step in eight
        for (int k = 0; k < len; k += 8) {
            const int4 a = *reinterpret_cast<const int4 *>(tile_idx + k), c = *reinterpret_cast<const int4 *>(tile_idx + k + 4);
            const int e[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
            bool any = false;
#pragma unroll
            for (int u = 0; u < 8; ++u) any |= e[u] == key;
            if (!any) continue;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (e[u] == key) {
                    const T g = tile_v[(k + u) * 4 + 0];
#pragma unroll
                    for (int d = 0; d < 3; ++d) acc[d] += -(g * (tile_v[(k + u) * 4 + 1 + d] - x[d]));
                }
            }
        }
    }
    if (!OWN_FIRST) {
#pragma unroll
        for (int d = 0; d < 3; ++d) acc[d] += own[d];
    }
    if (live) {
#pragma unroll
        for (int d = 0; d < 3; ++d) gmine[row * 3 + d] = acc[d];
    }
}

template <typename T>
int chamfer_fwd(int b, int n, int m, const T *xyz1, const T *xyz2, T *dist1, T *dist2, int32_t *idx1, int32_t *idx2, hipStream_t s) {
    if (b <= 0) return 0;
    if (n <= 0 || m <= 0) return eap::bad_arg("chamfer_forward: empty cloud");
    if (int e = eap::run_kernel("chamfer_forward", chamfer_nn_kernel<T>, eap::cdiv(n, CH_THREADS), b, 1, dim3(CH_THREADS), 0, s, n, m, xyz1, xyz2, dist1, idx1)) return e;
    return eap::run_kernel("chamfer_forward", chamfer_nn_kernel<T>, eap::cdiv(m, CH_THREADS), b, 1, dim3(CH_THREADS), 0, s, m, n, xyz2, xyz1, dist2, idx2);
}

template <typename T>
int chamfer_bwd_ordered(int b, int n, int m, const T *xyz1, const T *xyz2, const int32_t *idx1, const int32_t *idx2, const T *g1,
                        const T *g2, T *gxyz1, T *gxyz2, hipStream_t s) {
    if (b <= 0) return 0;
    if (n <= 0 || m <= 0) return eap::bad_arg("chamfer_backward_ordered: empty cloud");
    if (int e = eap::run_kernel("chamfer_backward_ordered", chamfer_grad_ordered_kernel<T, true>, eap::cdiv(n, CH_THREADS), b, 1, dim3(CH_THREADS), 0, s,
                                n, m, xyz1, xyz2, idx1, g1, idx2, g2, gxyz1)) return e;
    return eap::run_kernel("chamfer_backward_ordered", chamfer_grad_ordered_kernel<T, false>, eap::cdiv(m, CH_THREADS), b, 1, dim3(CH_THREADS), 0, s,
                           m, n, xyz2, xyz1, idx2, g2, idx1, g1, gxyz2);
}

}  // namespace

extern "C" int eap_chamfer_fwd_f32(int b, int n, int m, const float *xyz1, const float *xyz2,
                                   float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                                   eap_stream_t stream) {
    return chamfer_fwd<float>(b, n, m, xyz1, xyz2, dist1, dist2, idx1, idx2, eap::S(stream));
}

extern "C" int eap_chamfer_fwd_f64(int b, int n, int m, const double *xyz1, const double *xyz2,
                                   double *dist1, double *dist2, int32_t *idx1, int32_t *idx2,
                                   eap_stream_t stream) {
    return chamfer_fwd<double>(b, n, m, xyz1, xyz2, dist1, dist2, idx1, idx2, eap::S(stream));
}

extern "C" int eap_chamfer_bwd_f32(int b, int n, int m, const float *xyz1, const float *xyz2,
                                   const int32_t *idx1, const int32_t *idx2, const float *g1,
                                   const float *g2, float *gxyz1, float *gxyz2, eap_stream_t stream) {
    if (b <= 0) return 0;
    hipStream_t s = eap::S(stream);
    int e = eap::hip_fail(hipMemsetAsync(gxyz1, 0, sizeof(float) * (size_t)b * n * 3, s), "chamfer_backward memset");
    if (!e) e = eap::hip_fail(hipMemsetAsync(gxyz2, 0, sizeof(float) * (size_t)b * m * 3, s), "chamfer_backward memset");
    if (e || n <= 0 || m <= 0) return e;
    if ((e = eap::run_kernel("chamfer_backward", chamfer_grad_kernel, eap::cdiv(n, 256), b, 1, dim3(256), 0, s, n, m, xyz1, xyz2, g1, idx1, gxyz1, gxyz2))) return e;
    return eap::run_kernel("chamfer_backward", chamfer_grad_kernel, eap::cdiv(m, 256), b, 1, dim3(256), 0, s, m, n, xyz2, xyz1, g2, idx2, gxyz2, gxyz1);
}

extern "C" int eap_chamfer_bwd_ordered_f32(int b, int n, int m, const float *xyz1, const float *xyz2,
                                           const int32_t *idx1, const int32_t *idx2, const float *g1,
                                           const float *g2, float *gxyz1, float *gxyz2, eap_stream_t stream) {
    return chamfer_bwd_ordered<float>(b, n, m, xyz1, xyz2, idx1, idx2, g1, g2, gxyz1, gxyz2, eap::S(stream));
}

extern "C" int eap_chamfer_bwd_ordered_f64(int b, int n, int m, const double *xyz1, const double *xyz2,
                                           const int32_t *idx1, const int32_t *idx2, const double *g1,
                                           const double *g2, double *gxyz1, double *gxyz2, eap_stream_t stream) {
    return chamfer_bwd_ordered<double>(b, n, m, xyz1, xyz2, idx1, idx2, g1, g2, gxyz1, gxyz2, eap::S(stream));
}
