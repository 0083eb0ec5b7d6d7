// csrc/grouping.hip -- neighbour search for the SO(3) point convolution on gfx950.
//
// Replaces the reference's grouping extension (vgtk/vgtk/cuda/grouping_cuda.cpp L71-86,
// kernels grouping_cuda_kernel.cu L68-113).  The reference runs ONE block per cloud with a
// thread striding over the queries; here every query point gets a group of 16 lanes, the support
// cloud streams through LDS in tiles (a group tests 16 consecutive support points per step) and a
// block retires as soon as all of its 32 queries have found `nsample` neighbours -- with the
// large radii of the deeper layers (first-nsample-in-index-order semantics) that is after the
// first tile.
//
// Bit-exactness: d2 is evaluated as ((dx*dx + dy*dy) + dz*dz) with one rounding per operation
// (mul_rn/add_rn below never contract to FMA), the same order as grouping_cuda_kernel.cu:L93-94
// and as the CPU oracle; the neighbour lists are therefore identical integer-for-integer.  Every
// kernel here is one template over the scalar type (float, double), as the reference dispatches
// these ops with AT_DISPATCH_FLOATING_TYPES.
#include "common.h"

namespace {

constexpr int BQ_LANES = 16;                           // lanes that share one query point's scan
constexpr int BQ_THREADS = 512;
constexpr int BQ_QUERIES = BQ_THREADS / BQ_LANES;       // query points per block
constexpr int BQ_TILE = 1024;

// One rounding per operation in the operands' own type, never contracted (this file is built with -ffp-contract=off):
// the float and the double form of every chain below run the same operations in the same order.
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float sqrt_t(float a) { return sqrtf(a); }
__device__ __forceinline__ double sqrt_t(double a) { return sqrt(a); }
__device__ __forceinline__ float acos_t(float a) { return acosf(a); }
__device__ __forceinline__ double acos_t(double a) { return acos(a); }
__device__ __forceinline__ float min_t(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double min_t(double a, double b) { return fmin(a, b); }

// (x*x + y*y) + z*z
template <typename T>
__device__ __forceinline__ T sq3(T x, T y, T z) {
    return add_rn(add_rn(mul_rn(x, x), mul_rn(y, y)), mul_rn(z, z));
}
template <typename T>
__device__ __forceinline__ T d2_exact(T ax, T ay, T az, T bx, T by, T bz) {
    return sq3(sub_rn(ax, bx), sub_rn(ay, by), sub_rn(az, bz));
}

// A query point is scanned by a group of BQ_LANES consecutive lanes: lane l of the group tests candidate t0 + l, the
// group's slice of the wave's ballot ranks the hits (lower candidate = lower slot: ascending index order, as the serial scan)
// and the hits of one point land in its one row of idx.  The four groups of a wave walk the tile in step (one LDS address
// per candidate, broadcast to the groups), a wave leaves a tile when its four lists are full, a block the cloud when all are.
// With the first layer's small radius a list never fills and the scan is the whole cloud: 4096 / BQ_LANES steps per lane
// instead of 4096, on BQ_LANES times as many waves.
template <typename T>
__global__ __launch_bounds__(BQ_THREADS) void ball_query_kernel(
    int n, int m, T radius2, int nsample, const T *__restrict__ new_xyz,
    const T *__restrict__ xyz, int32_t *__restrict__ idx) {
    __shared__ T tile[3][BQ_TILE];
    const int bi = blockIdx.y;
    xyz += (size_t)bi * 3 * n;
    new_xyz += (size_t)bi * 3 * m;
    idx += (size_t)bi * m * nsample;

    const int lane = threadIdx.x & 63, gl = lane & (BQ_LANES - 1), gsh = lane & ~(BQ_LANES - 1);
    const int j = blockIdx.x * BQ_QUERIES + threadIdx.x / BQ_LANES;
    const bool live = j < m;
    T qx = 0, qy = 0, qz = 0;
    if (live) { qx = new_xyz[j]; qy = new_xyz[m + j]; qz = new_xyz[2 * m + j]; }
    int32_t *out = idx + (size_t)(live ? j : 0) * nsample;

    int cnt = live ? 0 : nsample;          // the same in every lane of a group
    for (int k0 = 0; k0 < n; k0 += BQ_TILE) {
        const int len = min(BQ_TILE, n - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < len; t += BQ_THREADS) {
            tile[0][t] = xyz[k0 + t];
            tile[1][t] = xyz[n + k0 + t];
            tile[2][t] = xyz[2 * n + k0 + t];
        }
        __syncthreads();
        for (int t0 = 0; t0 < len; t0 += BQ_LANES) {             // wave-uniform trip count
            if (__ballot(cnt < nsample) == 0ull) break;
            const int t = min(t0 + gl, len - 1);
            const T d2 = d2_exact(qx, qy, qz, tile[0][t], tile[1][t], tile[2][t]);
            const bool hit = t0 + gl < len && cnt < nsample && d2 < radius2;
            const unsigned mine = (unsigned)(__ballot(hit) >> gsh) & ((1u << BQ_LANES) - 1u);
            const int slot = cnt + __popc(mine & ((1u << gl) - 1u));
            if (hit && slot < nsample) out[slot] = k0 + t;
            cnt = min(nsample, cnt + __popc(mine));
        }
        if (__syncthreads_and(cnt >= nsample)) break;
    }
    // grouping_cuda_kernel.cu:L100-105: cyclic repeat-padding only when cnt < nsample-1; with
    // exactly nsample-1 hits the last slot keeps the host wrapper's zero initialisation.
    // The repeats read back what other lanes of the group stored: out[t] = out[t - cnt] = ... = out[t % cnt].
    __threadfence_block();
    __syncthreads();
    if (!live) return;
    if (cnt < nsample - 1) {
        if (cnt == 0) {
            for (int t = gl; t < nsample; t += BQ_LANES) out[t] = 0;
        } else {
            for (int t = cnt + gl; t < nsample; t += BQ_LANES) out[t] = out[t % cnt];
        }
    } else if (cnt == nsample - 1) {
        if (gl == 0) out[nsample - 1] = 0;
    }
}

template <typename T>
int launch_ball_query(int b, int n, int m, float radius, int nsample, const T *new_xyz,
                      const T *xyz, int32_t *idx, hipStream_t s) {
    if (b <= 0 || m <= 0 || nsample <= 0) return 0;
    if (n <= 0) return eap::bad_arg("ball_query: empty support cloud");
    const T r2 = (T)(radius * radius);  // float product first, grouping_cuda_kernel.cu:L82
    return eap::run_kernel("ball_query", ball_query_kernel<T>, eap::cdiv(m, BQ_QUERIES), b, 1, dim3(BQ_THREADS), 0, s, n, m, r2, nsample, new_xyz, xyz, idx);
}


// ---------------------------------------------------------------------------------------------
// furthest point sampling (grouping_cuda.cpp:L160-174, kernel grouping_cuda_kernel.cu:L352-466).
// Inherently sequential in m; one block per cloud.  Off the shipped models' path (stride is 1),
// kept for API completeness.  The winner of each round must match the reference exactly, ties
// included: per-thread first strict maximum over k = tid, tid+nt, ..., then a halving tree that
// keeps the lower slot on ties -- the same reduction shape, with nt = the reference's block size
// (largest power of two <= n, capped at 1024).  temp, the shared distances and the constants are of the
// cloud's own type (float: 8 KB of LDS, double: 12 KB).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void fps_kernel(int n, int m, const T *__restrict__ xyz,
                                                  T *__restrict__ temp, int32_t *__restrict__ idx) {
    __shared__ T s_d[1024];
    __shared__ int s_i[1024];
    const int bi = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    xyz += (size_t)bi * 3 * n;
    temp += (size_t)bi * n;
    idx += (size_t)bi * m;
    for (int k = tid; k < n; k += nt) temp[k] = (T)1e10;
    int old = 0;
    if (tid == 0) idx[0] = 0;
    __syncthreads();
    for (int j = 1; j < m; ++j) {
        const T x1 = xyz[old], y1 = xyz[n + old], z1 = xyz[2 * n + old];
        T best = (T)-1;
        int besti = 0;
        for (int k = tid; k < n; k += nt) {
            const T x2 = xyz[k], y2 = xyz[n + k], z2 = xyz[2 * n + k];
            const T mag = sq3(x2, y2, z2);
            if (mag <= (T)1e-3) continue;
            const T d = d2_exact(x2, y2, z2, x1, y1, z1);
            const T d2 = min_t(d, temp[k]);
            temp[k] = d2;
            if (d2 > best) { best = d2; besti = k; }
        }
        s_d[tid] = best;
        s_i[tid] = besti;
        __syncthreads();
        for (int s = nt >> 1; s >= 1; s >>= 1) {
            if (tid < s && s_d[tid + s] > s_d[tid]) { s_d[tid] = s_d[tid + s]; s_i[tid] = s_i[tid + s]; }
            __syncthreads();
        }
        old = s_i[0];
        if (tid == 0) idx[j] = old;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// anchor_query, S^2 variant (grouping_cuda.cpp:L88-108, kernel .cu:L181-247):
//   w[b,p,a,k,n] = (kw - |x|)^2 + ((kh - theta) |x|)^2,  theta = acos(x . anchor_a / |x|)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void anchor_query_kernel(int np, int nn, int na, int ks, const T *__restrict__ gxyz,
                                    const T *__restrict__ anchors, const T *__restrict__ kpts,
                                    T *__restrict__ w) {
    const int bi = blockIdx.y;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)np * nn) return;
    const int pi = (int)(e / nn), ni = (int)(e % nn);
    const T *g = gxyz + (size_t)bi * 3 * np * nn;
    const T x = g[e], y = g[(size_t)np * nn + e], z = g[(size_t)2 * np * nn + e];
    const T norm = add_rn(sqrt_t(sq3(x, y, z)), (T)1e-6);
    T *wp = w + (((size_t)bi * np + pi) * na) * ks * nn + ni;
    for (int ai = 0; ai < na; ++ai) {
        const T dot = add_rn(add_rn(mul_rn(x, anchors[ai * 3]), mul_rn(y, anchors[ai * 3 + 1])),
                             mul_rn(z, anchors[ai * 3 + 2]));
        const T theta = acos_t(div_rn(dot, norm));
        for (int ki = 0; ki < ks; ++ki) {
            const T a = sub_rn(kpts[ki * 2], norm);
            const T c = mul_rn(sub_rn(kpts[ki * 2 + 1], theta), norm);
            wp[((size_t)ai * ks + ki) * nn] = add_rn(mul_rn(a, a), mul_rn(c, c));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// initial_anchor_query (grouping_cuda.cpp:L138-158, kernel .cu:L117-167): kernel-point occupancy
// of a fragment around each centre.  The reference scatters with two atomicAdds per hit; here
// every output element (kernel point, centre, anchor) owns a lane that sums over the fragment
// points in index order -- deterministic, no atomics.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void initial_anchor_query_kernel(int nc, int m, int na, int ks, T radius, T sigma,
                                            const T *__restrict__ centers, const T *__restrict__ xyz,
                                            const T *__restrict__ kpts, T *__restrict__ w,
                                            T *__restrict__ cnt) {
    const int pn = blockIdx.x, bi = blockIdx.y;
    const T *C = centers + (size_t)bi * 3 * nc;
    const T cx = C[pn], cy = C[nc + pn], cz = C[2 * nc + pn];
    for (int e = threadIdx.x; e < ks * na; e += blockDim.x) {
        const int kn = e / na, an = e - kn * na;
        const T kx = add_rn(kpts[e * 3], cx), ky = add_rn(kpts[e * 3 + 1], cy), kz = add_rn(kpts[e * 3 + 2], cz);
        T sw = (T)0, sc = (T)0;
        for (int pm = 0; pm < m; ++pm) {
            const T x = xyz[3 * pm], y = xyz[3 * pm + 1], z = xyz[3 * pm + 2];
            const T dc = sqrt_t(d2_exact(cx, cy, cz, x, y, z));
            if (dc <= radius) {
                const T dk = sqrt_t(d2_exact(kx, ky, kz, x, y, z));
                const T wt = sub_rn((T)1, div_rn(mul_rn(dk, dk), sigma));
                if (wt > (T)0) sw = add_rn(sw, wt);
                sc = add_rn(sc, (T)1);
            }
        }
        const size_t o = (((size_t)bi * ks + kn) * nc + pn) * na + an;
        w[o] = sw;
        cnt[o] = sc;
    }
}

template <typename T>
int launch_fps(int b, int n, int m, const T *xyz, T *temp, int32_t *idx, hipStream_t s) {
    if (b <= 0 || m <= 0) return 0;
    if (n <= 0) return eap::bad_arg("furthest_point_sampling: empty cloud");
    int threads = 1;
    while (threads * 2 <= n && threads < 1024) threads *= 2;   // opt_n_threads, grouping_cuda_kernel.cu:L29-33
    return eap::run_kernel("furthest_point_sampling", fps_kernel<T>, b, 1, 1, dim3(threads), 0, s, n, m, xyz, temp, idx);
}

template <typename T>
int launch_anchor_query(int b, int np, int nn, int na, int ks, const T *grouped_xyz, const T *anchors,
                        const T *kernel_pts, T *w, hipStream_t s) {
    if (b <= 0 || np <= 0 || nn <= 0) return 0;
    return eap::run_kernel("anchor_query", anchor_query_kernel<T>, eap::cdiv((long long)np * nn, 256), b, 1, dim3(256), 0, s, np, nn, na, ks, grouped_xyz,
                           anchors, kernel_pts, w);
}

template <typename T>
int launch_initial_anchor_query(int b, int nc, int m, int na, int ks, float radius, float sigma, const T *centers,
                                const T *xyz, const T *kernel_pts, T *w, T *cnt, hipStream_t s) {
    if (b <= 0 || nc <= 0 || na <= 0 || ks <= 0) return 0;
    // radius and sigma arrive as float (grouping_cuda.cpp:L138) and are widened once, where the kernel compares and divides in T
    return eap::run_kernel("initial_anchor_query", initial_anchor_query_kernel<T>, nc, b, 1, dim3(256), 0, s, nc, m, na, ks, (T)radius, (T)sigma, centers,
                           xyz, kernel_pts, w, cnt);
}

}  // namespace

extern "C" int eap_ball_query_f32(int b, int n, int m, float radius, int nsample,
                                  const float *new_xyz, const float *xyz, int32_t *idx,
                                  eap_stream_t stream) {
    return launch_ball_query<float>(b, n, m, radius, nsample, new_xyz, xyz, idx, eap::S(stream));
}
extern "C" int eap_ball_query_f64(int b, int n, int m, float radius, int nsample,
                                  const double *new_xyz, const double *xyz, int32_t *idx,
                                  eap_stream_t stream) {
    return launch_ball_query<double>(b, n, m, radius, nsample, new_xyz, xyz, idx, eap::S(stream));
}

extern "C" int eap_furthest_point_sampling_f32(int b, int n, int m, const float *xyz, float *temp,
                                               int32_t *idx, eap_stream_t stream) {
    return launch_fps<float>(b, n, m, xyz, temp, idx, eap::S(stream));
}
extern "C" int eap_furthest_point_sampling_f64(int b, int n, int m, const double *xyz, double *temp,
                                               int32_t *idx, eap_stream_t stream) {
    return launch_fps<double>(b, n, m, xyz, temp, idx, eap::S(stream));
}

extern "C" int eap_anchor_query_f32(int b, int np, int nn, int na, int ks, const float *grouped_xyz,
                                    const float *anchors, const float *kernel_pts, float *w,
                                    eap_stream_t stream) {
    return launch_anchor_query<float>(b, np, nn, na, ks, grouped_xyz, anchors, kernel_pts, w, eap::S(stream));
}
extern "C" int eap_anchor_query_f64(int b, int np, int nn, int na, int ks, const double *grouped_xyz,
                                    const double *anchors, const double *kernel_pts, double *w,
                                    eap_stream_t stream) {
    return launch_anchor_query<double>(b, np, nn, na, ks, grouped_xyz, anchors, kernel_pts, w, eap::S(stream));
}

extern "C" int eap_initial_anchor_query_f32(int b, int nc, int m, int na, int ks, float radius, float sigma,
                                            const float *centers, const float *xyz, const float *kernel_pts,
                                            float *w, float *cnt, eap_stream_t stream) {
    return launch_initial_anchor_query<float>(b, nc, m, na, ks, radius, sigma, centers, xyz, kernel_pts, w, cnt, eap::S(stream));
}
extern "C" int eap_initial_anchor_query_f64(int b, int nc, int m, int na, int ks, float radius, float sigma,
                                            const double *centers, const double *xyz, const double *kernel_pts,
                                            double *w, double *cnt, eap_stream_t stream) {
    return launch_initial_anchor_query<double>(b, nc, m, na, ks, radius, sigma, centers, xyz, kernel_pts, w, cnt, eap::S(stream));
}
