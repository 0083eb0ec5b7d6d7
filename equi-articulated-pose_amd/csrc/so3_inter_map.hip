// csrc/so3_inter_map.hip -- the fused grouping of the pose-aware inter conv and its transpose THROUGH A PER-ENTRY ANCHOR MAP
// (csrc/so3_anchor_map.hip): anchor sets that are not a group, where the reference's anchor index
// (vgtk/vgtk/so3conv/functional.py:L1199-1204) is no table lookup and no permutation.
//
//   forward    X[b,c,k,p,a]   = sum_n w(p,a,k,n) F[b,c,idx_n,amap[b,p,n,a]]                           (functional.py:L1221-1261)
//   backward   dF[b,c,q,a']   = sum_{(p,n): idx = q} sum_{a: amap(a) = a'} sum_k w(p,a,k,n) dX[b,c,k,p,a]
//
// Both kernels: block = one point at a time, lane = (channel group, anchor) -- 64 / na channel groups share a wave, so 60 of
// 64 lanes work at 20 anchors -- and the weights w = relu(1 - |g - A_a kappa_k|^2 / sigma) are evaluated in registers from gx
// and rk exactly as csrc/so3_inter.hip does.
//
// The map is many-to-one in q AND in a, so the backward accumulates where the slab kernel of csrc/so3_inter_bwd.hip permutes:
// a wave parks its per-anchor sums in LDS and every target lane a' adds the ones whose map byte equals a', in anchor order.
// No float atomics: as there, every block (cloud x channel chunk x contiguous range of points) owns a private slab
// [q][channel][a'] and updates it with load-add-store; a slab word is only ever touched by ONE lane, in program order (so a
// list that names a row twice is summed in list order; the slab words of eight entries are requested together unless two of them
// name the same row -- the slab kernel's ordered slow path), and a second kernel adds the slabs of the point ranges in range
// order.  Bit-identical run to run.
#include "common.h"
#include "device_prims.h"

namespace {

constexpr int T_ = 256;     // 4 waves
constexpr int NW = 4;
constexpr int BCW = 2;      // backward: channels per lane
constexpr int NB = 8;       // backward: entries whose slab words are requested together

struct MapShared {
    float4 *g;       // [nn]
    int32_t *q;      // [nn]
    uint8_t *map;    // [nn][na]
};

__device__ __forceinline__ MapShared carve(unsigned char *base, int nn) {
    MapShared s;
    s.g = reinterpret_cast<float4 *>(base);
    s.q = reinterpret_cast<int32_t *>(base + 16 * (size_t)nn);
    s.map = base + 20 * (size_t)nn;
    return s;
}

__device__ __forceinline__ void load_point(const MapShared &s, size_t pn, int nn, int na, int n_sup, const int32_t *idx,
                                           const float4 *gx, const uint8_t *amap) {
    for (int i = threadIdx.x; i < nn; i += T_) {
        s.g[i] = gx[pn + i];
        const int q = idx[pn + i];
        s.q[i] = q < n_sup ? q : -1;   // shadow row (all zeros in the reference) -> skipped
    }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(amap + pn * na);      // na % 4 == 0: whole dwords
    uint32_t *dst = reinterpret_cast<uint32_t *>(s.map);
    for (int i = threadIdx.x; i < (nn * na) >> 2; i += T_) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------
// forward: the 4 waves split the kernel points, a lane keeps CC x KPW outputs of its (channel group, anchor)
// ---------------------------------------------------------------------------------------------
template <int KPW, int CC>
__global__ __launch_bounds__(T_) void so3_inter_group_fwd_map_kernel(
    int c, int p, int n_sup, int nn, int na, int ks, float inv_sigma, const float *__restrict__ feats,
    const int32_t *__restrict__ idx, const float4 *__restrict__ gx, const float *__restrict__ rk,
    const uint8_t *__restrict__ amap, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MapShared s = carve(smem, nn);
    const int pi = xcd_point(blockIdx.x, p), bi = blockIdx.y;
    load_point(s, ((size_t)bi * p + pi) * nn, nn, na, n_sup, idx, gx, amap);
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncg = 64 / na, cg = lane / na, a = lane - cg * na;
    const int k0 = wave * KPW;
    if (cg >= ncg || k0 >= ks) return;

    float kx[KPW], ky[KPW], kz[KPW];
#pragma unroll
    for (int kk = 0; kk < KPW; ++kk) {
        const float *r3 = rk + ((size_t)a * ks + min(k0 + kk, ks - 1)) * 3;
        kx[kk] = r3[0]; ky[kk] = r3[1]; kz[kk] = r3[2];
    }
    const float *fb = feats + (size_t)bi * c * n_sup * na;
    const size_t f_cs = (size_t)n_sup * na;
    float *ob = out + (size_t)bi * c * ks * p * na + (size_t)pi * na + a;
    const size_t o_ks = (size_t)p * na, o_cs = (size_t)ks * p * na;

    for (int c0 = cg; c0 < c; c0 += CC * ncg) {           // this lane's channels: c0 + cc * ncg
        float acc[CC][KPW];
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
#pragma unroll
            for (int kk = 0; kk < KPW; ++kk) acc[cc][kk] = 0.f;
        for (int n = 0; n < nn; ++n) {
            const int q = s.q[n];
            if (q < 0) continue;   // wave-uniform
            const float4 g = s.g[n];
            float wv[KPW];
#pragma unroll
            for (int kk = 0; kk < KPW; ++kk) {
                const float dx = g.x - kx[kk], dy = g.y - ky[kk], dz = g.z - kz[kk];
                wv[kk] = fmaxf(1.0f - (dx * dx + dy * dy + dz * dz) * inv_sigma, 0.0f);
            }
            const int a_src = min((int)s.map[n * na + a], na - 1);
            const float *f = fb + (size_t)q * na + a_src;
#pragma unroll
            for (int cc = 0; cc < CC; ++cc) {
                const float fv = (c0 + cc * ncg < c) ? f[(size_t)(c0 + cc * ncg) * f_cs] : 0.f;
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk) acc[cc][kk] = fmaf(fv, wv[kk], acc[cc][kk]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
            if (c0 + cc * ncg < c) {
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk)
                    if (k0 + kk < ks) ob[(size_t)(c0 + cc * ncg) * o_cs + (size_t)(k0 + kk) * o_ks] = acc[cc][kk];
            }
    }
}

template <int KPW>
int launch_fwd_map(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats, const int32_t *idx,
                   const float *gx, const float *rk, const uint8_t *amap, float *out, hipStream_t s) {
    const size_t shmem = 20 * (size_t)nn + (size_t)nn * na;
    const int ncg = 64 / na;
    auto kern = so3_inter_group_fwd_map_kernel<KPW, 1>;
    if (c > ncg) kern = c <= 4 * ncg ? so3_inter_group_fwd_map_kernel<KPW, 4> : so3_inter_group_fwd_map_kernel<KPW, 8>;
    return eap::run_kernel("so3_inter_group_fwd_map", kern, p, b, 1, dim3(T_), shmem, s, c, p, n, nn, na, ks, 1.0f / sigma, feats, idx,
                           reinterpret_cast<const float4 *>(gx), rk, amap, out);
}

// ---------------------------------------------------------------------------------------------
// backward: private slabs, see the header of this file
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ld_l2(const float *p) {
    // bypasses L1 (served by L2), so a lane always sees its own earlier (write-through) stores to the slab
    return __builtin_nontemporal_load(p);
}

template <int KS_MAX>
__global__ __launch_bounds__(T_) void so3_inter_group_bwd_map_kernel(
    int c, int p, int n_sup, int nn, int na, int ks, float inv_sigma, int nch, int ps, int ppb,
    const float *__restrict__ gout, const int32_t *__restrict__ idx, const float4 *__restrict__ gx,
    const float *__restrict__ rk, const uint8_t *__restrict__ amap, float *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_t = reinterpret_cast<float *>(smem);                                  // [NW][BCW][64] per-anchor sums of one entry
    const MapShared s = carve(smem + sizeof(float) * NW * BCW * 64, nn);
    int32_t *s_dup = reinterpret_cast<int32_t *>(s.map + (size_t)nn * na);        // [nn / NB + 1]: the group names a row twice
    const int ngroups = (nn + NB - 1) / NB;

    const int split = blockIdx.x, chunk = blockIdx.y, bi = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncg = 64 / na, cg = lane / na, a = lane - cg * na;
    const bool act = cg < ncg;
    const int cpw = ncg * BCW, ccb = NW * cpw;             // channels per wave / per block
    const int p_beg = split * ppb, p_end = min(p, p_beg + ppb);
    float *slab = ws + (((size_t)bi * nch + chunk) * ps + split) * ((size_t)n_sup * ccb * na);

    float kx[KS_MAX], ky[KS_MAX], kz[KS_MAX];
#pragma unroll
    for (int k = 0; k < KS_MAX; ++k) {
        const float *r3 = rk + ((size_t)min(a, na - 1) * ks + min(k, ks - 1)) * 3;
        kx[k] = r3[0]; ky[k] = r3[1]; kz[k] = r3[2];
    }
    int chl[BCW];                                           // this lane's channels within the block's chunk
    bool live[BCW];
#pragma unroll
    for (int cc = 0; cc < BCW; ++cc) {
        chl[cc] = wave * cpw + cc * ncg + min(cg, ncg - 1);
        live[cc] = act && chunk * ccb + chl[cc] < c;
    }
    const size_t o_ks = (size_t)p * na, o_cs = (size_t)ks * p * na;
    float *tb = s_t + wave * BCW * 64;

    for (int pi = p_beg; pi < p_end; ++pi) {
        __syncthreads();   // the previous point's reads of s.g / s.q / s.map are done
        load_point(s, ((size_t)bi * p + pi) * nn, nn, na, n_sup, idx, gx, amap);
        __syncthreads();
        // a group of NB entries whose rows are not pairwise distinct (repeat-padded lists) must not request its slab words up front
        for (int gi = threadIdx.x; gi < ngroups; gi += T_) {
            bool dup = false;
            for (int i = gi * NB; i < min(gi * NB + NB, nn); ++i)
                for (int j = gi * NB; j < i; ++j) dup |= s.q[i] >= 0 && s.q[i] == s.q[j];
            s_dup[gi] = dup ? 1 : 0;
        }
        float go[BCW][KS_MAX];
#pragma unroll
        for (int cc = 0; cc < BCW; ++cc) {
            const float *src = gout + (size_t)bi * c * o_cs + (size_t)min(chunk * ccb + chl[cc], c - 1) * o_cs + (size_t)pi * na + min(a, na - 1);
#pragma unroll
            for (int k = 0; k < KS_MAX; ++k) go[cc][k] = (live[cc] && k < ks) ? src[(size_t)min(k, ks - 1) * o_ks] : 0.f;
        }
        __syncthreads();
        for (int n0 = 0; n0 < nn; n0 += NB) {
            // ---- the slab words of the whole group requested up front: the L2 round trips overlap each other and the arithmetic
            const bool prefetch = s_dup[n0 / NB] == 0;
            float old[NB][BCW];
            if (prefetch) {
#pragma unroll
                for (int nl = 0; nl < NB; ++nl) {
                    const int q = max(s.q[min(n0 + nl, nn - 1)], 0);   // clamped; discarded if invalid
#pragma unroll
                    for (int cc = 0; cc < BCW; ++cc)
                        old[nl][cc] = live[cc] ? ld_l2(slab + ((size_t)q * ccb + chl[cc]) * na + a) : 0.f;
                }
            }
#pragma unroll
            for (int nl = 0; nl < NB; ++nl) {
                const int n = n0 + nl;
                const int q = n < nn ? s.q[n] : -1;
                if (q < 0) continue;   // block-uniform
                const float4 g = s.g[n];
                float t[BCW];
#pragma unroll
                for (int cc = 0; cc < BCW; ++cc) t[cc] = 0.f;
#pragma unroll
                for (int k = 0; k < KS_MAX; ++k) {
                    const float dx = g.x - kx[k], dy = g.y - ky[k], dz = g.z - kz[k];
                    const float wv = fmaxf(1.0f - (dx * dx + dy * dy + dz * dz) * inv_sigma, 0.0f);
#pragma unroll
                    for (int cc = 0; cc < BCW; ++cc) t[cc] = fmaf(wv, go[cc][k], t[cc]);
                }
                // out anchor a contributes to input anchor amap[n][a]: parked per (channel, anchor), then every target lane a'
                // adds the ones mapped onto it, in anchor order
#pragma unroll
                for (int cc = 0; cc < BCW; ++cc) tb[cc * 64 + lane] = t[cc];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                float sum[BCW];
#pragma unroll
                for (int cc = 0; cc < BCW; ++cc) sum[cc] = 0.f;
                const uint8_t *m = s.map + n * na;
                const float *tg = tb + min(cg, ncg - 1) * na;
                for (int a2 = 0; a2 < na; ++a2) {
                    const bool hit = (int)m[a2] == a;
#pragma unroll
                    for (int cc = 0; cc < BCW; ++cc) {
                        const float v = tg[cc * 64 + a2];
                        sum[cc] += hit ? v : 0.f;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int cc = 0; cc < BCW; ++cc)
                    if (live[cc]) {
                        float *word = slab + ((size_t)q * ccb + chl[cc]) * na + a;
                        *word = (prefetch ? old[nl][cc] : ld_l2(word)) + sum[cc];   // a row named twice: ordered slow path
                    }
            }
        }
    }
}

// gfeats[b,c,q,a] = sum over the point ranges, in range order, of slab[b,chunk,split][q][c % ccb][a]
__global__ void so3_inter_group_bwd_map_reduce_kernel(long long total, int c, int n_sup, int na, int nch, int ps, int ccb,
                                                      const float *__restrict__ ws, float *__restrict__ gfeats) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over (b,c,q,a)
    if (e >= total) return;
    const int a = (int)(e % na);
    long long r = e / na;
    const int q = (int)(r % n_sup); r /= n_sup;
    const int ci = (int)(r % c);
    const int bi = (int)(r / c);
    const int chunk = ci / ccb, cc = ci - chunk * ccb;
    const size_t slab_sz = (size_t)n_sup * ccb * na;
    const float *src = ws + ((size_t)bi * nch + chunk) * ps * slab_sz + ((size_t)q * ccb + cc) * na + a;
    float sum = 0.f;
    for (int z = 0; z < ps; ++z) sum += src[(size_t)z * slab_sz];
    gfeats[e] = sum;
}

// channel chunks, point ranges and points per range of the backward: at least one block per CU where the points allow,
// at least 16 points per block, at most 1 GiB of slabs where one range per chunk fits in it
void plan(int b, int c, int p, int n, int na, int *ccb, int *nch, int *ps, int *ppb) {
    *ccb = NW * (64 / na) * BCW;
    *nch = (c + *ccb - 1) / *ccb;
    const int want = (256 + b * *nch - 1) / (b * *nch);
    int s = 1;
    while (s < want) s *= 2;
    const int max_s = (p + 15) / 16;
    if (s > max_s) s = max_s;
    const long long per_range = (long long)b * *nch * n * *ccb * na * (long long)sizeof(float);
    while (s > 1 && per_range * s > (1ll << 30)) s /= 2;
    if (s < 1) s = 1;
    *ppb = (p + s - 1) / s;
    *ps = (p + *ppb - 1) / *ppb;
}

bool sizes_ok(int na, int ks) { return na > 0 && na <= 64 && na % 4 == 0 && ks <= 32; }

}  // namespace

extern "C" int eap_so3_inter_group_fwd_map_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                               const float *feats, const int32_t *idx, const float *gx, const float *rk,
                                               const uint8_t *amap, float *out, eap_stream_t stream) {
    if (!sizes_ok(na, ks)) return eap::bad_arg("so3_inter_group_fwd_map: a multiple of 4 anchors, at most 64; at most 32 kernel points");
    if (b <= 0 || c <= 0 || p <= 0 || ks <= 0) return 0;
    hipStream_t s = eap::S(stream);
    if (nn <= 0 || n <= 0)
        return eap::hip_fail(hipMemsetAsync(out, 0, sizeof(float) * (size_t)b * c * ks * p * na, s), "so3_inter_group_fwd_map memset");
    if (amap == nullptr) return eap::bad_arg("so3_inter_group_fwd_map: the anchor map is required");
    if (20 * (size_t)nn + (size_t)nn * na > 48 * 1024) return eap::bad_arg("so3_inter_group_fwd_map: too many neighbours for one block's shared memory");
    if (ks <= 24) return launch_fwd_map<6>(b, c, p, n, nn, na, ks, sigma, feats, idx, gx, rk, amap, out, s);
    return launch_fwd_map<8>(b, c, p, n, nn, na, ks, sigma, feats, idx, gx, rk, amap, out, s);
}

extern "C" int64_t eap_so3_inter_group_bwd_map_workspace(int b, int c, int p, int n, int na) {
    if (b <= 0 || c <= 0 || p <= 0 || n <= 0 || na <= 0 || na > 64) return 0;
    int ccb, nch, ps, ppb;
    plan(b, c, p, n, na, &ccb, &nch, &ps, &ppb);
    return (int64_t)b * nch * ps * n * ccb * na;
}

extern "C" int eap_so3_inter_group_bwd_map_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                               const float *gout, const int32_t *idx, const float *gx, const float *rk,
                                               const uint8_t *amap, float *gfeats, float *workspace, eap_stream_t stream) {
    if (!sizes_ok(na, ks)) return eap::bad_arg("so3_inter_group_bwd_map: a multiple of 4 anchors, at most 64; at most 32 kernel points");
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    hipStream_t s = eap::S(stream);
    if (p <= 0 || nn <= 0 || ks <= 0)
        return eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(float) * (size_t)b * c * n * na, s), "so3_inter_group_bwd_map memset");
    if (amap == nullptr || workspace == nullptr) return eap::bad_arg("so3_inter_group_bwd_map: the anchor map and the workspace are required");
    const size_t shmem = sizeof(float) * NW * BCW * 64 + 20 * (size_t)nn + (size_t)nn * na + 4 * ((size_t)nn / NB + 1);
    if (shmem > 48 * 1024) return eap::bad_arg("so3_inter_group_bwd_map: too many neighbours for one block's shared memory");
    int ccb, nch, ps, ppb;
    plan(b, c, p, n, na, &ccb, &nch, &ps, &ppb);
    const size_t ws_floats = (size_t)b * nch * ps * n * ccb * na;
    int e = eap::hip_fail(hipMemsetAsync(workspace, 0, sizeof(float) * ws_floats, s), "so3_inter_group_bwd_map memset");
    if (e) return e;
    e = eap::run_kernel("so3_inter_group_bwd_map", ks <= 24 ? so3_inter_group_bwd_map_kernel<24> : so3_inter_group_bwd_map_kernel<32>, ps, nch, b, dim3(T_),
                        shmem, s, c, p, n, nn, na, ks, 1.0f / sigma, nch, ps, ppb, gout, idx, reinterpret_cast<const float4 *>(gx), rk, amap, workspace);
    if (e) return e;
    const long long total = (long long)b * c * n * na;
    return eap::run_kernel("so3_inter_group_bwd_map_reduce", so3_inter_group_bwd_map_reduce_kernel, eap::cdiv(total, 256), 1, 1, dim3(256), 0, s, total, c, n,
                           na, nch, ps, ccb, workspace, gfeats);
}
