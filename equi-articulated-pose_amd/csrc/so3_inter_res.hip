// csrc/so3_inter_res.hip -- the `use_2d` inter conv with REALLY PERMUTED RESIDUAL INDICES: an anchor axis of na x 4 (every
// icosahedral anchor times four rotations about y), where output anchor (a, z) of entry (p, n) reads feature anchor (a, s) with
//   s = rotated_anchor_idx[b,p,n,z] = argmax_j tr(R_rel^T RES_z RES_j^T),   R_rel = R_p R_idx^T
// (vgtk/vgtk/so3conv/functional.py:L1934-1938 the index, L1944-1957 the gather through it, L2124 the weighted sum).  The
// icosahedral index a is never permuted: the whole map of an entry is four 2-bit fields, ONE BYTE (field z = bits 2z, 2z+1).
//
//   index      shift[b,p,n]        = the byte above, searched per entry (16 traces)
//   forward    X[b,c,k,p,a,z]      = sum_n w(p,(a,z),k,n) F[b,c,idx_n,a,shift_z(b,p,n)]
//   backward   dF[b,c,q,a,s]       = sum_{(p,n): idx = q} sum_{z: shift_z = s} sum_k w(p,(a,z),k,n) dX[b,c,k,p,a,z]
//
// The four fields are a cyclic shift where no trace ties; on a tie (the lowest j wins, as torch.argmax) the map is many-to-one, so
// the grouping kernels take ANY byte 0..255.
//
// Forward: block = one point, the 4 waves split the kernel points, lane = (channel group, anchor a).  A lane loads the 16-byte quad
// F[..,a,0..3] of a row once and serves its four outputs z from it -- whole 16 na-byte rows are read, where a kernel per z would read
// every fourth float -- and writes them as one 16-byte store: the reference layout [b,c,ks,p,na*4], one contraction for all anchors.
// The weights w = relu(1 - |g - A_a RES_z kappa_k|^2 / sigma) are evaluated in registers from gx and rk as csrc/so3_inter.hip does.
//
// Backward: the private-slab formulation of csrc/so3_inter_bwd.hip / csrc/so3_inter_map.hip, no float atomics.  Block = (cloud,
// channel chunk, contiguous range of points); wave z evaluates the sums over k of OUTPUT plane z, parks them in LDS, and after one
// block barrier wave s adds, in the order z = 0..3, the ones whose field equals s: wave s owns FEATURE plane s of the slab
// [q][channel][s][a].  A slab word is only ever touched by ONE lane, in program order (points in order, entries in list order, so a
// list that names a row twice is summed in list order; the slab words of eight entries are requested together unless two of them
// name the same row), and a second kernel adds the slabs of the point ranges in range order.  Bit-identical run to run.
#include "common.h"
#include "device_prims.h"

namespace {

constexpr int T_ = 256;     // 4 waves
constexpr int BCW = 4;      // backward: channels per lane
constexpr int NB = 8;       // backward: entries whose slab words are requested together
constexpr unsigned IDENT = 0xE4u;   // field z = z

// ---------------------------------------------------------------------------------------------
// the index: one entry per lane, 16 traces each
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void so3_residual_index_kernel(
    int p, int n_sup, int nn, const int32_t *__restrict__ idx, const float *__restrict__ q_pose,
    const float *__restrict__ s_pose, const float *__restrict__ res, uint8_t *__restrict__ shift,
    int32_t *__restrict__ nontrivial) {
    __shared__ float s_res[36];
    if (threadIdx.x < 36) s_res[threadIdx.x] = res[threadIdx.x];
    __syncthreads();
    const int bi = blockIdx.y;
    const long long total = (long long)p * nn;
    const long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = e0 < total;
    const long long e = live ? e0 : total - 1;        // (idle lanes repeat the last entry and store nothing)
    const int pi = (int)(e / nn);
    const int q = min(max(idx[(size_t)bi * total + e], 0), n_sup - 1);
    const float *Rp = q_pose + ((size_t)bi * p + pi) * 16;
    const float *Rn = s_pose + ((size_t)bi * n_sup + q) * 16;
    float R[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)   // R_rel = R_p R_n^T (the expression of so3_prep_kernel)
            R[i][j] = Rp[i * 4 + 0] * Rn[j * 4 + 0] + Rp[i * 4 + 1] * Rn[j * 4 + 1] + Rp[i * 4 + 2] * Rn[j * 4 + 2];
    unsigned byte = 0u;
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        const float *A = s_res + z * 9;
        float M[9];                                     // M = R_rel^T RES_z
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) M[i * 3 + k] = R[0][i] * A[k] + R[1][i] * A[3 + k] + R[2][i] * A[6 + k];
        float best = -1e30f;
        unsigned arg = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *B = s_res + j * 9;             // tr(M RES_j^T) = <M, RES_j>_F
            const float t = M[0] * B[0] + M[1] * B[1] + M[2] * B[2] + M[3] * B[3] + M[4] * B[4] + M[5] * B[5] + M[6] * B[6] +
                            M[7] * B[7] + M[8] * B[8];
            if (t > best) { best = t; arg = (unsigned)j; }   // strict: the lowest j wins a tie (torch.argmax)
        }
        byte |= arg << (2 * z);
    }
    if (live) shift[(size_t)bi * total + e] = (uint8_t)byte;
    // (no lane has left: lane 0 of every wave is there to report)
    if (__any(live && byte != IDENT) && (threadIdx.x & 63) == 0) atomicOr(nontrivial + bi, 1);
}

// ---------------------------------------------------------------------------------------------
// what a block keeps of one point's list
// ---------------------------------------------------------------------------------------------
struct ResShared {
    float4 *g;       // [nn]
    int32_t *q;      // [nn]
    uint8_t *sh;     // [nn]
};

__host__ __device__ inline size_t list_bytes(int nn) { return (21 * (size_t)nn + 15) & ~(size_t)15; }

__device__ __forceinline__ ResShared carve(unsigned char *base, int nn) {
    ResShared s;
    s.g = reinterpret_cast<float4 *>(base);
    s.q = reinterpret_cast<int32_t *>(base + 16 * (size_t)nn);
    s.sh = base + 20 * (size_t)nn;
    return s;
}

__device__ __forceinline__ void load_point(const ResShared &s, size_t pn, int nn, int n_sup, const int32_t *idx, const float4 *gx,
                                           const uint8_t *shift) {
    for (int i = threadIdx.x; i < nn; i += T_) {
        s.g[i] = gx[pn + i];
        const int q = idx[pn + i];
        s.q[i] = q < n_sup ? q : -1;   // shadow row (all zeros in the reference) -> skipped
        s.sh[i] = shift[pn + i];
    }
}

// component `sel` (wave-uniform, 0..3) of a quad: the four are NAMED, then selected -- no dynamically indexed register array
__device__ __forceinline__ float pick(const float4 &f, unsigned sel) {
    const float lo = (sel & 1u) ? f.y : f.x, hi = (sel & 1u) ? f.w : f.z;
    return (sel & 2u) ? hi : lo;
}

// ---------------------------------------------------------------------------------------------
// forward: the 4 waves split the kernel points, a lane keeps CC x 4 x KPW outputs of its (channel group, anchor)
// ---------------------------------------------------------------------------------------------
template <int KPW, int CC>
__global__ __launch_bounds__(T_) void so3_inter_group_fwd_res_kernel(
    int c, int p, int n_sup, int nn, int na, int ks, float inv_sigma, const float *__restrict__ feats,
    const int32_t *__restrict__ idx, const float4 *__restrict__ gx, const float *__restrict__ rk,
    const uint8_t *__restrict__ shift, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ResShared s = carve(smem, nn);
    const int pi = xcd_point(blockIdx.x, p), bi = blockIdx.y;
    load_point(s, ((size_t)bi * p + pi) * nn, nn, n_sup, idx, gx, shift);
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncg = 64 / na, cg = lane / na, a = lane - cg * na;
    const int k0 = wave * KPW;
    if (cg >= ncg || k0 >= ks) return;

    float kx[4][KPW], ky[4][KPW], kz[4][KPW];
#pragma unroll
    for (int z = 0; z < 4; ++z)
#pragma unroll
        for (int kk = 0; kk < KPW; ++kk) {
            const float *r3 = rk + ((size_t)(a * 4 + z) * ks + min(k0 + kk, ks - 1)) * 3;
            kx[z][kk] = r3[0]; ky[z][kk] = r3[1]; kz[z][kk] = r3[2];
        }
    const float4 *fb = reinterpret_cast<const float4 *>(feats) + (size_t)bi * c * n_sup * na;      // quads [c][n][na]
    const size_t f_cs = (size_t)n_sup * na;
    float *ob = out + ((size_t)bi * c * ks * p * na + (size_t)pi * na + a) * 4;
    const size_t o_ks = (size_t)p * na * 4, o_cs = (size_t)ks * p * na * 4;

    for (int c0 = cg; c0 < c; c0 += CC * ncg) {           // this lane's channels: c0 + cc * ncg
        float acc[CC][4][KPW];
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
#pragma unroll
            for (int z = 0; z < 4; ++z)
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk) acc[cc][z][kk] = 0.f;
        for (int n = 0; n < nn; ++n) {
            const int q = s.q[n];
            if (q < 0) continue;   // wave-uniform
            const float4 g = s.g[n];
            const unsigned byte = s.sh[n];
            float wv[4][KPW];
#pragma unroll
            for (int z = 0; z < 4; ++z)
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk) {
                    const float dx = g.x - kx[z][kk], dy = g.y - ky[z][kk], dz = g.z - kz[z][kk];
                    wv[z][kk] = fmaxf(1.0f - (dx * dx + dy * dy + dz * dz) * inv_sigma, 0.0f);
                }
            const float4 *f = fb + (size_t)q * na + a;
#pragma unroll
            for (int cc = 0; cc < CC; ++cc) {
                const float4 f4 = (c0 + cc * ncg < c) ? f[(size_t)(c0 + cc * ncg) * f_cs] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int z = 0; z < 4; ++z) {
                    const float fv = pick(f4, (byte >> (2 * z)) & 3u);
#pragma unroll
                    for (int kk = 0; kk < KPW; ++kk) acc[cc][z][kk] = fmaf(fv, wv[z][kk], acc[cc][z][kk]);
                }
            }
        }
#pragma unroll
        for (int cc = 0; cc < CC; ++cc)
            if (c0 + cc * ncg < c) {
#pragma unroll
                for (int kk = 0; kk < KPW; ++kk)
                    if (k0 + kk < ks)
                        *reinterpret_cast<float4 *>(ob + (size_t)(c0 + cc * ncg) * o_cs + (size_t)(k0 + kk) * o_ks) =
                            make_float4(acc[cc][0][kk], acc[cc][1][kk], acc[cc][2][kk], acc[cc][3][kk]);
            }
    }
}

template <int KPW>
int launch_fwd_res(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats, const int32_t *idx,
                   const float *gx, const float *rk, const uint8_t *shift, float *out, hipStream_t s) {
    const int ncg = 64 / na;
    auto kern = so3_inter_group_fwd_res_kernel<KPW, 1>;
    if (c > ncg) kern = c <= 2 * ncg ? so3_inter_group_fwd_res_kernel<KPW, 2> : so3_inter_group_fwd_res_kernel<KPW, 4>;
    return eap::run_kernel("so3_inter_group_fwd_res", kern, p, b, 1, dim3(T_), list_bytes(nn), s, c, p, n, nn, na, ks, 1.0f / sigma, feats, idx,
                           reinterpret_cast<const float4 *>(gx), rk, shift, out);
}

// ---------------------------------------------------------------------------------------------
// backward: private slabs, see the header of this file
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ld_l2(const float *p) {
    // bypasses L1 (served by L2), so a lane always sees its own earlier (write-through) stores to the slab
    return __builtin_nontemporal_load(p);
}

template <int KS_MAX>
__global__ __launch_bounds__(T_) void so3_inter_group_bwd_res_kernel(
    int c, int p, int n_sup, int nn, int na, int ks, float inv_sigma, int nch, int ps, int ppb,
    const float *__restrict__ gout, const int32_t *__restrict__ idx, const float4 *__restrict__ gx,
    const float *__restrict__ rk, const uint8_t *__restrict__ shift, float *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_t = reinterpret_cast<float *>(smem);                                  // [2][4][BCW][64] per-plane sums of one entry, two buffers
    const ResShared s = carve(smem + sizeof(float) * 2 * 4 * BCW * 64, nn);
    int32_t *s_dup = reinterpret_cast<int32_t *>(smem + sizeof(float) * 2 * 4 * BCW * 64 + list_bytes(nn));   // [nn / NB + 1]
    const int ngroups = (nn + NB - 1) / NB;

    const int split = blockIdx.x, chunk = blockIdx.y, bi = blockIdx.z;
    const int z = threadIdx.x >> 6, lane = threadIdx.x & 63;      // the wave: output plane z while it sums over k, feature plane z at the slab
    const int ncg = 64 / na, cg = lane / na, a = min(lane - cg * na, na - 1);
    const bool act = cg < ncg;
    const int ccb = ncg * BCW;                              // channels per block
    const int p_beg = split * ppb, p_end = min(p, p_beg + ppb);
    float *slab = ws + (((size_t)bi * nch + chunk) * ps + split) * ((size_t)n_sup * ccb * 4 * na);

    float kx[KS_MAX], ky[KS_MAX], kz[KS_MAX];
#pragma unroll
    for (int k = 0; k < KS_MAX; ++k) {
        const float *r3 = rk + ((size_t)(a * 4 + z) * ks + min(k, ks - 1)) * 3;
        kx[k] = r3[0]; ky[k] = r3[1]; kz[k] = r3[2];
    }
    int chl[BCW];                                           // this lane's channels within the block's chunk
    bool live[BCW];
#pragma unroll
    for (int cc = 0; cc < BCW; ++cc) {
        chl[cc] = cc * ncg + min(cg, ncg - 1);
        live[cc] = act && chunk * ccb + chl[cc] < c;
    }
    const size_t o_ks = (size_t)p * na * 4, o_cs = (size_t)ks * p * na * 4;
    int buf = 0;

    for (int pi = p_beg; pi < p_end; ++pi) {
        __syncthreads();   // the previous point's reads of s.g / s.q / s.sh / s_dup are done
        load_point(s, ((size_t)bi * p + pi) * nn, nn, n_sup, idx, gx, shift);
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
            const float *src = gout + (size_t)bi * c * o_cs + (size_t)min(chunk * ccb + chl[cc], c - 1) * o_cs + ((size_t)pi * na + a) * 4 + z;
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
                        old[nl][cc] = live[cc] ? ld_l2(slab + (((size_t)q * ccb + chl[cc]) * 4 + z) * na + a) : 0.f;
                }
            }
#pragma unroll
            for (int nl = 0; nl < NB; ++nl) {
                const int n = n0 + nl;
                const int q = n < nn ? s.q[n] : -1;
                if (q < 0) continue;   // block-uniform: every thread of the block skips the barrier below, or none does
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
                // output plane z contributes to feature plane shift_z: parked per (plane, channel, lane); after the barrier the wave
                // that owns feature plane s adds the ones whose field equals s, in the order z = 0..3.  Two buffers, alternating over
                // the entries that run: a wave that parks entry j has passed the barrier of entry j - 1, which every wave reaches only
                // after its reads of entry j - 2 -- the buffer's previous use
                float *tb = s_t + buf * (4 * BCW * 64);
#pragma unroll
                for (int cc = 0; cc < BCW; ++cc) tb[(z * BCW + cc) * 64 + lane] = t[cc];
                __syncthreads();
                const unsigned byte = s.sh[n];
                float sum[BCW];
#pragma unroll
                for (int cc = 0; cc < BCW; ++cc) sum[cc] = 0.f;
#pragma unroll
                for (int z2 = 0; z2 < 4; ++z2) {
                    const bool hit = ((byte >> (2 * z2)) & 3u) == (unsigned)z;
#pragma unroll
                    for (int cc = 0; cc < BCW; ++cc) {
                        const float v = tb[(z2 * BCW + cc) * 64 + lane];
                        sum[cc] += hit ? v : 0.f;
                    }
                }
                buf ^= 1;
#pragma unroll
                for (int cc = 0; cc < BCW; ++cc)
                    if (live[cc]) {
                        float *word = slab + (((size_t)q * ccb + chl[cc]) * 4 + z) * na + a;
                        *word = (prefetch ? old[nl][cc] : ld_l2(word)) + sum[cc];   // a row named twice: ordered slow path
                    }
            }
        }
    }
}

// gfeats[b,c,q,a,s] = sum over the point ranges, in range order, of slab[b,chunk,split][q][c % ccb][s][a]
__global__ void so3_inter_group_bwd_res_reduce_kernel(long long total, int c, int n_sup, int na, int nch, int ps, int ccb,
                                                      const float *__restrict__ ws, float *__restrict__ gfeats) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over (b,c,q,a,s)
    if (e >= total) return;
    const int sp = (int)(e & 3);
    long long r = e >> 2;
    const int a = (int)(r % na); r /= na;
    const int q = (int)(r % n_sup); r /= n_sup;
    const int ci = (int)(r % c);
    const int bi = (int)(r / c);
    const int chunk = ci / ccb, cc = ci - chunk * ccb;
    const size_t slab_sz = (size_t)n_sup * ccb * 4 * na;
    const float *src = ws + ((size_t)bi * nch + chunk) * ps * slab_sz + (((size_t)q * ccb + cc) * 4 + sp) * na + a;
    float sum = 0.f;
    for (int i = 0; i < ps; ++i) sum += src[(size_t)i * slab_sz];
    gfeats[e] = sum;
}

// channel chunks, point ranges and points per range of the backward: at least one block per CU where the points allow,
// at least 16 points per block, at most 1 GiB of slabs where one range per chunk fits in it
void plan(int b, int c, int p, int n, int na, int *ccb, int *nch, int *ps, int *ppb) {
    *ccb = (64 / na) * BCW;
    *nch = (c + *ccb - 1) / *ccb;
    const long long blocks = (long long)b * *nch;
    const long long want = (256 + blocks - 1) / blocks;
    int s = 1;
    while (s < want) s *= 2;
    const int max_s = (p + 15) / 16;
    if (s > max_s) s = max_s;
    const long long per_range = blocks * n * *ccb * 4 * na * (long long)sizeof(float);
    while (s > 1 && per_range * s > (1ll << 30)) s /= 2;
    if (s < 1) s = 1;
    *ppb = (p + s - 1) / s;
    *ps = (p + *ppb - 1) / *ppb;
}

bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }

// the sizes every grouping entry takes; positive ones past this point
int sizes_ok(const char *what, int b, int c, int p, int n, int nn, int na, int ks) {
    char buf[192];
    if (na <= 0 || na > 64 || ks > 32 || b < 0 || c < 0 || p < 0 || n < 0 || nn < 0 || ks < 0) {
        snprintf(buf, sizeof(buf), "%s: 1..64 anchors (times four residual rotations), at most 32 kernel points, no negative size", what);
        return eap::bad_arg(buf);
    }
    return 0;
}

}  // namespace

extern "C" int eap_so3_residual_index_f32(int b, int p, int n, int nn, const int32_t *idx, const float *q_pose,
                                          const float *s_pose, const float *res, uint8_t *shift, int32_t *nontrivial,
                                          eap_stream_t stream) {
    if (b < 0 || p < 0 || n < 0 || nn < 0) return eap::bad_arg("so3_residual_index: no negative size");
    if (q_pose == nullptr || s_pose == nullptr || res == nullptr) return eap::bad_arg("so3_residual_index: both pose tensors and the residual rotations are required");
    if (b == 0) return 0;
    if (nontrivial == nullptr) return eap::bad_arg("so3_residual_index: the per-cloud flags are required");
    const bool work = p > 0 && nn > 0;
    if (work && (n <= 0 || idx == nullptr || shift == nullptr)) return eap::bad_arg("so3_residual_index: no support points, or no index / output");
    dim3 grid;
    if (work)
        if (int e = eap::launch_dims("so3_residual_index", eap::cdiv((long long)p * nn, 256), b, 1, dim3(256), &grid)) return e;
    int e = eap::hip_fail(hipMemsetAsync(nontrivial, 0, sizeof(int32_t) * b, eap::S(stream)), "so3_residual_index memset");
    if (e || !work) return e;
    return eap::run_kernel("so3_residual_index", so3_residual_index_kernel, eap::cdiv((long long)p * nn, 256), b, 1, dim3(256), 0, eap::S(stream), p, n, nn,
                           idx, q_pose, s_pose, res, shift, nontrivial);
}

extern "C" int eap_so3_inter_group_fwd_res_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                               const float *feats, const int32_t *idx, const float *gx, const float *rk,
                                               const uint8_t *shift, float *out, eap_stream_t stream) {
    if (int e = sizes_ok("so3_inter_group_fwd_res", b, c, p, n, nn, na, ks)) return e;
    if (!aligned16(feats) || !aligned16(out)) return eap::bad_arg("so3_inter_group_fwd_res: feats and out must be 16-byte aligned");
    if (b == 0 || c == 0 || p == 0 || ks == 0) return 0;
    if (out == nullptr) return eap::bad_arg("so3_inter_group_fwd_res: out is required");
    hipStream_t s = eap::S(stream);
    if (nn == 0 || n == 0)
        return eap::hip_fail(hipMemsetAsync(out, 0, sizeof(float) * (size_t)b * c * ks * p * na * 4, s), "so3_inter_group_fwd_res memset");
    if (feats == nullptr || idx == nullptr || gx == nullptr || rk == nullptr || shift == nullptr)
        return eap::bad_arg("so3_inter_group_fwd_res: feats, idx, gx, rk and the residual index are required");
    if (list_bytes(nn) > 48 * 1024) return eap::bad_arg("so3_inter_group_fwd_res: too many neighbours for one block's shared memory");
    if (ks <= 24) return launch_fwd_res<6>(b, c, p, n, nn, na, ks, sigma, feats, idx, gx, rk, shift, out, s);
    return launch_fwd_res<8>(b, c, p, n, nn, na, ks, sigma, feats, idx, gx, rk, shift, out, s);
}

extern "C" int64_t eap_so3_inter_group_bwd_res_workspace(int b, int c, int p, int n, int na) {
    if (b <= 0 || c <= 0 || p <= 0 || n <= 0 || na <= 0 || na > 64) return 0;
    int ccb, nch, ps, ppb;
    plan(b, c, p, n, na, &ccb, &nch, &ps, &ppb);
    return (int64_t)b * nch * ps * n * ccb * 4 * na;
}

extern "C" int eap_so3_inter_group_bwd_res_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                               const float *gout, const int32_t *idx, const float *gx, const float *rk,
                                               const uint8_t *shift, float *gfeats, float *workspace, eap_stream_t stream) {
    if (int e = sizes_ok("so3_inter_group_bwd_res", b, c, p, n, nn, na, ks)) return e;
    if (!aligned16(gout) || !aligned16(gfeats)) return eap::bad_arg("so3_inter_group_bwd_res: gout and gfeats must be 16-byte aligned");
    if (b == 0 || c == 0 || n == 0) return 0;
    if (gfeats == nullptr) return eap::bad_arg("so3_inter_group_bwd_res: gfeats is required");
    hipStream_t s = eap::S(stream);
    if (p == 0 || nn == 0 || ks == 0)
        return eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(float) * (size_t)b * c * n * na * 4, s), "so3_inter_group_bwd_res memset");
    if (gout == nullptr || idx == nullptr || gx == nullptr || rk == nullptr || shift == nullptr || workspace == nullptr)
        return eap::bad_arg("so3_inter_group_bwd_res: gout, idx, gx, rk, the residual index and the workspace are required");
    const size_t shmem = sizeof(float) * 2 * 4 * BCW * 64 + list_bytes(nn) + 4 * ((size_t)nn / NB + 1);
    if (shmem > 48 * 1024) return eap::bad_arg("so3_inter_group_bwd_res: too many neighbours for one block's shared memory");
    int ccb, nch, ps, ppb;
    plan(b, c, p, n, na, &ccb, &nch, &ps, &ppb);
    const long long total = (long long)b * c * n * na * 4;
    dim3 grid;      // both grids before anything is queued
    if (int e = eap::launch_dims("so3_inter_group_bwd_res", ps, nch, b, dim3(T_), &grid)) return e;
    if (int e = eap::launch_dims("so3_inter_group_bwd_res_reduce", eap::cdiv(total, 256), 1, 1, dim3(256), &grid)) return e;
    const size_t ws_floats = (size_t)b * nch * ps * n * ccb * 4 * na;
    int e = eap::hip_fail(hipMemsetAsync(workspace, 0, sizeof(float) * ws_floats, s), "so3_inter_group_bwd_res memset");
    if (e) return e;
    e = eap::run_kernel("so3_inter_group_bwd_res", ks <= 24 ? so3_inter_group_bwd_res_kernel<24> : so3_inter_group_bwd_res_kernel<32>, ps, nch, b, dim3(T_),
                        shmem, s, c, p, n, nn, na, ks, 1.0f / sigma, nch, ps, ppb, gout, idx, reinterpret_cast<const float4 *>(gx), rk, shift, workspace);
    if (e) return e;
    return eap::run_kernel("so3_inter_group_bwd_res_reduce", so3_inter_group_bwd_res_reduce_kernel, eap::cdiv(total, 256), 1, 1, dim3(256), 0, s, total, c, n,
                           na, nch, ps, ccb, workspace, gfeats);
}
