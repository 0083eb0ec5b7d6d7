// csrc/pointnet_max.hip -- PointnetSO3Conv / PointnetSO3PoseConv (vgtk/vgtk/so3conv/modules.py:L393-413, L432-449): the 1x1 `embed` over
// [feats ; A_a^T (x - centre)] fused with the max over the points.  With W = embed.weight [O, C+3], W_f = W[:, :C], W_x = W[:, C:],
// V[o,a,:] = A_a W_x[o,:] and xc = xyz - centre[b]:
//     y[b,o,n,a] = sum_c W_f[o,c] feats[b,c,n,a] + V[o,a,:] . xc[b,:,n] + bias[o]          (never written)
//     out[b,o,a] = max over the member points n of y,   arg[b,o,a] = the lowest member n attaining it
// Neither y, the (C+3)-channel concatenation nor the coordinate channels [B,3,N,A] exist in the forward.
//
// Forward mapping (the operands swapped as in DESIGN section 7 item 3: the POINTS on the MFMA's M side).  A feature row feats[b,c,:,:] is one
// run of n * na floats; 8 points x na anchors (na % 4 == 0) are na / 4 whole tiles of 32 flat columns.  A workgroup = (32 output channels,
// PN_GROUP = 128 points of one cloud), 8 waves, walks its 16 chunks of 8 points in ascending order; wave w owns the tiles t = w, w + 8 of every
// chunk (at most 2), one v_mfma_f32_32x32x2_f32 accumulator each: A[i = flat column][k = channel] one dword per lane straight from global
// memory (128 contiguous bytes per half-wave), B[k = channel][j = output channel] one dword of wt = W_f transposed [C, O] (the caller makes it:
// 32 consecutive output channels per half-wave) shared by the wave's tiles.  After the k loop
// a lane holds, for ITS output channel, 16 flat columns per tile, and register (tile, r) names the same anchor in every chunk (8 na is a
// multiple of 32) at the point chunk + const: the rank-3 term, the bias and a running (max, arg) per register are lane-private VALU work;
// ascending chunks and ">" keep the lowest point of equals.  At the end the 8 point residues of every (channel, anchor) are folded through LDS
// (one owner lane per residue and round, so plain read-modify-write), the workgroup writes one partial per (channel, anchor), and a second
// kernel folds the partials of a cloud in ascending order.  No atomics: bit-identical run to run.  NaN is compared explicitly (v_max_f32
// drops it): the first NaN of a chain stays, a NaN beats every number between chains, the lower point wins between two NaNs.
//
// Backward: dfeats[b,c,n,a] = sum_{o: arg[b,o,a] = n} W_f[o,c] g[b,o,a] touches at most O points per (cloud, anchor): one workgroup per
// (cloud, anchor) links the channels that share a point into chains (ascending o), and writes one sum per (chain, input channel) -- the three
// coordinate channels included, as dcoords [B,3,N,A]; the caller zero-fills both.  dW[o,:] = sum_{b,a} g feats[b,:,arg,a] is a gather-sum per
// (cloud, channel) over the anchors in ascending order; the clouds are added by the caller in float64.
#include "common.h"
#include "device_prims.h"

#include <initializer_list>

namespace {

constexpr int PN_CHUNK = 8;        // points per chunk: 8 na flat columns = na / 4 tiles
constexpr int PN_GROUP = 128;      // points per workgroup = per partial
constexpr int PN_OB = 32;          // output channels per workgroup: the N side of one tile
constexpr int PN_WAVES = 8, PN_THREADS = 64 * PN_WAVES;
constexpr int PN_SLOTS = 2;        // tiles per wave and chunk: 8 waves x 2 >= 64 / 4
constexpr int PN_KU = 4;           // k-steps per trip; three trips' operands are held (8, or 16 waves x 1 tile x 8, spill: DESIGN.md 3.2.6)
constexpr int PN_MAXNA = 64;
constexpr int PN_MAXO = 2048;      // output channels the backward's LDS tables hold

// within a lane's ascending chain: the first value, a larger one, or the first NaN
__device__ __forceinline__ bool pn_chain_takes(float a, float best, int at) { return at < 0 || a > best || (a != a && best == best); }
// between chains (k, at < 0: empty): NaN first, else the larger, the lower point among equals (-0.0 == +0.0)
__device__ __forceinline__ bool pn_fold_takes(float u, int k, float best, int at) {
    if (k < 0) return false;
    if (at < 0) return true;
    const bool un = u != u, bn = best != best;
    return (un || bn) ? (un && (!bn || k < at)) : (u > best || (u == best && k < at));
}

template <int NA>
__global__ __launch_bounds__(PN_THREADS) void pointnet_max_kernel(int nb, int c, int o, int n, int na_rt, int parts, const float *__restrict__ feats,
                                                           const float *__restrict__ xyz, const float *__restrict__ centre,
                                                           const float *__restrict__ member, const float *__restrict__ wt,
                                                           const float *__restrict__ v, const float *__restrict__ bias,
                                                           float *__restrict__ pval, int32_t *__restrict__ parg) {
    __shared__ float s_v[PN_MAXNA * 3 * PN_OB];               // [anchor][component][channel]
    __shared__ float s_bv[PN_MAXNA * (PN_OB + 1)];            // [anchor][channel], padded: the fold of the point residues
    __shared__ int s_bi[PN_MAXNA * (PN_OB + 1)];
    __shared__ float s_x[3 * PN_GROUP];                       // centred coordinates of the workgroup's points
    __shared__ float s_m[PN_GROUP];                           // membership (0 past the cloud's end)
    const int na = NA ? NA : na_rt;
    // workgroups go to the 8 XCDs round-robin by linear id: the channel blocks of one (cloud, point group) run back to back on ONE XCD and
    // read its feature rows through that XCD's L2 once
    const unsigned xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, nob = (unsigned)(o + PN_OB - 1) / PN_OB;
    const unsigned pb = (slot / nob) * 8u + xcd;
    if (pb >= (unsigned)parts * (unsigned)nb) return;                             // (the whole workgroup: the pairs are padded to a multiple of 8)
    const int ob = slot % nob, part = pb % (unsigned)parts, bi = pb / (unsigned)parts;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, kh = lane >> 5;
    const int p_lo = part * PN_GROUP, p_hi = min(n, p_lo + PN_GROUP);
    const int oo = ob * PN_OB + li;
    const bool o_ok = oo < o;
    for (int e = tid; e < na * 3 * PN_OB; e += PN_THREADS) {
        const int ol = e % PN_OB, aj = e / PN_OB, og = ob * PN_OB + ol;
        s_v[e] = og < o ? v[(size_t)og * na * 3 + aj] : 0.f;
    }
    for (int e = tid; e < PN_GROUP; e += PN_THREADS) {
        const int p = p_lo + e;
        const bool ok = p < p_hi;
#pragma unroll
        for (int j = 0; j < 3; ++j) s_x[j * PN_GROUP + e] = ok ? xyz[((size_t)bi * 3 + j) * n + p] - centre[bi * 3 + j] : 0.f;
        s_m[e] = ok ? (member ? member[(size_t)bi * n + p] : 1.f) : 0.f;
    }
    for (int e = tid; e < na * (PN_OB + 1); e += PN_THREADS) { s_bv[e] = 0.f; s_bi[e] = -1; }
    __syncthreads();

    const int ntiles = na >> 2;
    const float bo = (o_ok && bias) ? bias[oo] : 0.f;
    float best[PN_SLOTS][16];
    int at[PN_SLOTS][16];
#pragma unroll
    for (int s = 0; s < PN_SLOTS; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) { best[s][r] = 0.f; at[s][r] = -1; }
    const size_t rowlen = (size_t)n * na;
    const float *fb = feats + (size_t)bi * c * rowlen;
    const float *wcol = wt + min(oo, o - 1);                  // W_f transposed [c, o]: a half-wave reads 32 consecutive floats
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (int pc = p_lo; pc < p_hi; pc += PN_CHUNK) {
        f32x16 acc[PN_SLOTS];
#pragma unroll
        for (int s = 0; s < PN_SLOTS; ++s) acc[s] = zero16;
        const size_t cbase = (size_t)pc * na + li;
        // the operands of one trip = PN_KU k-steps (2 channels each): a tile column past the cloud's end, a channel past c and a tile the
        // wave does not own read nothing and feed zeros
        auto load_block = [&](int k0, float (&fa)[PN_KU][PN_SLOTS], float (&fw)[PN_KU]) {
#pragma unroll
            for (int u = 0; u < PN_KU; ++u) {
                const int cc = k0 + 2 * u + kh;
                const bool cok = cc < c;
                fw[u] = (cok && o_ok) ? wcol[(size_t)cc * o] : 0.f;
                const float *row = fb + (size_t)min(cc, c - 1) * rowlen;
#pragma unroll
                for (int s = 0; s < PN_SLOTS; ++s) {
                    const size_t col = cbase + 32 * (wave + PN_WAVES * s);
                    fa[u][s] = (cok && wave + PN_WAVES * s < ntiles && col < rowlen) ? row[col] : 0.f;
                }
            }
        };
        auto products = [&](const float (&fa)[PN_KU][PN_SLOTS], const float (&fw)[PN_KU]) {
#pragma unroll
            for (int u = 0; u < PN_KU; ++u)
#pragma unroll
                for (int s = 0; s < PN_SLOTS; ++s)
                    if (wave + PN_WAVES * s < ntiles)                            // (wave-uniform)
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u][s], fw[u], acc[s], 0, 0, 0);
        };
        // three register sets in rotation: the loads of a trip are issued two trips of products before they are used, and no set is copied
        constexpr int KT = 2 * PN_KU;                                            // channels per trip
        float a0[PN_KU][PN_SLOTS], w0[PN_KU], a1[PN_KU][PN_SLOTS], w1[PN_KU], a2[PN_KU][PN_SLOTS], w2[PN_KU];
        load_block(0, a0, w0);
        load_block(KT, a1, w1);
        for (int k0 = 0; k0 < c; k0 += 3 * KT) {
            load_block(k0 + 2 * KT, a2, w2);
            products(a0, w0);
            if (k0 + KT >= c) break;
            load_block(k0 + 3 * KT, a0, w0);
            products(a1, w1);
            if (k0 + 2 * KT >= c) break;
            load_block(k0 + 4 * KT, a1, w1);
            products(a2, w2);
        }
        // D: column = lane & 31 (this lane's output channel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (the flat column within the tile)
#pragma unroll
        for (int s = 0; s < PN_SLOTS; ++s) {
            const int t = wave + PN_WAVES * s;
            if (t < ntiles) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * kh, pi = f / na, a = f - pi * na;
                    const int p = pc + pi, pl = p - p_lo;                 // pl < PN_GROUP: pc - p_lo <= PN_GROUP - 8, pi < 8
                    if (p < p_hi && s_m[pl] != 0.f) {
                        const float *vp = s_v + a * 3 * PN_OB + li;
                        // (spelled with fmaf: one order of operations for every register, equal points give equal bits)
                        const float y = acc[s][r] + fmaf(vp[2 * PN_OB], s_x[2 * PN_GROUP + pl], fmaf(vp[PN_OB], s_x[PN_GROUP + pl], vp[0] * s_x[pl])) + bo;
                        if (pn_chain_takes(y, best[s][r], at[s][r])) { best[s][r] = y; at[s][r] = p; }
                    }
                }
            }
        }
    }

    // the 8 point residues of every (channel, anchor): residue `round` of (anchor a, channel li) is held by exactly one (wave, slot, r, half-wave)
#pragma unroll 1
    for (int round = 0; round < PN_CHUNK; ++round) {
#pragma unroll
        for (int s = 0; s < PN_SLOTS; ++s) {
            const int t = wave + PN_WAVES * s;
            if (t < ntiles) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * kh, pi = f / na, a = f - pi * na;
                    if (pi == round) {
                        const int i = a * (PN_OB + 1) + li;
                        if (pn_fold_takes(best[s][r], at[s][r], s_bv[i], s_bi[i])) { s_bv[i] = best[s][r]; s_bi[i] = at[s][r]; }
                    }
                }
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < PN_OB * na; e += PN_THREADS) {
        const int ol = e / na, a = e - ol * na, og = ob * PN_OB + ol;
        if (og < o) {
            const size_t dst = (((size_t)bi * parts + part) * o + og) * na + a;
            pval[dst] = s_bv[a * (PN_OB + 1) + ol];
            parg[dst] = s_bi[a * (PN_OB + 1) + ol];
        }
    }
}

// out, arg [b, o*na] from the partials [b, parts, o*na], ascending parts (a cloud without a member: -inf and -1)
__global__ __launch_bounds__(256) void pointnet_max_fold_kernel(long long total, int ona, int parts, const float *__restrict__ pval,
                                                                const int32_t *__restrict__ parg, float *__restrict__ out,
                                                                int32_t *__restrict__ arg) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long bi = e / ona, r = e - bi * ona;
    const size_t src = (size_t)bi * parts * ona + r;
    float best = 0.f;
    int at = -1;
    for (int part = 0; part < parts; ++part) {
        const float u = pval[src + (size_t)part * ona];
        const int k = parg[src + (size_t)part * ona];
        if (pn_fold_takes(u, k, best, at)) { best = u; at = k; }
    }
    out[e] = at < 0 ? -INFINITY : best;
    arg[e] = at;
}

// block = (anchor, cloud): the o channels of the pair grouped by their arg point, each group summed in ascending o for every input channel
// and the three coordinate channels (column c + i of w)
__global__ __launch_bounds__(256) void pointnet_max_bwd_data_kernel(int c, int o, int n, int na, const float *__restrict__ g,
                                                                    const int32_t *__restrict__ arg, const float *__restrict__ w, int ldw,
                                                                    float *__restrict__ dfeats, float *__restrict__ dcoords) {
    __shared__ int s_arg[PN_MAXO];          // the point, -1: none (no member, or an index outside the cloud)
    __shared__ int s_next[PN_MAXO];         // the next higher channel with the same point, -1: last
    __shared__ int s_lead[PN_MAXO];         // the lowest channel of its group
    __shared__ float s_g[PN_MAXO];
    const int a = blockIdx.x, bi = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < o; i += 256) {
        const size_t idx = ((size_t)bi * o + i) * na + a;
        const int p = arg[idx];
        s_arg[i] = (p >= 0 && p < n) ? p : -1;
        s_g[i] = g[idx];
    }
    __syncthreads();
    for (int i = tid; i < o; i += 256) {
        const int p = s_arg[i];
        int nx = -1, lead = p >= 0;
        if (p >= 0) {
            for (int j = i + 1; j < o; ++j)
                if (s_arg[j] == p) { nx = j; break; }
            for (int j = 0; j < i; ++j)
                if (s_arg[j] == p) { lead = 0; break; }
        }
        s_next[i] = nx;
        s_lead[i] = lead;
    }
    __syncthreads();
    for (int cc = dfeats ? tid : c + tid; cc < (dcoords ? c + 3 : c); cc += 256) {
        for (int i = 0; i < o; ++i) {
            if (!s_lead[i]) continue;
            float acc = 0.f;
            for (int j = i; j >= 0; j = s_next[j]) acc = fmaf(w[(size_t)j * ldw + cc], s_g[j], acc);
            const int p = s_arg[i];
            if (cc < c) dfeats[(((size_t)bi * c + cc) * n + p) * na + a] = acc;
            else dcoords[(((size_t)bi * 3 + (cc - c)) * n + p) * na + a] = acc;
        }
    }
}

// block = (output channel, cloud): dwp[b,o,:] = sum_a g[b,o,a] [feats[b,:,p,a] ; A_a^T xc[b,:,p] ; 1] at p = arg[b,o,a], anchors ascending
__global__ __launch_bounds__(256) void pointnet_max_bwd_weight_kernel(int c, int o, int n, int na, const float *__restrict__ g,
                                                                      const int32_t *__restrict__ arg, const float *__restrict__ feats,
                                                                      const float *__restrict__ xyz, const float *__restrict__ centre,
                                                                      const float *__restrict__ anchors, float *__restrict__ dwp) {
    __shared__ int s_p[PN_MAXNA];
    __shared__ float s_g[PN_MAXNA];
    __shared__ float s_co[PN_MAXNA][3];
    const int oi = blockIdx.x, bi = blockIdx.y, tid = threadIdx.x;
    if (tid < na) {
        const size_t idx = ((size_t)bi * o + oi) * na + tid;
        const int p = arg[idx];
        const bool ok = p >= 0 && p < n;
        s_p[tid] = ok ? p : -1;
        s_g[tid] = g[idx];
        float x[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) x[j] = ok ? xyz[((size_t)bi * 3 + j) * n + p] - centre[bi * 3 + j] : 0.f;
        const float *A = anchors + tid * 9;
#pragma unroll
        for (int i = 0; i < 3; ++i) s_co[tid][i] = (A[i] * x[0] + A[3 + i] * x[1]) + A[6 + i] * x[2];
    }
    __syncthreads();
    for (int cc = tid; cc < c + 4; cc += 256) {
        float acc = 0.f;
        for (int a = 0; a < na; ++a) {
            const int p = s_p[a];
            if (p < 0) continue;
            const float val = cc < c ? feats[(((size_t)bi * c + cc) * n + p) * na + a] : cc < c + 3 ? s_co[a][cc - c] : 1.f;
            acc = fmaf(s_g[a], val, acc);
        }
        dwp[((size_t)bi * o + oi) * (c + 4) + cc] = acc;
    }
}

// sizes first (the operand named), then the pointers: nothing is queued past a refusal
inline int pointnet_dims(const char *who, int c, int o, int n, int na) {
    char buf[200];
    const char *bad = c <= 0 ? "c (input channels) must be positive" : o <= 0 ? "o (output channels) must be positive"
                    : o > PN_MAXO ? "o (output channels) must be at most 2048" : n <= 0 ? "n (points) must be positive"
                    : (na <= 0 || na > PN_MAXNA || (na & 3) != 0) ? "na (anchors) must be a multiple of 4, at most 64" : nullptr;
    if (!bad) return 0;
    snprintf(buf, sizeof(buf), "%s: %s", who, bad);
    return eap::bad_arg(buf);
}

inline int pointnet_null(const char *who, const char *names, std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!p) {
            char buf[240];
            snprintf(buf, sizeof(buf), "%s: a null pointer among %s", who, names);
            return eap::bad_arg(buf);
        }
    return 0;
}

}  // namespace

extern "C" int eap_pointnet_max_parts(int n) { return n > 0 ? (int)eap::cdiv(n, PN_GROUP) : 0; }

extern "C" int eap_pointnet_max_fwd_f32(int b, int c, int o, int n, int na, const float *feats, const float *xyz, const float *centre,
                                        const float *member, const float *wt, const float *v, const float *bias, float *pval,
                                        int32_t *parg, float *out, int32_t *arg, eap_stream_t stream) {
    if (b <= 0) return 0;
    if (int e = pointnet_dims("pointnet_max_fwd", c, o, n, na)) return e;
    if (int e = pointnet_null("pointnet_max_fwd", "feats, xyz, centre, wt, v, pval, parg, out, arg", {feats, xyz, centre, wt, v, pval, parg, out, arg})) return e;
    const int parts = eap_pointnet_max_parts(n);
    const long long gx = eap::cdiv(o, PN_OB) * 8 * eap::cdiv((long long)parts * b, 8);      // (cloud, point group) pairs padded to the 8 XCDs
    int e;
#define PN_RUN(NA) eap::run_kernel("pointnet_max_fwd", pointnet_max_kernel<NA>, gx, 1, 1, dim3(PN_THREADS), 0, eap::S(stream), b, c, o, n, na, parts, feats, \
                                   xyz, centre, member, wt, v, bias, pval, parg)
    if (na == 60) e = PN_RUN(60);
    else if (na == 40) e = PN_RUN(40);
    else if (na == 20) e = PN_RUN(20);
    else if (na == 12) e = PN_RUN(12);
    else e = PN_RUN(0);
#undef PN_RUN
    if (e) return e;
    const long long total = (long long)b * o * na;
    e = eap::run_kernel("pointnet_max_fwd (fold)", pointnet_max_fold_kernel, eap::cdiv(total, 256), 1, 1, dim3(256), 0, eap::S(stream), total, o * na, parts,
                        pval, parg, out, arg);
    if (!e) eap::set_kernel(na == 60 ? "pointnet_max_kernel<60>" : na == 40 ? "pointnet_max_kernel<40>" : na == 20 ? "pointnet_max_kernel<20>" : na == 12 ? "pointnet_max_kernel<12>" : "pointnet_max_kernel<0>");
    return e;
}

extern "C" int eap_pointnet_max_bwd_data_f32(int b, int c, int o, int n, int na, const float *g, const int32_t *arg, const float *w, int ldw,
                                             float *dfeats, float *dcoords, eap_stream_t stream) {
    if (b <= 0) return 0;
    if (int e = pointnet_dims("pointnet_max_bwd_data", c, o, n, na)) return e;
    if (ldw < c + 3) return eap::bad_arg("pointnet_max_bwd_data: ldw (row pitch of w) must be at least c + 3");
    if (int e = pointnet_null("pointnet_max_bwd_data", "g, arg, w", {g, arg, w})) return e;
    if (!dfeats && !dcoords) return eap::bad_arg("pointnet_max_bwd_data: dfeats and dcoords are both null");
    return eap::run_kernel("pointnet_max_bwd_data", pointnet_max_bwd_data_kernel, na, b, 1, dim3(256), 0, eap::S(stream), c, o, n, na, g, arg, w, ldw, dfeats,
                           dcoords);
}

extern "C" int eap_pointnet_max_bwd_weight_f32(int b, int c, int o, int n, int na, const float *g, const int32_t *arg, const float *feats,
                                               const float *xyz, const float *centre, const float *anchors, float *dwp, eap_stream_t stream) {
    if (b <= 0) return 0;
    if (int e = pointnet_dims("pointnet_max_bwd_weight", c, o, n, na)) return e;
    if (int e = pointnet_null("pointnet_max_bwd_weight", "g, arg, feats, xyz, centre, anchors, dwp", {g, arg, feats, xyz, centre, anchors, dwp})) return e;
    return eap::run_kernel("pointnet_max_bwd_weight", pointnet_max_bwd_weight_kernel, o, b, 1, dim3(256), 0, eap::S(stream), c, o, n, na, g, arg, feats, xyz,
                           centre, anchors, dwp);
}
