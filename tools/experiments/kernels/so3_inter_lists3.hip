// csrc/so3_inter_lists3.hip -- the entry-list grouping kernel (csrc/so3_inter_lists2.hip) with its products on the bf16
// matrix cores: fp32 features, fp32 weights, fp32 accumulation, every product formed from exact 3 x bf16 splits of both
// operands (six v_mfma_f32_32x32x16_bf16 per tile, the scheme of csrc/gemm_bf16x3.hip).
//
//   forward   X[b,c,k,p,a]  = sum_n  F[b,c,idx[b,p,n],a]  * w(p,a,k,n)          (vgtk/vgtk/so3conv/functional.py:L1112-1261)
//   backward  Z[b,o,k,r,a]  = sum_{(p,n)->q_r} dY[b,o,p,a] * w(p,a,k,n)         (its autograd transpose over inverse lists)
//   w(p,a,k,n) = relu(1 - |g(p,n) - A_a kappa_k|^2 / sigma)
//
// STATUS: an experiment (eap_so3_group_lists_tiles(3)), correct (tests compare it with the fp32-MFMA kernels) but NOT the
// default: on the deepest layer's backward it runs 43.7 ms against 39.6 ms (34.0 against 36.4 ms with the gathered rows
// resident in L1, profiles/r03_lists3_experiment.txt).  Why it was tried: the fp32-MFMA formulation is at 87 % of a bound of
// 0.552 of the fp32 matrix peak and the bf16 pipe does 16 x the MACs per cycle: with 6 MFMAs per
// fp32-accurate product the matrix time of 16 entries falls from 4096 to 1536 cycles.  Why it does not pay: (1) splitting
// the operands costs 11 vector instructions per pair of values and nothing is shared -- ~340 vector instructions per wave
// and 16 entries, 2 700 cycles per SIMD: the kernel is vector-bound; (2) the grouping gathers 64 KB of feature rows per
// workgroup and 16 entries, i.e. 12 algorithmic flop per byte moved L2 -> LDS: at the fp32 kernel's speed that stream is
// already 6.5 TB/s (13 TB/s of L1 fills, two anchor groups per 128-byte line), and a kernel twice as fast would need more
// than the CUs' L1 fill bandwidth; (3) 128 KB of LDS allow one workgroup per CU, so nothing covers the DMA latency.  x = h + m + l exactly (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m));
// a b ~ ah bh + ah bm + am bh + ah bl + al bh + am bm, the dropped terms below 2^-23 |a b|.
//
// Geometry: workgroup = 8 waves (two per SIMD) = (row run, 64 channels, 16 anchors); wave = 2 anchors x 2 channel tiles
// (64 accumulators); K = 16 entries per MFMA: lane half h contracts entries 8h .. 8h+7 of a 16-entry stage.  LDS image of
// a stage: [16 entries][64 channel rows][4 slots of 16 bytes] (64 KB, two stages), the slot of piece w of row r is
// (w + (r >> 2)) & 3 as in so3_inter_lists2.hip; a wave reads its two anchors as 8 bytes.  One workgroup per CU.
#include "common.h"
#include "device_prims.h"
#include <type_traits>

namespace {

constexpr int CT = 2;         // channel tiles (MFMA M tiles) per wave
constexpr int CB = 32 * CT;   // channels per block
constexpr int NBK = 16;       // entries per LDS stage = K of one bf16 MFMA
constexpr int APW = 2;        // anchors per wave
constexpr int NWV = 8;
constexpr int TM = 64 * NWV;
constexpr int SL = 4;         // 16-byte slots per LDS row (= pieces of a 16-anchor group)
constexpr int GSZ = 4 * SL;   // anchors per workgroup
constexpr int PITCH = 4 * SL; // floats per LDS row
constexpr int NSTD = NBK * CB * SL / TM;   // DMA instructions per thread and stage (8): instruction u carries entries 2u, 2u+1
constexpr unsigned BUF_BYTES = NBK * CB * PITCH * 4;      // 64 KB
static_assert(2 * CB * SL == TM, "one DMA instruction per entry pair: thread t <-> (entry parity t >> 8, row (t >> 2) & 63, slot t & 3)");

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {          // [15:0] = bf16(a), [31:16] = bf16(b), round to nearest even
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned &h, unsigned &m, unsigned &l) {
    h = pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);       // exact
    m = pk_bf16(r0, r1);
    const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);       // exact
    l = pk_bf16(s0, s1);
}
struct Planes { u32x4 h, m, l; };         // 8 values along K as three planes of 8 bf16

// LISTS = true : rows / off / cnt describe variable-length entry lists (backward);
// LISTS = false: row r of cloud b owns entries [ (b*R + r)*nn, +nn ) (forward: its neighbours).
// LAYOUT of the output: 0 = [b,c,k,row,a] (reference), 2 = transposed [row*na+a][c*ks+k]
template <bool LISTS, int LAYOUT>
__global__ __launch_bounds__(TM, 2) void so3_group_lists3_kernel(
    int C, int PF, int na, int fpitch, int ks, int R, int nn, int ent_stride, int AG, int RPB, float inv_sigma,
    const float *__restrict__ F, const int32_t *__restrict__ rows, const int32_t *__restrict__ off,
    const int32_t *__restrict__ cnt, const int32_t *__restrict__ ent_p, const float4 *__restrict__ ent_gx,
    const float *__restrict__ rk, const int32_t *__restrict__ nonident, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    // ---- block -> (row run, anchor group, channel slice, cloud), as csrc/so3_inter_lists2.hip ----
    const int nrun = (R + RPB - 1) / RPB;
    const int ny = gridDim.y, nsl = ny * gridDim.z, per_slice = nrun * AG;
    int qd = blockIdx.x, sl = blockIdx.y + ny * blockIdx.z;
    if ((nsl & 7) == 0) {
        const unsigned lin = blockIdx.x + (unsigned)per_slice * (blockIdx.y + (unsigned)ny * blockIdx.z);
        const unsigned j = lin >> 3;
        sl = (int)((lin & 7u) + 8u * (j / (unsigned)per_slice));
        qd = (int)(j % (unsigned)per_slice);
    } else {
        qd = xcd_point(blockIdx.x, per_slice);
    }
    const int run = qd / AG, ag = qd - run * AG;
    const int r_begin = run * RPB, rows_blk = min(RPB, R - r_begin);
    const int cy = sl % ny, bi = sl / ny, c0 = cy * CB;
    if (nonident != nullptr && __builtin_amdgcn_readfirstlane(nonident[bi]) != 0) return;   // permuted cloud: not ours

    const int t = threadIdx.x, lane = t & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lk = lane & 31, lh = lane >> 5;
    const int a0 = ag * GSZ, gcount = min(GSZ, na - a0);      // anchors [a0, a0 + gcount) of this block
    const int npg = gcount >> 2;                               // 16-byte pieces per feature row that exist
    const int al_beg = wave_u * APW;                           // this wave's anchors: half (wave_u & 1) of piece wave_u >> 1
    const bool active = al_beg < gcount;                       // wave-uniform

    float *s_f = reinterpret_cast<float *>(smem);                           // [2][NBK][CB][PITCH]
    float4 *s_g = reinterpret_cast<float4 *>(s_f + 2 * NBK * CB * PITCH);   // [3][NBK] ring
    int *s_p = reinterpret_cast<int *>(s_g + 3 * NBK);                      // [3][NBK] ring

    int n_ent, nchunk_row;
    size_t e0;
    if (LISTS) {
        const int q = rows[(size_t)bi * R + r_begin];
        n_ent = q >= 0 ? cnt[(size_t)bi * R + r_begin] : 0;
        e0 = (size_t)bi * ent_stride + (q >= 0 ? off[(size_t)bi * R + r_begin] : 0);
        nchunk_row = (n_ent + NBK - 1) / NBK;
    } else {
        n_ent = rows_blk * nn;
        e0 = ((size_t)bi * R + r_begin) * nn;
        nchunk_row = (nn + NBK - 1) / NBK;
    }
    const int nchunk = LISTS ? nchunk_row : rows_blk * nchunk_row;

    // ---- per-lane weight constants of this wave's two anchors (k = lane & 31) ----
    f32x2 kxp, kyp, kzp, kcp;
#pragma unroll
    for (int ai = 0; ai < APW; ++ai) {
        const int a = a0 + min(al_beg + ai, gcount - 1);
        const float *r3 = rk + ((size_t)a * ks + min(lk, ks - 1)) * 3;
        const float x = r3[0], y = r3[1], z = r3[2];
        kxp[ai] = 2.f * inv_sigma * x;
        kyp[ai] = 2.f * inv_sigma * y;
        kzp[ai] = 2.f * inv_sigma * z;
        kcp[ai] = lk < ks ? -inv_sigma * (x * x + y * y + z * z) : -1e30f;
    }
    // operand read: the wave's two anchors are 8 bytes of piece wave_u >> 1 of a channel row; tile 1 = rows + 32
    const float2 *fa_lane = reinterpret_cast<const float2 *>(s_f + (size_t)(8 * lh * CB + lk) * PITCH + 4 * (((wave_u >> 1) + (lk >> 2)) & 3) + 2 * (wave_u & 1));
    constexpr int ENT_F2 = CB * PITCH / 2;             // float2s between consecutive entries
    constexpr int TILE_F2 = 32 * PITCH / 2;            // float2s between the two channel tiles of an entry
    constexpr int BUF_F2 = NBK * CB * PITCH / 2;

    f32x16 acc[CT][APW];

    // ---- DMA: instruction u of a stage carries entries 2u and 2u+1; thread t <-> entry parity t >> 8, channel row
    //      (t >> 2) & 63, slot t & 3.  Pieces a smaller anchor group does not have are requested clamped (a duplicate of its
    //      last piece lands in a slot nobody reads): no branch inside the loop ----
    const float *fb = F + ((size_t)bi * C + c0) * PF * fpitch;   // fpitch: floats between consecutive feature rows (>= na)
    const unsigned lds_f = lds_addr(s_f);
    const unsigned row_bytes = (unsigned)fpitch * 4u;
    const int d_row = (t >> 2) & 63, d_piece = ((t & 3) - (d_row >> 2)) & 3, d_par = t >> 8;
    const unsigned dma_off = ((unsigned)(min(c0 + d_row, C - 1) - c0) * (unsigned)PF * (unsigned)fpitch + (unsigned)(a0 + 4 * min(d_piece, npg - 1))) * 4u;
    const unsigned lds_g = lds_addr(s_g), lds_p = lds_addr(s_p);
    auto issue_idx = [&](int j0, int slot) {
        if (wave_u == 0 && lane < NBK) {
            const size_t e = e0 + min(j0 + lane, max(n_ent - 1, 0));
            glds4(ent_p + e, __builtin_amdgcn_readfirstlane(lds_p + (unsigned)slot * NBK * 4u));
            glds16(ent_gx + e, __builtin_amdgcn_readfirstlane(lds_g + (unsigned)slot * NBK * 16u));
        }
    };
    unsigned src_off[NSTD];
    auto prep_rows = [&](int slot) {
#pragma unroll
        for (int u = 0; u < NSTD; ++u) {
            int pe = s_p[slot * NBK + 2 * u + d_par];
            if (!LISTS) pe = (unsigned)pe < (unsigned)PF ? pe : 0;     // shadow row: any valid row, weight 0
            src_off[u] = dma_off + __umul24((unsigned)pe, row_bytes);
        }
    };
    auto issue = [&](int u, int buf) {
        glds16s(fb, src_off[u], __builtin_amdgcn_readfirstlane(lds_f + (unsigned)buf * BUF_BYTES + (unsigned)(u * TM + wave_u * 64) * 16u));
    };

    if (nchunk > 0) {
        issue_idx(0, 0);
        issue_idx(NBK, 1);
        dma_wait();
        __syncthreads();
        prep_rows(0);
#pragma unroll
        for (int u = 0; u < NSTD; ++u) issue(u, 0);
        dma_wait();
    }
    __syncthreads();

    // per stage: lane e (mod 16) evaluates the per-entry term 1 - |g_e|^2/s of the stage's entry e, or a dead value for
    // entries past the end of the list and for the forward's shadow rows; every lane fetches its eight by bpermute
    auto chunk_bases = [&](int ch, int gslot) {
        const int e = lane & (NBK - 1);
        const float4 g = s_g[gslot * NBK + e];
        float b = 1.0f - inv_sigma * (g.x * g.x + g.y * g.y + g.z * g.z);
        bool dead = ch * NBK + e >= n_ent;
        if (!LISTS) dead = dead || (unsigned)s_p[gslot * NBK + e] >= (unsigned)PF;
        return __float_as_int(dead ? -1e30f : b);
    };

    // Row end: accumulators straight to global memory.  D[i = channel][j = kernel point] sits as col = lane&31,
    // row = (r&3) + 8*(r>>2) + 4*(lane>>5).
    const size_t o_ks = (size_t)R * na, o_cs = (size_t)ks * R * na;
    float *ob = out + (size_t)bi * C * o_cs + (size_t)c0 * o_cs + a0;
    const unsigned lane_off = (unsigned)((size_t)(4 * lh) * o_cs + (size_t)min(lk, ks - 1) * o_ks) + (unsigned)al_beg;
    float *obb = out + (size_t)bi * C * o_cs;
    auto store_row = [&](int row) {
        if (active && lk < ks) {
            if (LAYOUT == 2) {
                const size_t CK = (size_t)C * ks;
                float *rb = obb + ((size_t)row * na + a0 + al_beg) * CK + (size_t)c0 * ks;      // uniform
                const unsigned lo_b = (unsigned)((4 * lh) * ks + lk) * 4u;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (c0 + 32 * ct + 32 <= C || c0 + 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * lh < C) {
#pragma unroll
                            for (int ai = 0; ai < APW; ++ai)
                                *reinterpret_cast<float *>(reinterpret_cast<char *>(rb + (size_t)ai * CK + (size_t)(32 * ct + (r & 3) + 8 * (r >> 2)) * ks) + lo_b) = acc[ct][ai][r];
                        }
            } else {
                float *rb = ob + (size_t)row * na;             // uniform
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (c0 + 32 * ct + 32 <= C || c0 + 32 * ct + (r & 3) + 8 * (r >> 2) + 4 * lh < C)
                            *reinterpret_cast<float2 *>(rb + (size_t)(32 * ct + (r & 3) + 8 * (r >> 2)) * o_cs + lane_off) = make_float2(acc[ct][0][r], acc[ct][1][r]);
            }
        }
    };

    int g0 = 0, g1 = 1, g2 = 2;                           // ring slots of stages ch, ch+1, ch+2
    int ch_row = 0, row = r_begin;
    if (active) {
        for (int ch = 0; ch < nchunk; ++ch) {
            const int buf = ch & 1, nb = buf ^ 1;
            const float2 *fbuf = fa_lane + buf * BUF_F2;
            const int bases = chunk_bases(ch, g0);
            prep_rows(g1);
            issue_idx((ch + 2) * NBK, g2);
            // ---- B operand: the weights of this lane's kernel point for its 8 entries and the wave's two anchors ----
            f32x2 wv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 g = s_g[g0 * NBK + 8 * lh + i];
                const float bk = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (8 * lh + i), bases));
                f32x2 x = __builtin_elementwise_fma((f32x2){g.x, g.x}, kxp, kcp + (f32x2){bk, bk});
                x = __builtin_elementwise_fma((f32x2){g.y, g.y}, kyp, x);
                asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] clamp" : "=v"(wv[i]) : "v"((f32x2){g.z, g.w}), "v"(kzp), "v"(x));
            }
            Planes B[APW];
#pragma unroll
            for (int ai = 0; ai < APW; ++ai) {
                unsigned h[4], m[4], l[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) split_pair(wv[2 * j][ai], wv[2 * j + 1][ai], h[j], m[j], l[j]);
                B[ai].h = (u32x4){h[0], h[1], h[2], h[3]};
                B[ai].m = (u32x4){m[0], m[1], m[2], m[3]};
                B[ai].l = (u32x4){l[0], l[1], l[2], l[3]};
            }
            issue(0, nb);
            issue(1, nb);
            // ---- per channel tile: A operand (8 entries of this lane's channel row, two anchors), then 12 MFMAs ----
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                float2 fv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) fv[i] = fbuf[i * ENT_F2 + ct * TILE_F2];
                Planes A[APW];
#pragma unroll
                for (int ai = 0; ai < APW; ++ai) {
                    unsigned h[4], m[4], l[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        split_pair(ai ? fv[2 * j].y : fv[2 * j].x, ai ? fv[2 * j + 1].y : fv[2 * j + 1].x, h[j], m[j], l[j]);
                    A[ai].h = (u32x4){h[0], h[1], h[2], h[3]};
                    A[ai].m = (u32x4){m[0], m[1], m[2], m[3]};
                    A[ai].l = (u32x4){l[0], l[1], l[2], l[3]};
                }
                issue(2 + 3 * ct, nb);
                issue(3 + 3 * ct, nb);
                issue(4 + 3 * ct, nb);
#define L3_MFMA(AP, BP, CIN) __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A[ai].AP), __builtin_bit_cast(bf16x8, B[ai].BP), CIN, 0, 0, 0)
                if (ch_row == 0) {        // block-uniform: the first stage of a row starts from C = 0 (accumulators are never zeroed)
                    const f32x16 zc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ai = 0; ai < APW; ++ai) acc[ct][ai] = L3_MFMA(h, l, zc);
                } else {
#pragma unroll
                    for (int ai = 0; ai < APW; ++ai) acc[ct][ai] = L3_MFMA(h, l, acc[ct][ai]);
                }
#pragma unroll
                for (int ai = 0; ai < APW; ++ai) acc[ct][ai] = L3_MFMA(l, h, acc[ct][ai]);
#pragma unroll
                for (int ai = 0; ai < APW; ++ai) acc[ct][ai] = L3_MFMA(m, m, acc[ct][ai]);
#pragma unroll
                for (int ai = 0; ai < APW; ++ai) acc[ct][ai] = L3_MFMA(h, m, acc[ct][ai]);
#pragma unroll
                for (int ai = 0; ai < APW; ++ai) acc[ct][ai] = L3_MFMA(m, h, acc[ct][ai]);
#pragma unroll
                for (int ai = 0; ai < APW; ++ai) acc[ct][ai] = L3_MFMA(h, h, acc[ct][ai]);
#undef L3_MFMA
            }
            dma_wait();
            if (++ch_row == nchunk_row) {
                store_row(row);
                ch_row = 0;
                ++row;
            }
            __syncthreads();
            const int gt = g0; g0 = g1; g1 = g2; g2 = gt;
        }
        if (nchunk == 0) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int ai = 0; ai < APW; ++ai)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[ct][ai][r] = 0.f;
            store_row(r_begin);
        }
    } else {
        for (int ch = 0; ch < nchunk; ++ch) {
            prep_rows(g1);
#pragma unroll
            for (int u = 0; u < NSTD; ++u) issue(u, (ch & 1) ^ 1);
            dma_wait();
            __syncthreads();
            const int gt = g0; g0 = g1; g1 = g2; g2 = gt;
        }
    }
}

constexpr size_t SHMEM = 2 * BUF_BYTES + 16 * 3 * NBK + 16 * NBK;

template <bool LISTS>
int launch3(int layout, int b, int C, int PF, int na, int fpitch, int ks, int R, int nn, int ent_stride, float sigma, const float *F,
            const int32_t *rows, const int32_t *off, const int32_t *cnt, const int32_t *ent_p, const float *ent_gx,
            const float *rk, const int32_t *nonident, float *out, hipStream_t s, const char *what) {
    if (fpitch < na || (fpitch & 3) != 0) return eap::bad_arg("so3_group_lists3: the feature row pitch must be a multiple of 4, at least the anchor count");
    if ((long long)CB * PF * fpitch * 4 >= (1ll << 32) || PF >= (1 << 24) || fpitch * 4 >= (1 << 24))
        return eap::bad_arg("so3_group_lists3: 64 feature rows of a cloud exceed the 32-bit request offsets");
    if (((long long)ks * R * na * 4 + 64ll * R * na + 64) * 4 >= (1ll << 31) || (long long)CB * ks * 4 >= (1ll << 31))
        return eap::bad_arg("so3_group_lists3: output rows too far apart for 32-bit store offsets");
    auto kern = layout == 2 ? so3_group_lists3_kernel<LISTS, LISTS ? 0 : 2> : so3_group_lists3_kernel<LISTS, 0>;
    int e = eap::allow_dynamic_lds(kern, SHMEM, what);
    if (e) return e;
    const int AG = (na + GSZ - 1) / GSZ;
    const int RPB = LISTS ? 1 : ((nn % NBK) == 0 ? 8 : 1);
    dim3 grid((R + RPB - 1) / RPB * AG, (C + CB - 1) / CB, b);
    hipLaunchKernelGGL(kern, grid, dim3(TM), SHMEM, s, C, PF, na, fpitch, ks, R, nn, ent_stride, AG, RPB, 1.0f / sigma, F,
                       rows, off, cnt, ent_p, reinterpret_cast<const float4 *>(ent_gx), rk, nonident, out);
    eap::set_kernel(LISTS ? "so3_group_lists3_kernel<true, 0>" : layout == 2 ? "so3_group_lists3_kernel<false, 2>" : "so3_group_lists3_kernel<false, 0>");
    return eap::check_launch(what);
}

}  // namespace

namespace eap {

int group_lists3_fwd(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats,
                     const int32_t *idx, const float *gx, const float *rk, const int32_t *nonident, int layout, float *out,
                     hipStream_t s) {
    return launch3<false>(layout, b, c, n, na, na, ks, p, nn, 0, sigma, feats, nullptr, nullptr, nullptr, idx, gx, rk, nonident, out, s,
                          "so3_inter_group_fwd (lists, 3 x bf16 split)");
}

int group_lists3_inv(int b, int o, int p, int nn, int na, int gy_pitch, int ks, int rcap, float sigma, const float *gy,
                     const int32_t *rows, const int32_t *off, const int32_t *cnt, const int32_t *ent_p,
                     const float *ent_gx, const float *rk, float *z, hipStream_t s) {
    return launch3<true>(0, b, o, p, na, gy_pitch, ks, rcap, nn, p * nn, sigma, gy, rows, off, cnt, ent_p, ent_gx, rk, nullptr, z, s,
                         "so3_inter_group_inv (lists, 3 x bf16 split)");
}

}  // namespace eap
