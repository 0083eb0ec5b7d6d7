// csrc/native_ordered.hip -- the backward of the three native scatter operators as ORDERED sums: no floating-point atomic,
// the same bits every run (twins of gather_bwd_kernel in csrc/gathering.hip and of the two BWD kernels in csrc/zpconv.hip;
// reference: vgtk/vgtk/cuda/gathering_cuda.cpp L45-60, zpconv_cuda.cpp L58-75 and L94-110).
//
// Every term is what the scatter kernels add: the product grad * w rounded once in the operand width (this file is compiled
// with -ffp-contract=off, see the Makefile: the product is never fused into the add), then added to the running sum, which
// starts at zero.  Only the order of the additions is new, and it is fixed:
//   gather  grad_pts[b,c,q]   : j ascending over idx[b,j] == q
//   intra   gfeats[b,c,p,a']  : a ascending, then k ascending, then n ascending over idx[a,n] == a'
//   inter   gfeats[b,c,q,a]   : the entry number (p ks + k) ann + n ascending over idx[b,p,a,k,n] == q
// The gather and the inter op walk inverse lists: rows, offsets and counts from csrc/inv_lists.hip (eap_inv_lists_rows), the entry
// numbers from eap_inv_lists_entries_ws below; the intra op inverts its table (at most 64 x ann entries) in LDS.  Every output element is stored
// exactly once, by the lane that owns it -- zero where nothing names it -- so no memset and no accumulation into the output.
//
// The lists come sorted by length, not by row, so a block that owns a tile of target rows first finds their list slots:
// one pass over rows[cloud, :] (at most 64 KB, L2 resident), the slots of its own tile kept in LDS.
#include "common.h"

namespace {

constexpr int MAX_ROWS = 16384;     // the list builders' limit (the LDS sort of eap_inv_lists_rows)
constexpr int GC = 4;               // gather: channels per thread (one walk of the entry list serves them all)
constexpr int ZQ = 16, ZC = 16;     // inter: target rows x channels of a block
constexpr int PPW = 8;              // intra: points per wave (the block inverts the table once for 4 PPW points)

// slot of every target row of the tile [q0, q0 + tile) in s_slot (-1: nothing names the row); all threads of the block call
__device__ inline void tile_slots(const int32_t *__restrict__ rows, int n, int q0, int tile, int *s_slot) {
    for (int i = threadIdx.x; i < tile; i += blockDim.x) s_slot[i] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int q = rows[i];
        if (q >= q0 && q < q0 + tile) s_slot[q - q0] = i;      // (the referenced rows are distinct: one writer per slot)
    }
    __syncthreads();
}

// [beg, beg + len) of a slot's entries inside a list of `per_cloud` entries (an empty range for slot < 0 or anything outside)
__device__ inline void slot_range(const int32_t *__restrict__ off, const int32_t *__restrict__ cnt, int slot, int per_cloud, int *beg, int *len) {
    *beg = 0;
    *len = 0;
    if (slot < 0) return;
    const int o = off[slot], n = cnt[slot];
    if (o < 0 || o >= per_cloud || n <= 0) return;
    *beg = o;
    *len = min(n, per_cloud - o);
}

// ---------------------------------------------------------------------------------------------
// gather: lane = target row q, GC channels per thread; grid (row tiles, channel groups, clouds)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gather_bwd_ordered_kernel(int c, int n, int m, const T *__restrict__ grad_out,
                                                                 const int32_t *__restrict__ rows, const int32_t *__restrict__ off,
                                                                 const int32_t *__restrict__ cnt, const int32_t *__restrict__ ent,
                                                                 T *__restrict__ grad_pts) {
    __shared__ int s_slot[256];
    const int bi = blockIdx.z, q0 = blockIdx.x * 256, c0 = blockIdx.y * GC;
    tile_slots(rows + (size_t)bi * n, n, q0, 256, s_slot);
    const int q = q0 + threadIdx.x;
    if (q >= n) return;
    int beg, len;
    slot_range(off + (size_t)bi * n, cnt + (size_t)bi * n, s_slot[threadIdx.x], m, &beg, &len);
    const int32_t *el = ent + (size_t)bi * m + beg;
    const T *g = grad_out + ((size_t)bi * c + c0) * m;
    T acc[GC];
#pragma unroll
    for (int cc = 0; cc < GC; ++cc) acc[cc] = 0;
    for (int j = 0; j < len; ++j) {
        const int e = el[j];
        if ((unsigned)e >= (unsigned)m) continue;
#pragma unroll
        for (int cc = 0; cc < GC; ++cc)
            if (c0 + cc < c) acc[cc] += g[(size_t)cc * m + e];
    }
#pragma unroll
    for (int cc = 0; cc < GC; ++cc)
        if (c0 + cc < c) grad_pts[((size_t)bi * c + c0 + cc) * n + q] = acc[cc];
}

// ---------------------------------------------------------------------------------------------
// intra: idx [na_out,ann], w [na_out,ks,ann] are shared by every point.  The block inverts the table once -- s_ent: the
// table positions a * ann + n of every input anchor a', ascending, at [s_off[a'], s_off[a' + 1]) -- and each of its 4 waves
// then serves PPW points of one (cloud, channel): lane = a', a run of equal a walked once per kernel point.  The inversion is a scan
// of the whole table per lane and a serial prefix over na_in, repeated by every block: sized for the small tables the op has (60 x 12).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void intra_zpconv_bwd_ordered_kernel(int np, int na_in, int na_out, int ks, int ann, int c,
                                                                       const int32_t *__restrict__ idx, const T *__restrict__ w,
                                                                       const T *__restrict__ grad, T *__restrict__ gfeats) {
    extern __shared__ int s_mem[];
    const int tab = na_out * ann, t = threadIdx.x;
    int *s_off = s_mem, *s_ent = s_mem + na_in + 1, *s_idx = s_ent + tab;     // s_idx: the table itself, read tab times per lane below
    for (int e = t; e < tab; e += 256) s_idx[e] = idx[e];
    if (t == 0) s_off[0] = 0;
    __syncthreads();
    for (int a2 = t; a2 < na_in; a2 += 256) {
        int found = 0;
        for (int e = 0; e < tab; ++e) found += s_idx[e] == a2;
        s_off[a2 + 1] = found;
    }
    __syncthreads();
    if (t == 0)
        for (int a2 = 1; a2 <= na_in; ++a2) s_off[a2] += s_off[a2 - 1];      // (the total is at most tab: every position has one value)
    __syncthreads();
    for (int a2 = t; a2 < na_in; a2 += 256) {
        int pos = s_off[a2];
        for (int e = 0; e < tab; ++e)
            if (s_idx[e] == a2) s_ent[pos++] = e;
    }
    __syncthreads();

    const int lane = t & 63, wave = t >> 6, ci = blockIdx.y, bn = blockIdx.z;
    const size_t k_stride = (size_t)np * na_out;
    for (int i = 0; i < PPW; ++i) {
        const int p = (blockIdx.x * 4 + wave) * PPW + i;
        if (p >= np) break;                                                  // wave-uniform, no barrier below
        const size_t f_row = (((size_t)bn * c + ci) * np + p) * na_in;        // gfeats row
        const size_t o_row = (((size_t)bn * c + ci) * ks * np + p) * na_out;  // + k*np*na_out
        for (int a2 = lane; a2 < na_in; a2 += 64) {
            T acc = 0;
            int i0 = s_off[a2];
            const int end = s_off[a2 + 1];
            while (i0 < end) {
                const int a = s_ent[i0] / ann;
                int i1 = i0 + 1;
                while (i1 < end && s_ent[i1] / ann == a) ++i1;
                for (int k = 0; k < ks; ++k) {
                    const T g = grad[o_row + (size_t)k * k_stride + a];
                    const T *wk = w + ((size_t)a * (ks - 1) + k) * ann;                  // + table position a * ann + n
                    for (int j = i0; j < i1; ++j) acc += g * wk[s_ent[j]];
                }
                i0 = i1;
            }
            gfeats[f_row + a2] = acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// inter: per (cloud, anchor) the op is the transpose of a gather through an index [np, ks*ann].
//   1. idx [b,np,na,ks*ann] -> idxT [b*na, np, ks*ann]: the anchor axis next to the batch, so that the two list builders see
//      b*na "clouds" of np points with ks*ann neighbours;
//   2. eap_inv_lists_rows (rows, off, cnt) and eap_inv_lists_entries_ws (below) on idxT;
//   3. the walk: block = ZQ target rows x ZC channels of one (cloud, anchor); a thread sums its row's entries in entry order.
//      A lane's grad loads are ks*np*na elements apart from its neighbour's (the channel stride) and follow the list: strided.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void anchor_major_index_kernel(long long total, int np, int na, int run, const int32_t *__restrict__ idx,
                                                                 int32_t *__restrict__ idxT) {
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d >= total) return;
    const int e = (int)(d % run);
    const long long r = d / run;
    const int p = (int)(r % np);
    const long long ba = r / np;
    const int a = (int)(ba % na);
    const long long bi = ba / na;
    idxT[d] = idx[((bi * np + p) * na + a) * run + e];
}

// ---------------------------------------------------------------------------------------------
// eap_inv_lists_entries_ws: the entry numbers of every referenced row, ascending -- what eap_inv_lists_entries (csrc/so3_f64.hip)
// writes -- by a stable counting sort in chunks of ECH entries: per chunk a histogram over the rows, a scan over the chunks that
// turns it into each chunk's first position in every row's list, and one wavefront per chunk that places its entries in entry
// order.  The index is read twice whatever the number of rows; eap_inv_lists_entries reads a cloud's entries twice PER REFERENCED
// ROW, which is fine for the few long lists of the SO(3) backward and 97 of 123 ms for the 60 x 1024 lists of one 1024-point cloud here.
// ---------------------------------------------------------------------------------------------
constexpr int ECH = 8192;          // entries per chunk

// cc[cloud, chunk, q] = how many entries of the chunk name row q
__global__ __launch_bounds__(256) void chunk_count_kernel(int per, int nq, const int32_t *__restrict__ idxT, int32_t *__restrict__ cc) {
    extern __shared__ int s_hist[];
    const int ch = blockIdx.x, cl = blockIdx.y, t = threadIdx.x;
    for (int i = t; i < nq; i += 256) s_hist[i] = 0;
    __syncthreads();
    const int beg = ch * ECH, end = beg + min(ECH, per - beg);
    const int32_t *src = idxT + (size_t)cl * per;
    for (int e = beg + t; e < end; e += 256) {
        const int q = src[e];
        if ((unsigned)q < (unsigned)nq) atomicAdd(&s_hist[q], 1);             // (integer, in LDS)
    }
    __syncthreads();
    int32_t *dst = cc + ((size_t)cl * gridDim.x + ch) * nq;
    for (int i = t; i < nq; i += 256) dst[i] = s_hist[i];
}

// cc[cloud, chunk, q] -> the position, in the cloud's entry list, of the chunk's first entry that names q: the row's offset plus the
// counts of the chunks before it.  One thread per referenced row slot.
__global__ __launch_bounds__(256) void chunk_scan_kernel(int nch, int nq, const int32_t *__restrict__ rows, const int32_t *__restrict__ off,
                                                         int32_t *__restrict__ cc) {
    const int slot = blockIdx.x * 256 + threadIdx.x, cl = blockIdx.y;
    if (slot >= nq) return;
    const int q = rows[(size_t)cl * nq + slot];
    if (q < 0 || q >= nq) return;
    int run = off[(size_t)cl * nq + slot];
    int32_t *col = cc + (size_t)cl * nch * nq + q;
    for (int ch = 0; ch < nch; ++ch) {
        const int here = col[(size_t)ch * nq];
        col[(size_t)ch * nq] = run;
        run += here;
    }
}

// One wavefront per (chunk, cloud) walks the chunk 64 entries at a time: the lanes that name the same row as the first lane not yet
// placed take consecutive positions in lane order (ballot + mbcnt), the row's next position moves past them, until every lane is placed.
__global__ __launch_bounds__(64) void chunk_place_kernel(int per, int nq, const int32_t *__restrict__ idxT, const int32_t *__restrict__ cc,
                                                         int32_t *__restrict__ ent) {
    extern __shared__ int s_next[];                                           // next position of every row
    const int ch = blockIdx.x, cl = blockIdx.y, lane = threadIdx.x;
    const int32_t *first = cc + ((size_t)cl * gridDim.x + ch) * nq;
    for (int i = lane; i < nq; i += 64) s_next[i] = first[i];
    __syncthreads();
    const int beg = ch * ECH, end = beg + min(ECH, per - beg);
    const int32_t *src = idxT + (size_t)cl * per;
    int32_t *dst = ent + (size_t)cl * per;
    for (int i0 = beg; i0 < end; i0 += 64) {                                  // wave-uniform trip count
        const int i = i0 + lane;
        const int q = i < end ? src[i] : -1;
        const bool valid = (unsigned)q < (unsigned)nq;
        unsigned long long todo = __ballot(valid);
        while (todo != 0ull) {                                                // wave-uniform
            const int leader = __ffsll((long long)todo) - 1;
            const int qq = __shfl(q, leader);
            const bool mine = valid && q == qq;
            const unsigned long long group = __ballot(mine);
            const int start = s_next[qq];                                     // (one address: a broadcast read)
            __syncthreads();                                                  // every lane has read before the leader moves it (one wave: cheap)
            if (mine) {
                const int pos = start + __builtin_amdgcn_mbcnt_hi((unsigned)(group >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)group, 0));
                if (pos >= 0 && pos < per) dst[pos] = i;
            }
            if (lane == leader) s_next[qq] = start + __popcll(group);
            __syncthreads();
            todo &= ~group;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(ZQ * ZC) void inter_zpconv_bwd_ordered_kernel(int np, int nq, int na, int ks, int ann, int c,
                                                                           const T *__restrict__ w, const T *__restrict__ grad,
                                                                           const int32_t *__restrict__ rows, const int32_t *__restrict__ off,
                                                                           const int32_t *__restrict__ cnt, const int32_t *__restrict__ ent,
                                                                           T *__restrict__ gfeats) {
    __shared__ int s_slot[ZQ];
    const int ba = blockIdx.z, bi = ba / na, a = ba - bi * na, q0 = blockIdx.x * ZQ;
    tile_slots(rows + (size_t)ba * nq, nq, q0, ZQ, s_slot);
    const int cx = threadIdx.x % ZC, qy = threadIdx.x / ZC;
    const int q = q0 + qy, ci = blockIdx.y * ZC + cx;
    if (q >= nq || ci >= c) return;
    const int run = ks * ann, per = np * run;                                 // (per < 2^31: launcher)
    int beg, len;
    slot_range(off + (size_t)ba * nq, cnt + (size_t)ba * nq, s_slot[qy], per, &beg, &len);
    const int32_t *el = ent + (size_t)ba * per + beg;
    const T *gb = grad + ((size_t)bi * c + ci) * ks * np * na + a;           // + (k*np + p)*na
    const T *wb = w + ((size_t)bi * np * na + a) * run;                      // + p*na*run + k*ann + n
    T acc = 0;
    for (int j = 0; j < len; ++j) {
        const int e = el[j];
        if ((unsigned)e >= (unsigned)per) continue;
        const int p = e / run, r = e - p * run, k = r / ann;
        acc += gb[((size_t)k * np + p) * na] * wb[(size_t)p * na * run + r];
    }
    gfeats[(((size_t)bi * c + ci) * nq + q) * na + a] = acc;
}

// Workspace of the inter op, every chunk on a 256-byte boundary:
//   idxT [b*na, np*ks*ann] | ent [b*na, np*ks*ann] | counts, rows, off, cnt [b*na, nq] | n_rows [b*na] | cc [b*na, chunks, nq]
struct InterWorkspace {
    int64_t idxT, ent, counts, rows, off, cnt, n_rows, cc, total;
    InterWorkspace(int b, int np, int nq, int na, int ks, int ann) {
        const int64_t clouds = (int64_t)b * na, entries = clouds * np * ks * ann;
        int64_t at = 0;
        auto take = [&](int64_t bytes) { const int64_t r = at; at += (bytes + 255) / 256 * 256; return r; };
        idxT = take(4 * entries);
        ent = take(4 * entries);
        counts = take(4 * clouds * nq);
        rows = take(4 * clouds * nq);
        off = take(4 * clouds * nq);
        cnt = take(4 * clouds * nq);
        n_rows = take(4 * clouds);
        cc = take(eap_inv_lists_entries_workspace((int)clouds, np, nq, ks * ann));
        total = at;
    }
};

template <typename T>
int gather_ordered(int b, int c, int n, int m, const T *grad_out, const int32_t *rows, const int32_t *off, const int32_t *cnt,
                   const int32_t *ent, T *grad_pts, hipStream_t s) {
    if (b <= 0 || c <= 0 || n <= 0) return 0;
    if (n > MAX_ROWS) return eap::bad_arg("gather_points_bwd_ordered: more than 16384 target rows per cloud (the inverse lists)");
    // nothing gathered: the list builders write nothing either, the gradient is all zeros
    if (m <= 0) return eap::hip_fail(hipMemsetAsync(grad_pts, 0, sizeof(T) * (size_t)b * c * n, s), "gather_points_bwd_ordered memset");
    const int e = eap::run_kernel("gather_points_bwd_ordered", gather_bwd_ordered_kernel<T>, eap::cdiv(n, 256), eap::cdiv(c, GC), b, dim3(256), 0, s, c, n, m,
                                  grad_out, rows, off, cnt, ent, grad_pts);
    if (!e) eap::set_kernel("gather_points_bwd_ordered");
    return e;
}

template <typename T>
int intra_ordered(int b, int np, int na_in, int na_out, int ks, int ann, int c, const int32_t *idx, const T *w, const T *grad, T *gfeats,
                  hipStream_t s) {
    if (b <= 0 || c <= 0 || np <= 0 || na_in <= 0) return 0;
    if (na_in > MAX_ROWS) return eap::bad_arg("intra_zpconv_bwd_ordered: more than 16384 target rows (input anchors)");
    if (na_out > 64) return eap::bad_arg("intra_zpconv_bwd_ordered: at most 64 output anchors are supported");
    if (ks <= 0 || na_out <= 0 || ann <= 0)
        return eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(T) * (size_t)b * c * np * na_in, s), "intra_zpconv_bwd_ordered memset");
    const size_t shmem = sizeof(int) * ((size_t)na_in + 1 + 2 * (size_t)na_out * ann);
    if (shmem > 64 * 1024) return eap::bad_arg("intra_zpconv_bwd_ordered: the inverted table does not fit 64 KB of LDS");
    const int e = eap::run_kernel("intra_zpconv_bwd_ordered", intra_zpconv_bwd_ordered_kernel<T>, eap::cdiv(np, 4 * PPW), c, b, dim3(256), shmem, s, np, na_in,
                                  na_out, ks, ann, c, idx, w, grad, gfeats);
    if (!e) eap::set_kernel("intra_zpconv_bwd_ordered");
    return e;
}

template <typename T>
int inter_ordered(int b, int np, int nq, int na, int ks, int ann, int c, const int32_t *idx, const T *w, const T *grad, T *gfeats,
                  void *workspace, eap_stream_t stream) {
    if (b <= 0 || c <= 0 || nq <= 0 || na <= 0) return 0;
    if (nq > MAX_ROWS) return eap::bad_arg("inter_zpconv_bwd_ordered: more than 16384 target rows per cloud (the inverse lists)");
    hipStream_t s = eap::S(stream);
    if (np <= 0 || ks <= 0 || ann <= 0)
        return eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(T) * (size_t)b * c * nq * na, s), "inter_zpconv_bwd_ordered memset");
    if ((long long)np * ks * ann >= (1ll << 31)) return eap::bad_arg("inter_zpconv_bwd_ordered: more than 2^31 entries per (cloud, anchor)");
    if ((long long)b * na > 65535) return eap::bad_arg("inter_zpconv_bwd_ordered: more than 65535 (cloud, anchor) pairs per call -- split the batch");
    if (workspace == nullptr) return eap::bad_arg("inter_zpconv_bwd_ordered: needs its workspace (eap_inter_zpconv_bwd_ordered_workspace bytes)");
    const InterWorkspace L(b, np, nq, na, ks, ann);
    char *wsb = reinterpret_cast<char *>(workspace);
    int32_t *idxT = reinterpret_cast<int32_t *>(wsb + L.idxT), *ent = reinterpret_cast<int32_t *>(wsb + L.ent);
    int32_t *counts = reinterpret_cast<int32_t *>(wsb + L.counts), *rows = reinterpret_cast<int32_t *>(wsb + L.rows);
    int32_t *off = reinterpret_cast<int32_t *>(wsb + L.off), *cnt = reinterpret_cast<int32_t *>(wsb + L.cnt);
    int32_t *n_rows = reinterpret_cast<int32_t *>(wsb + L.n_rows);
    const int run = ks * ann, clouds = b * na;
    const long long total = (long long)clouds * np * run;
    int e = eap::run_kernel("inter_zpconv_bwd_ordered (index)", anchor_major_index_kernel, eap::cdiv(total, 256), 1, 1, dim3(256), 0, s, total, np, na, run, idx,
                            idxT);
    if (e) return e;
    e = eap_inv_lists_rows(clouds, np, nq, run, idxT, counts, rows, off, cnt, n_rows, stream);
    if (e) return e;
    e = eap_inv_lists_entries_ws(clouds, np, nq, run, idxT, rows, off, ent, wsb + L.cc, stream);
    if (e) return e;
    e = eap::run_kernel("inter_zpconv_bwd_ordered", inter_zpconv_bwd_ordered_kernel<T>, eap::cdiv(nq, ZQ), eap::cdiv(c, ZC), clouds, dim3(ZQ * ZC), 0, s, np, nq, na,
                        ks, ann, c, w, grad, rows, off, cnt, ent, gfeats);
    if (!e) eap::set_kernel("zpconv_bwd_ordered");
    return e;
}

}  // namespace

extern "C" int64_t eap_inv_lists_entries_workspace(int b, int p, int n, int nn) {
    if (b <= 0 || p <= 0 || n <= 0 || nn <= 0) return 256;
    const int64_t chunks = ((int64_t)p * nn + ECH - 1) / ECH;
    return (4 * (int64_t)b * chunks * n + 255) / 256 * 256;
}

extern "C" int eap_inv_lists_entries_ws(int b, int p, int n, int nn, const int32_t *idx, const int32_t *rows, const int32_t *off, int32_t *ent,
                                        void *workspace, eap_stream_t stream) {
    if (b <= 0 || p <= 0 || nn <= 0 || n <= 0) return 0;
    if (n > MAX_ROWS) return eap::bad_arg("inv_lists_entries_ws: more than 16384 support points per cloud");
    if ((long long)p * nn >= (1ll << 31)) return eap::bad_arg("inv_lists_entries_ws: more than 2^31 entries per cloud");
    if (workspace == nullptr) return eap::bad_arg("inv_lists_entries_ws: needs its workspace (eap_inv_lists_entries_workspace bytes)");
    hipStream_t s = eap::S(stream);
    int32_t *cc = reinterpret_cast<int32_t *>(workspace);
    const int per = p * nn, nch = (int)(((long long)per + ECH - 1) / ECH);
    int e = eap::run_kernel("inv_lists_entries_ws (chunk counts)", chunk_count_kernel, nch, b, 1, dim3(256), sizeof(int) * n, s, per, n, idx, cc);
    if (e) return e;
    e = eap::run_kernel("inv_lists_entries_ws (chunk scan)", chunk_scan_kernel, eap::cdiv(n, 256), b, 1, dim3(256), 0, s, nch, n, rows, off, cc);
    if (e) return e;
    e = eap::run_kernel("inv_lists_entries_ws (placement)", chunk_place_kernel, nch, b, 1, dim3(64), sizeof(int) * n, s, per, n, idx, cc, ent);
    if (!e) eap::set_kernel("chunk_place_kernel");
    return e;
}

#define EAP_GATHER_ORDERED(NAME, T)                                                                                             \
    extern "C" int NAME(int b, int c, int n, int m, const T *grad_out, const int32_t *rows, const int32_t *off, const int32_t *cnt, \
                        const int32_t *ent, T *grad_pts, eap_stream_t stream) {                                                  \
        return gather_ordered<T>(b, c, n, m, grad_out, rows, off, cnt, ent, grad_pts, eap::S(stream));                          \
    }
EAP_GATHER_ORDERED(eap_gather_points_bwd_ordered_f32, float)
EAP_GATHER_ORDERED(eap_gather_points_bwd_ordered_f64, double)

#define EAP_INTRA_ORDERED(NAME, T)                                                                                              \
    extern "C" int NAME(int b, int np, int na_in, int na_out, int ks, int ann, int c, const int32_t *idx, const T *w, const T *grad, \
                        T *gfeats, eap_stream_t stream) {                                                                        \
        return intra_ordered<T>(b, np, na_in, na_out, ks, ann, c, idx, w, grad, gfeats, eap::S(stream));                        \
    }
EAP_INTRA_ORDERED(eap_intra_zpconv_bwd_ordered_f32, float)
EAP_INTRA_ORDERED(eap_intra_zpconv_bwd_ordered_f64, double)

extern "C" int64_t eap_inter_zpconv_bwd_ordered_workspace(int b, int np, int nq, int na, int ks, int ann) {
    if (b <= 0 || np <= 0 || nq <= 0 || na <= 0 || ks <= 0 || ann <= 0) return 256;
    return InterWorkspace(b, np, nq, na, ks, ann).total;
}

#define EAP_INTER_ORDERED(NAME, T)                                                                                              \
    extern "C" int NAME(int b, int np, int nq, int na, int ks, int ann, int c, const int32_t *idx, const T *w, const T *grad,   \
                        T *gfeats, void *workspace, eap_stream_t stream) {                                                       \
        return inter_ordered<T>(b, np, nq, na, ks, ann, c, idx, w, grad, gfeats, workspace, stream);                            \
    }
EAP_INTER_ORDERED(eap_inter_zpconv_bwd_ordered_f32, float)
EAP_INTER_ORDERED(eap_inter_zpconv_bwd_ordered_f64, double)
