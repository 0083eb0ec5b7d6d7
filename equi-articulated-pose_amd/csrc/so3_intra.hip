// csrc/so3_intra.hip -- intra-SO(3) (group) convolution, grouping stage
// (vgtk/vgtk/so3conv/functional.py:L2553-2602):
//     out[b,c,t,p,a] = feats[b,c,p,intra_idx[a,t]]
// The reference does index_select + permute + contiguous (two materialised copies); here one
// kernel reads each 4*na-byte feature row once (lanes along the anchor dimension) and writes the
// `t` permuted copies as coalesced rows.  The backward is the deterministic transpose: every
// block first inverts the (tiny) index table in LDS, then each lane sums the rows that read it.
// The 2-D variant (functional.py:L2606-2627) has the anchor axis (na, 4) with the residual innermost and gathers on na alone:
//     out[b,c,t,p,a,r] = feats[b,c,p,intra_idx[a,t],r]
// -- the same two kernels with a 16-byte quad (V = float4) per lane instead of a float: rows are 16*na-byte runs.
#include "common.h"

namespace {

constexpr int ROWS = 4;  // (c,p) rows per block = waves per block

__device__ __forceinline__ void accumulate(float &acc, const float &v) { acc += v; }
__device__ __forceinline__ void accumulate(double &acc, const double &v) { acc += v; }
__device__ __forceinline__ void accumulate(float4 &acc, const float4 &v) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }

// V: what a lane moves per anchor (float, the float4 of an anchor's four residuals, or a double: the float64 regime)
template <typename V>
__global__ __launch_bounds__(64 * ROWS) void so3_intra_group_fwd_kernel(
    long long rows, int c, int p, int na, int t, const V *__restrict__ feats,
    const int32_t *__restrict__ intra_idx, V *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * ROWS + wave;  // over (b,c,p)
    if (row >= rows || lane >= na) return;
    const long long bc = row / p;
    const int pi = (int)(row - bc * p);
    const V *f = feats + row * na;
    V *o = out + (bc * t * p + pi) * na + lane;
    for (int ti = 0; ti < t; ++ti) o[(long long)ti * p * na] = f[intra_idx[lane * t + ti]];
}

template <typename V>
__global__ __launch_bounds__(64 * ROWS) void so3_intra_group_bwd_kernel(
    long long rows, int rows_per_block, int c, int p, int na, int t,
    const V *__restrict__ gout, const int32_t *__restrict__ intra_idx,
    V *__restrict__ gfeats) {
    extern __shared__ int32_t s_tab[];   // [na*t] index | [na+1] offsets | [na*t] CSR of (a*t+ti)
    int32_t *s_idx = s_tab, *s_off = s_tab + na * t, *s_csr = s_off + na + 1;
    const int total = na * t;
    for (int i = threadIdx.x; i < total; i += blockDim.x) s_idx[i] = intra_idx[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        int cnt = 0;
        if (lane < na)
            for (int e = 0; e < total; ++e) cnt += (s_idx[e] == lane);
        int incl = cnt;   // wave-wide inclusive scan
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        if (lane < na) {
            s_off[lane + 1] = incl;
            if (lane == 0) s_off[0] = 0;
            int w = incl - cnt;
            for (int e = 0; e < total; ++e)
                if (s_idx[e] == lane) s_csr[w++] = e;
        }
    }
    __syncthreads();
    if (lane >= na) return;
    const int beg = s_off[lane], end = s_off[lane + 1];
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    for (int r = wave; r < rows_per_block; r += ROWS) {
        const long long row = row0 + r;
        if (row >= rows) break;
        const long long bc = row / p;
        const int pi = (int)(row - bc * p);
        const V *g = gout + (bc * t * p + pi) * na;
        V acc = {};
        for (int j = beg; j < end; ++j) {
            const int e = s_csr[j];
            const int a = e / t, ti = e - a * t;
            accumulate(acc, g[(long long)ti * p * na + a]);
        }
        gfeats[row * na + lane] = acc;
    }
}

template <typename V>
int group_fwd(long long rows, int c, int p, int na, int t, const float *feats, const int32_t *intra_idx, float *out, hipStream_t s, const char *what) {
    return eap::run_kernel(what, so3_intra_group_fwd_kernel<V>, eap::cdiv(rows, ROWS), 1, 1, dim3(64 * ROWS), 0, s, rows, c, p, na, t,
                           reinterpret_cast<const V *>(feats), intra_idx, reinterpret_cast<V *>(out));
}

template <typename V>
int group_bwd(long long rows, int c, int p, int na, int t, const float *gout, const int32_t *intra_idx, float *gfeats, hipStream_t s, const char *what) {
    const int rows_per_block = 64;
    const size_t shmem = sizeof(int32_t) * ((size_t)2 * na * t + na + 1);
    return eap::run_kernel(what, so3_intra_group_bwd_kernel<V>, eap::cdiv(rows, rows_per_block), 1, 1, dim3(64 * ROWS), shmem, s, rows,
                           rows_per_block, c, p, na, t, reinterpret_cast<const V *>(gout), intra_idx, reinterpret_cast<V *>(gfeats));
}

// the limits of the 2-D pair (include/eap_hip.h), checked before a pointer is looked at
const char *group2d_refusal(int na, int nr, int t) {
    if (nr != 4) return "so3_intra_group2d: nr = 4 residuals per anchor (one 16-byte quad)";
    if (na > 64) return "so3_intra_group2d: at most 64 anchors";
    if (t > 16) return "so3_intra_group2d: at most 16 taps";
    return nullptr;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int eap_so3_intra_group_fwd_f32(int b, int c, int p, int na, int t, const float *feats,
                                           const int32_t *intra_idx, float *out, eap_stream_t stream) {
    const long long rows = (long long)b * c * p;
    if (rows <= 0 || t <= 0 || na <= 0) return 0;
    if (na > 64) return eap::bad_arg("so3_intra_group_fwd: at most 64 anchors");
    return group_fwd<float>(rows, c, p, na, t, feats, intra_idx, out, eap::S(stream), "so3_intra_group_fwd");
}

extern "C" int eap_so3_intra_group_bwd_f32(int b, int c, int p, int na, int t, const float *gout,
                                           const int32_t *intra_idx, float *gfeats, eap_stream_t stream) {
    const long long rows = (long long)b * c * p;
    if (rows <= 0 || na <= 0) return 0;
    if (na > 64) return eap::bad_arg("so3_intra_group_bwd: at most 64 anchors");
    if (t <= 0)
        return eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(float) * rows * na, eap::S(stream)), "so3_intra_group_bwd memset");
    return group_bwd<float>(rows, c, p, na, t, gout, intra_idx, gfeats, eap::S(stream), "so3_intra_group_bwd");
}

// the float64 pair (the same kernels at V = double; the launch helpers carry the pointers untyped)
extern "C" int eap_so3_intra_group_fwd_f64(int b, int c, int p, int na, int t, const double *feats, const int32_t *intra_idx, double *out,
                                           eap_stream_t stream) {
    const long long rows = (long long)b * c * p;
    if (rows <= 0 || t <= 0 || na <= 0) return 0;
    if (na > 64) return eap::bad_arg("so3_intra_group_fwd_f64: at most 64 anchors");
    eap::set_kernel("so3_intra_group_fwd_kernel<double>");
    return group_fwd<double>(rows, c, p, na, t, reinterpret_cast<const float *>(feats), intra_idx, reinterpret_cast<float *>(out), eap::S(stream),
                             "so3_intra_group_fwd_f64");
}

extern "C" int eap_so3_intra_group_bwd_f64(int b, int c, int p, int na, int t, const double *gout, const int32_t *intra_idx, double *gfeats,
                                           eap_stream_t stream) {
    const long long rows = (long long)b * c * p;
    if (rows <= 0 || na <= 0) return 0;
    if (na > 64) return eap::bad_arg("so3_intra_group_bwd_f64: at most 64 anchors");
    if (t <= 0)
        return eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(double) * rows * na, eap::S(stream)), "so3_intra_group_bwd_f64 memset");
    eap::set_kernel("so3_intra_group_bwd_kernel<double>");
    return group_bwd<double>(rows, c, p, na, t, reinterpret_cast<const float *>(gout), intra_idx, reinterpret_cast<float *>(gfeats), eap::S(stream),
                             "so3_intra_group_bwd_f64");
}

// intra_so3conv_grouping_2D (so3conv/functional.py:L2606-2627): out[b,c,t,p,a,r] = feats[b,c,p,intra_idx[a,t],r]
extern "C" int eap_so3_intra_group2d_fwd_f32(int b, int c, int p, int na, int nr, int t, const float *feats, const int32_t *intra_idx, float *out,
                                             eap_stream_t stream) {
    const long long rows = (long long)b * c * p;
    if (rows <= 0 || t <= 0 || na <= 0) return 0;
    if (const char *why = group2d_refusal(na, nr, t)) return eap::bad_arg(why);
    if (!aligned16(feats) || !aligned16(out)) return eap::bad_arg("so3_intra_group2d_fwd: feats and out must be 16-byte aligned");
    eap::set_kernel("so3_intra_group_fwd_kernel<float4>");
    return group_fwd<float4>(rows, c, p, na, t, feats, intra_idx, out, eap::S(stream), "so3_intra_group2d_fwd");
}

// its transpose (the autograd of the index_select in functional.py:L2606-2627), summed in table order
extern "C" int eap_so3_intra_group2d_bwd_f32(int b, int c, int p, int na, int nr, int t, const float *gout, const int32_t *intra_idx, float *gfeats,
                                             eap_stream_t stream) {
    const long long rows = (long long)b * c * p;
    if (rows <= 0 || na <= 0) return 0;
    if (const char *why = group2d_refusal(na, nr, t)) return eap::bad_arg(why);
    if (t <= 0)
        return eap::hip_fail(hipMemsetAsync(gfeats, 0, sizeof(float) * rows * na * nr, eap::S(stream)), "so3_intra_group2d_bwd memset");
    if (!aligned16(gout) || !aligned16(gfeats)) return eap::bad_arg("so3_intra_group2d_bwd: gout and gfeats must be 16-byte aligned");
    eap::set_kernel("so3_intra_group_bwd_kernel<float4>");
    return group_bwd<float4>(rows, c, p, na, t, gout, intra_idx, gfeats, eap::S(stream), "so3_intra_group2d_bwd");
}
