// csrc/list_probe.hip -- the words the host reads after the first half of a layer's inverse neighbour lists.
//
// vgtk.so3conv.functional._ListHead decides on the host which kernels a layer takes (list kernels or the dense product, the
// product's row slots, whether the norm joins the node).  The numbers it needs come from device tensors -- n_rows and the member
// flags (csrc/inv_lists.hip, csrc/so3_dense.hip), the membership bits, the pose blocks, the norm's parameters -- and were
// formed by some thirty tensor-op launches per layer while the forward waited.  Here they are one entry:
//
//   out[0]  max over clouds of n_rows
//   out[1]  max of nonident (1 when absent)
//   out[2]  dense_bad: max of the member flags (1 without them) + 1 per given pose tensor with a 3x3 block that is not exactly
//           the identity + 1 when a per-cloud 3x3 has max |R R^T - I| > 1e-6 (float64)
//   out[3]  groups16: the non-zero 16-bit halves of a cloud's membership words, the largest cloud, times float32 16/p, truncated
//   out[4]  a norm channel with gamma != 0 and |beta| > ratio |gamma| (0 without a norm)
//
// Three launches: the scratch words zeroed, one grid-wide pass over the membership words and the pose blocks (integer atomics:
// order-independent), one block that folds everything into the five words.
#include "common.h"

namespace {

constexpr int PROBE_THREADS = 256;

// work[0..b) = non-zero halves per cloud, work[b] / work[b + 1] = a block of pose tensor a / b is not the identity
__global__ __launch_bounds__(PROBE_THREADS) void probe_scan_kernel(int b, long long quads_per_cloud, const uint4 *__restrict__ memb,
                                                                   const float4 *__restrict__ rot_a, long long blocks_a,
                                                                   const float4 *__restrict__ rot_b, long long blocks_b,
                                                                   int32_t *__restrict__ work) {
    // grid (column blocks, clouds): a block counts in its own cloud's words; the pose blocks are spread over the whole grid
    const int lane = threadIdx.x & 63, bi = blockIdx.y;
    if (memb != nullptr) {
        const uint4 *src = memb + (long long)bi * quads_per_cloud;
        int mine = 0;
        for (long long i = (long long)blockIdx.x * PROBE_THREADS + threadIdx.x; i < quads_per_cloud; i += (long long)gridDim.x * PROBE_THREADS) {
            const uint4 v = src[i];
            mine += ((v.x & 0xffffu) != 0) + ((v.x >> 16) != 0) + ((v.y & 0xffffu) != 0) + ((v.y >> 16) != 0) +
                    ((v.z & 0xffffu) != 0) + ((v.z >> 16) != 0) + ((v.w & 0xffffu) != 0) + ((v.w >> 16) != 0);
        }
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
        if (lane == 0 && mine) atomicAdd(&work[bi], mine);
    }
    const long long tid = ((long long)bi * gridDim.x + blockIdx.x) * PROBE_THREADS + threadIdx.x;
    const long long nth = (long long)gridDim.x * gridDim.y * PROBE_THREADS;
    // a pose block is 4 x 4 floats, its rotation the upper left 3 x 3; `!(x == 1)`: a NaN is not the identity
    auto off_identity = [](const float4 *blk) {
        const float4 r0 = blk[0], r1 = blk[1], r2 = blk[2];
        return !(r0.x == 1.f) || !(r0.y == 0.f) || !(r0.z == 0.f) || !(r1.x == 0.f) || !(r1.y == 1.f) || !(r1.z == 0.f) ||
               !(r2.x == 0.f) || !(r2.y == 0.f) || !(r2.z == 1.f);
    };
    bool bad_a = false, bad_b = false;
    for (long long i = tid; i < blocks_a; i += nth) bad_a |= off_identity(rot_a + 4 * i);
    for (long long i = tid; i < blocks_b; i += nth) bad_b |= off_identity(rot_b + 4 * i);
    if (__ballot(bad_a) != 0ull && lane == 0) atomicOr(&work[b], 1);
    if (__ballot(bad_b) != 0ull && lane == 0) atomicOr(&work[b + 1], 1);
}

__global__ __launch_bounds__(PROBE_THREADS) void probe_fold_kernel(int b, float per16, const int32_t *__restrict__ n_rows,
                                                                   const int32_t *__restrict__ nonident, const int32_t *__restrict__ dflags,
                                                                   int has_memb, int has_a, int has_b, const float *__restrict__ rot_cloud,
                                                                   const float *__restrict__ norm_w, const float *__restrict__ norm_b,
                                                                   int channels, float ratio, const int32_t *__restrict__ work,
                                                                   int32_t *__restrict__ out) {
    __shared__ int s_rows, s_flag, s_bad, s_touched, s_off, s_nan, s_ill;
    const int t = threadIdx.x;
    if (t == 0) { s_rows = INT32_MIN; s_flag = INT32_MIN; s_bad = INT32_MIN; s_touched = 0; s_off = 0; s_nan = 0; s_ill = 0; }
    __syncthreads();
    for (int bi = t; bi < b; bi += PROBE_THREADS) {
        atomicMax(&s_rows, n_rows[bi]);
        if (nonident != nullptr) atomicMax(&s_flag, nonident[bi]);
        if (dflags != nullptr) atomicMax(&s_bad, dflags[bi]);
        if (has_memb) atomicMax(&s_touched, work[bi]);
        if (rot_cloud != nullptr) {
            // max |R R^T - I| > 1e-6 over ALL clouds' elements, as the maximum of a tensor says it: a NaN anywhere makes the maximum a
            // NaN, which is not above the bar
            const float *r = rot_cloud + 9 * (long long)bi;
            bool off = false, nan = false;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    double s = 0.0;
                    for (int k = 0; k < 3; ++k) s += (double)r[3 * i + k] * (double)r[3 * j + k];
                    const double d = fabs(s - (i == j ? 1.0 : 0.0));
                    off |= d > 1e-6;
                    nan |= d != d;
                }
            if (off) atomicOr(&s_off, 1);
            if (nan) atomicOr(&s_nan, 1);
        }
    }
    if (norm_w != nullptr) {
        bool ill = false;
        for (int c = t; c < channels; c += PROBE_THREADS) ill |= fabsf(norm_b[c]) > ratio * fabsf(norm_w[c]) && norm_w[c] != 0.f;
        if (ill) atomicOr(&s_ill, 1);
    }
    __syncthreads();
    if (t != 0) return;
    out[0] = s_rows;
    out[1] = nonident != nullptr ? s_flag : 1;
    int bad = dflags != nullptr ? s_bad : 1;
    if (has_a) bad += work[b];
    if (has_b) bad += work[b + 1];
    if (rot_cloud != nullptr) bad += (s_off && !s_nan) ? 1 : 0;
    out[2] = bad;
    out[3] = has_memb ? (int)((float)s_touched * per16) : 0;
    out[4] = s_ill;
}

}  // namespace

extern "C" int64_t eap_so3_dense_probe_workspace(int b) { return b > 0 ? (int64_t)b + 2 : 0; }

// memb [b,p,words] (words 16 or 32) with dflags [b], or both null (no dense probe: dense_bad = 1, groups16 = 0); rot_a / rot_b
// [blocks, 4, 4] pose tensors or null; rot_cloud [b,3,3] or null; norm_w / norm_b [channels] or both null;
// work int32 [eap_so3_dense_probe_workspace(b)], out int32 [5]
extern "C" int eap_so3_dense_probe(int b, int p, int words, const int32_t *n_rows, const int32_t *nonident, const int32_t *dflags,
                                   const uint32_t *memb, const float *rot_a, int64_t blocks_a, const float *rot_b, int64_t blocks_b,
                                   const float *rot_cloud, const float *norm_w, const float *norm_b, int channels, float ratio,
                                   int32_t *work, int32_t *out, eap_stream_t stream) {
    if (b <= 0 || p <= 0) return eap::bad_arg("so3_dense_probe: b and p must be positive");
    if (!n_rows || !work || !out) return eap::bad_arg("so3_dense_probe: n_rows, work and out are required");
    if ((memb == nullptr) != (dflags == nullptr)) return eap::bad_arg("so3_dense_probe: the membership words and the member flags come together");
    if (memb != nullptr && words != 16 && words != 32) return eap::bad_arg("so3_dense_probe: 16 or 32 membership words per point");
    if ((norm_w == nullptr) != (norm_b == nullptr) || (norm_w != nullptr && channels <= 0))
        return eap::bad_arg("so3_dense_probe: the norm's weight and bias come together, over at least one channel");
    if ((rot_a != nullptr && blocks_a <= 0) || (rot_b != nullptr && blocks_b <= 0))
        return eap::bad_arg("so3_dense_probe: a pose tensor needs at least one block");
    if (!eap::aligned16(memb, rot_a, rot_b)) return eap::bad_arg("so3_dense_probe: membership words and pose tensors 16-byte aligned");
    hipStream_t s = eap::S(stream);
    if (int e = eap::hip_fail(hipMemsetAsync(work, 0, sizeof(int32_t) * ((size_t)b + 2), s), "so3_dense_probe memset")) return e;
    const long long quads = (long long)p * (memb ? words : 0) / 4;
    const long long na = rot_a ? (long long)blocks_a : 0, nb = rot_b ? (long long)blocks_b : 0;
    // per cloud: its membership quads, its share of the pose blocks; four items per thread, at most 64 blocks per cloud
    const long long pa = eap::cdiv(na, b), pb = eap::cdiv(nb, b);
    const long long widest = quads > pa ? (quads > pb ? quads : pb) : (pa > pb ? pa : pb);
    if (widest > 0) {
        const long long blocks = eap::cdiv(widest, 4 * PROBE_THREADS);
        if (int e = eap::run_kernel("so3_dense_probe (scan)", probe_scan_kernel, blocks < 64 ? blocks : 64, b, 1, dim3(PROBE_THREADS), 0, s, b, quads,
                                    reinterpret_cast<const uint4 *>(memb), reinterpret_cast<const float4 *>(rot_a), na,
                                    reinterpret_cast<const float4 *>(rot_b), nb, work))
            return e;
    }
    const float per16 = (float)(16.0 / (double)p);
    return eap::run_kernel("so3_dense_probe (fold)", probe_fold_kernel, 1, 1, 1, dim3(PROBE_THREADS), 0, s, b, per16, n_rows, nonident, dflags,
                           memb != nullptr ? 1 : 0, rot_a != nullptr ? 1 : 0, rot_b != nullptr ? 1 : 0, rot_cloud, norm_w, norm_b, channels, ratio,
                           (const int32_t *)work, out);
}
