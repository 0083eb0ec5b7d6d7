// csrc/so3_anchor_map.hip -- the per-entry anchor index of the pose-aware inter conv for anchor sets that are NOT a group
// (the 20- and 40-anchor subsets of the icosahedral rotations, so3conv/functional.py:L2641-2649).
//
// Reference (vgtk/vgtk/so3conv/functional.py:L1199-1204):
//   amap[b,p,n,a] = argmax_j tr(R_rel^T A_a A_j^T) = argmax_j <R_rel^T A_a, A_j>_F,     R_rel = R_p R_idx[b,p,n]^T
// For a closed set the search collapses to one nearest-anchor search + a byte table (csrc/so3_inter.hip so3_prep_kernel):
// R_rel^T A_a is then itself (close to) an anchor times a fixed element.  On a subset the product leaves the set, the
// nearest member depends on the actual R_rel, and the map is in general many-to-one -- so it is searched per entry:
// na * (27 + 9 na) FMA.  One entry per lane, the anchors broadcast from LDS (every lane reads the same address), four
// source anchors per pass over the candidates so that a candidate's nine words are loaded once per four traces and the
// four result bytes leave as one dword.
#include "common.h"
#include "device_prims.h"

namespace {

constexpr int AP = 12;   // LDS pitch of one anchor (9 words used): rows stay 16-byte aligned

__global__ __launch_bounds__(256) void so3_anchor_map_kernel(
    int p, int n_sup, int nn, int na, const int32_t *__restrict__ idx, const float *__restrict__ q_pose,
    const float *__restrict__ s_pose, const float *__restrict__ anchors, uint32_t *__restrict__ amap,
    int32_t *__restrict__ nontrivial) {
    __shared__ __attribute__((aligned(16))) float s_anchor[64 * AP];
    for (int i = threadIdx.x; i < na * 9; i += blockDim.x) s_anchor[(i / 9) * AP + i % 9] = anchors[i];
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
    uint32_t *dst = amap + ((size_t)bi * total + e) * (na >> 2);
    bool moved = false;
    for (int aq = 0; aq < (na >> 2); ++aq) {
        float M[4][9];                                  // M_u = R_rel^T A_(4 aq + u)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float *A = s_anchor + (4 * aq + u) * AP;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) M[u][i * 3 + k] = R[0][i] * A[k] + R[1][i] * A[3 + k] + R[2][i] * A[6 + k];
        }
        float best[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
        uint32_t arg[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < na; ++j) {
            const float *B = s_anchor + j * AP;
            const float4 b0 = *reinterpret_cast<const float4 *>(B), b1 = *reinterpret_cast<const float4 *>(B + 4);
            const float b8 = B[8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float t = M[u][0] * b0.x + M[u][1] * b0.y + M[u][2] * b0.z + M[u][3] * b0.w + M[u][4] * b1.x +
                                M[u][5] * b1.y + M[u][6] * b1.z + M[u][7] * b1.w + M[u][8] * b8;
                if (t > best[u]) { best[u] = t; arg[u] = (uint32_t)j; }   // strict: the lowest j wins a tie (torch.argmax)
            }
        }
        const uint32_t word = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
        const uint32_t a0 = 4u * aq;
        moved |= word != (a0 | ((a0 + 1) << 8) | ((a0 + 2) << 16) | ((a0 + 3) << 24));
        if (live) dst[aq] = word;
    }
    // (no lane has left: lane 0 of every wave is there to report)
    if (__any(live && moved) && (threadIdx.x & 63) == 0) atomicOr(nontrivial + bi, 1);
}

}  // namespace

extern "C" int eap_so3_anchor_map_f32(int b, int p, int n, int nn, int na, const int32_t *idx, const float *q_pose,
                                      const float *s_pose, const float *anchors, uint8_t *amap, int32_t *nontrivial,
                                      eap_stream_t stream) {
    if (na <= 0 || na > 64 || na % 4 != 0) return eap::bad_arg("so3_anchor_map: the anchor count must be a multiple of 4, at most 64");
    if (q_pose == nullptr || s_pose == nullptr) return eap::bad_arg("so3_anchor_map: both pose tensors are required");
    if (b <= 0) return 0;
    int e = eap::hip_fail(hipMemsetAsync(nontrivial, 0, sizeof(int32_t) * b, eap::S(stream)), "so3_anchor_map memset");
    if (e || p <= 0 || nn <= 0) return e;
    if (n <= 0) return eap::bad_arg("so3_anchor_map: no support points");
    return eap::run_kernel("so3_anchor_map", so3_anchor_map_kernel, eap::cdiv((long long)p * nn, 256), b, 1, dim3(256), 0, eap::S(stream), p, n, nn, na, idx,
                           q_pose, s_pose, anchors, reinterpret_cast<uint32_t *>(amap), nontrivial);
}
