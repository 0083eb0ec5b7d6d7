// csrc/common.h -- host-side helpers shared by the launchers behind include/eap_hip.h, in three parts: error / launch
// helpers, the side-stream helpers, the cross-file launcher prototypes.  (Device-side primitives: csrc/device_prims.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/eap_hip.h"

namespace eap {

// ---- 1. error / launch helpers --------------------------------------------------------------------------------------
void set_error(const char *msg);
// name (with template arguments, as rocprofv3 prints it) of the dominant kernel the calling thread launched last -- set by
// the launchers of the hot kernels, read by bench.py through eap_last_kernel() to attribute time per KERNEL, not per entry
void set_kernel(const char *name);

static inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
        set_error(buf);
        return (int)e;
    }
    return 0;
}

static inline int bad_arg(const char *what) {
    set_error(what);
    return (int)hipErrorInvalidValue;
}

static inline int hip_fail(hipError_t e, const char *what) {
    if (e == hipSuccess) return 0;
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    set_error(buf);
    return (int)e;
}

static inline hipStream_t S(eap_stream_t s) { return (hipStream_t)s; }

static inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// Row slots of a cloud with n_rows referenced rows in a batch of rp slots, in whole 16-row groups (csrc/so3_dense.hip: the dense index keeps
// 16 row slots together): where the trimmed backward product ends, and the anchor pitch of PACKED Z -- column (a, r) of the cloud at
// a live16 + r, its na live16 live columns one prefix of the row.  0 for a cloud without rows.
__host__ __device__ static inline int live16(int n_rows, int rp) {
    const int n = n_rows < rp ? n_rows : rp;
    return n > 0 ? (n + 15) & ~15 : 0;
}

// true when every pointer is 16-byte aligned: the predicate of a kernel lists exactly the operands it touches with 16-byte
// instructions (a contiguous tensor view may start at any 4-byte offset of its storage)
template <typename... P>
static inline bool aligned16(const P *...p) { return ((reinterpret_cast<uintptr_t>(p) | ... | (uintptr_t)0) & 15) == 0; }

// The launch limits, without a HIP call: every grid and block dimension >= 1, at most 1024 threads per block, gx * block.x < 2^32
// (hip_runtime_api.h at the launch functions: "HIP does not support kernel launch with total work items defined in dimension with
// size gridDim x blockDim >= 2^32"), gy and gz <= 65535.  -> 0 and *grid, or bad_arg with the sizes in the message.
static inline int launch_dims(const char *what, long long gx, long long gy, long long gz, dim3 block, dim3 *grid) {
    const bool block_ok = block.x >= 1 && block.y >= 1 && block.z >= 1 && block.x <= 1024 && block.y <= 1024 && block.z <= 1024 &&
                          block.x * block.y * block.z <= 1024;
    if (!block_ok || gx < 1 || gy < 1 || gz < 1 || gx > 0xffffffffLL / block.x || gy > 65535 || gz > 65535) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s: grid (%lld, %lld, %lld) x block (%u, %u, %u) is outside the launch limits: every size >= 1, block <= 1024 "
                 "threads, grid.x * block.x < 2^32, grid.y and grid.z <= 65535", what, gx, gy, gz, block.x, block.y, block.z);
        return bad_arg(buf);
    }
    *grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
    return 0;
}

// The opt-in a kernel needs before it is launched with `bytes` of dynamic LDS, made once per kernel and device and again only for a
// larger request: the largest size set so far per (kernel, device id) in an open-addressed table, lock-free.  A size is published
// only after hipFuncSetAttribute succeeded; a publisher that finds the entry changed under it sets the larger of the two again, so
// the table never promises more than the attribute holds once the calls have returned.  (Two host threads that launch ONE kernel
// on ONE device with DIFFERENT sizes at the same moment can still see the smaller attribute for an instant; the launch is then
// refused by the runtime, an error.  Entries are meant to be called from one host thread per device, see SideJoin.)
struct LdsOptIn {
    std::atomic<const void *> kernel{nullptr};
    std::atomic<unsigned> bytes[64] = {};
};
inline LdsOptIn g_lds_opt_in[256];

static inline int allow_dynamic_lds(const void *kernel, size_t bytes, const char *what) {
    int dev = 0;
    if (int e = hip_fail(hipGetDevice(&dev), what)) return e;
    std::atomic<unsigned> *seen = nullptr;        // (stays null past 64 devices or 256 kernels: the attribute is then set every time)
    for (size_t i = 0, h = reinterpret_cast<uintptr_t>(kernel) >> 4; i < 256 && dev >= 0 && dev < 64; ++i) {
        LdsOptIn &slot = g_lds_opt_in[(h + i) & 255];
        const void *k = slot.kernel.load(std::memory_order_acquire);
        if (k == nullptr && slot.kernel.compare_exchange_strong(k, kernel, std::memory_order_acq_rel)) k = kernel;
        if (k == kernel) { seen = &slot.bytes[dev]; break; }
    }
    unsigned have = seen ? seen->load(std::memory_order_acquire) : 0u;
    if (have >= bytes) return 0;
    for (;;) {
        if (int e = hip_fail(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), what)) return e;
        if (!seen || seen->compare_exchange_strong(have, (unsigned)bytes, std::memory_order_acq_rel)) return 0;
        if (have > bytes) bytes = have;           // published meanwhile, before or after our call: the larger of the two, once more
    }
}

// Every kernel launch of the library: the limits above, the dynamic-LDS opt-in, the launch, the runtime's verdict -- in that order,
// nothing launched past an error
template <typename K, typename... Args>
static inline int run_kernel(const char *what, K kernel, long long gx, long long gy, long long gz, dim3 block, size_t lds_bytes, hipStream_t s,
                             Args... args) {
    dim3 grid;
    if (int e = launch_dims(what, gx, gy, gz, block, &grid)) return e;
    if (lds_bytes)
        if (int e = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), lds_bytes, what)) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
    return check_launch(what);
}

// ---- 2. side-stream helpers -----------------------------------------------------------------------------------------
// csrc/abi.hip: a side stream per device (fork: it waits for `s` so far; join: `s` waits for it)
int side_fork(hipStream_t s, hipStream_t *side);
int side_join(hipStream_t s);
// Joins on EVERY exit path after a fork: an early error return must not leave the side stream reading buffers the caller frees
// once the entry has failed.  (One side stream and one fork / join event pair per device, shared by every caller: entries that
// fork are meant to be called from ONE host thread per device -- the autograd thread of a process that owns the GPU, as the
// reference's extensions are; two host threads forking on the same device would share the events.)
struct SideJoin {
    hipStream_t s;
    bool armed = true;
    explicit SideJoin(hipStream_t stream) : s(stream) {}
    ~SideJoin() { if (armed) side_join(s); }
    int join() { armed = false; return side_join(s); }
};

// ---- 3. cross-file launcher prototypes ------------------------------------------------------------------------------
// csrc/gemm_f32.hip: C[M,N] (leading dimension ldc, mn = M * N) = the sum of `slabs` contiguous partial slabs of `ws`, in slab order
int reduce_slabs(const float *ws, float *C, long long mn, int N, int slabs, long long ldc, hipStream_t s, const char *what);
// csrc/so3_inter_lists.hip: the two-workgroups-per-CU grouping kernel (no anchor permutation)
bool group_lists_supported(int na, int ks);
int group_lists_fwd(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats,
                    const int32_t *idx, const float *gx, const float *rk, const int32_t *nonident, int blocked, float *out,
                    hipStream_t s);
int group_lists_inv(int b, int o, int p, int nn, int na, int gy_pitch, int ks, int rcap, float sigma, const float *gy,
                    const int32_t *rows, const int32_t *off, const int32_t *cnt, const int32_t *ent_p,
                    const float *ent_gx, const float *rk, float *z, hipStream_t s);
// csrc/so3_inter_lists2.hip: the same kernel with two channel tiles per wave sharing one weight evaluation (64-channel
// blocks); group_lists2_preferred: the channel count fills the wider blocks and the variant has not been switched off
// with eap_so3_group_lists_tiles(1)
bool group_lists2_preferred(int c, int na, int ks, int layout);
int group_lists2_fwd(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats,
                     const int32_t *idx, const float *gx, const float *rk, const int32_t *nonident, int layout, float *out,
                     hipStream_t s);
int group_lists2_inv(int b, int o, int p, int nn, int na, int gy_pitch, int ks, int rcap, float sigma, const float *gy,
                     const int32_t *rows, const int32_t *off, const int32_t *cnt, const int32_t *ent_p,
                     const float *ent_gx, const float *rk, float *z, hipStream_t s);
// csrc/zpconv_rows.hip: native inter zpconv forward near HBM speed (shared neighbour list per point)
bool inter_zpconv_rows_supported(int np, int nq, int na, int ks, int nn, int c);
// (only_flagged != nullptr: clouds whose flag is zero are left untouched)
int inter_zpconv_rows_fwd(int b, int np, int nq, int na, int ks, int nn, int c, const int32_t *idx, const float *w,
                          const float *feats, float *out, const int32_t *only_flagged, hipStream_t s);
// csrc/zpconv_mfma.hip: the same op on the matrix cores for clouds with one neighbour list per point (skip[b] == 0)
bool inter_zpconv_mfma_supported(int np, int nq, int na, int ks, int nn, int c);
int inter_zpconv_mfma_fwd(int b, int np, int nq, int na, int ks, int nn, int c, const int32_t *idx0, const float *w,
                          const float *feats, const int32_t *skip, float *out, hipStream_t s);
// index pattern check shared by the zpconv forward and backward (csrc/zpconv_mfma.hip), the flag-gated scatter backward
// (csrc/zpconv.hip)
// (idx0 == nullptr: only the comparison)
int zpconv_index_check(int b, int np, int per_point, int nn, const int32_t *idx, int32_t *idx0, float *eid, int32_t *flag, hipStream_t s);
// idx0[b,p,:] = the first (a,k) row of every point's 5-D index (1 MB per cloud): what the matrix kernels walk while the full
// comparison above still streams on the side stream
int zpconv_first_rows(int b, int np, int per_point, int nn, const int32_t *idx, int32_t *idx0, hipStream_t s);
// csrc/zpconv.hip: the flag-gated scatter backward
int inter_zpconv_bwd_flagged(int b, int np, int nq, int na, int ks, int ann, int c, const int32_t *idx, const float *w,
                             const float *grad, float *gfeats, const int32_t *only_flagged, hipStream_t s);
// csrc/so3_inter_mfma.hip with the clouds already served by group_lists_fwd skipped
int group_fwd_perm_lists(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats, const int32_t *idx,
                         const float *gx, const float *rk, const uint8_t *mult, const int32_t *nonident, int blocked, float *out,
                         hipStream_t s);      // csrc/so3_inter_inv.hip; -1 = shape not taken
int group_fwd_mfma(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats,
                   const int32_t *idx, const float *gx, const float *rk, const uint8_t *mult,
                   const int32_t *nonident, int skip_plain, int blocked, float *out, hipStream_t s);

}  // namespace eap
