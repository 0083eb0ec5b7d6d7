/*
 * include/eap_hip.h -- C ABI of libeap_hip.so, the MI355X (gfx950) implementation of the
 * SE(3)-equivariant point-convolution hot path of Meowuu7/equi-articulated-pose.
 *
 * Drop-in boundary B2: every entry point below replaces one pybind11
 * function of the reference's CUDA extensions (the .cpp files of vgtk/vgtk/cuda and extensions/chamfer_dist)
 * or one stage of the Python "naive" operator path that the shipped models execute
 * (vgtk/vgtk/so3conv/functional.py).  The reference interface each one replaces is cited as
 * file:line (paths relative to /root/reference).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers, tensors are
 *     contiguous in the layout written next to each argument;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); launches are
 *     asynchronous, nothing synchronises;
 *   - outputs are fully written by the call (no pre-zeroing needed) unless stated otherwise;
 *   - return value: 0 on success, otherwise the hipError_t of the failed launch / argument
 *     check (eap_last_error() returns a message).  The reference only printf()s launch errors
 *     (vgtk/vgtk/cuda/zpconv_cuda_kernel.cu:L232-234); this ABI reports them.
 *   - *_f32 / *_f64: the reference dispatches AT_DISPATCH_FLOATING_TYPES for its native ops.
 *
 * Vocabulary.  The Python package reads THIS FILE at import and builds one typed ctypes prototype per `ret eap_name(params);` below
 * (equi-articulated-pose_amd/vgtk/_hip.py, `abi`), so a declaration is plain C over these types and nothing else:
 *   returns      int, int64_t, const char *
 *   scalars      int, int64_t, float
 *   pointers     [const] float / double / int32_t / uint32_t / int64_t / uint64_t / uint8_t / void *
 *   the stream   eap_stream_t
 * with `(void)` for no parameters, no macros, no function pointers, no arrays.  Anything else makes the import fail (ImportError naming
 * the entry and the parameter): extend the table in _hip.py together with the header, never the header alone.
 */
#ifndef EAP_HIP_H
#define EAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *eap_stream_t;

const char *eap_last_error(void);
/* The limits every kernel launch of the library is checked against BEFORE it is made (csrc/common.h, launch_dims): every grid and
 * block size >= 1, at most 1024 threads per block, gx * bx < 2^32, gy and gz <= 65535.  The x rule is HIP's own, stated at the
 * launch functions of hip_runtime_api.h ("HIP does not support kernel launch with total work items defined in dimension with
 * size gridDim x blockDim >= 2^32"); 65535 is the y / z grid limit.  An entry whose shape needs more returns
 * hipErrorInvalidValue with the six sizes in eap_last_error() and launches nothing.  This entry applies the same function to the
 * sizes given, on the host alone: 0, or hipErrorInvalidValue with eap_last_error() set (a negative block size reads as its
 * unsigned value). */
int eap_launch_dims_ok(int64_t gx, int64_t gy, int64_t gz, int bx, int by, int bz);
/* Name, with its template arguments, of the dominant HIP kernel the calling thread's last entry launched ("" when the
 * entry does not record one); reading clears it.  Lets a profiler-less caller (bench.py) attribute launch times to kernels. */
const char *eap_last_kernel(void);
int eap_abi_version(void);

/* ---- grouping (vgtk/vgtk/cuda/grouping_cuda.cpp) ------------------------------------------ */

/* ball_query: grouping_cuda.cpp:L71-86, kernel grouping_cuda_kernel.cu:L68-113.
 * new_xyz [b,3,m], xyz [b,3,n] -> idx int32 [b,m,nsample]: first `nsample` support indices in
 * index order with d2 < radius^2; repeat-padding when fewer than nsample-1 hits. */
int eap_ball_query_f32(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                       const float *xyz, int32_t *idx, eap_stream_t stream);
int eap_ball_query_f64(int b, int n, int m, float radius, int nsample, const double *new_xyz,
                       const double *xyz, int32_t *idx, eap_stream_t stream);

/* furthest_point_sampling: grouping_cuda.cpp:L160-174, kernel .cu:L352-466.
 * xyz [b,3,n] -> idx int32 [b,m]; temp [b,n] is scratch (initialised by the call). */
int eap_furthest_point_sampling_f32(int b, int n, int m, const float *xyz, float *temp,
                                    int32_t *idx, eap_stream_t stream);
/* the double instantiation of grouping_cuda_kernel.cu:L638-726: distances, temp, the 1e10 / -1 start
 * values and the 1e-3 skip threshold in double; same block size and tie rules. */
int eap_furthest_point_sampling_f64(int b, int n, int m, const double *xyz, double *temp,
                                    int32_t *idx, eap_stream_t stream);

/* anchor_query (S^2 variant): grouping_cuda.cpp:L88-108, kernel .cu:L181-247.
 * grouped_xyz [b,3,np,nn], anchors [na,3], kernel_pts [ks,2] -> w [b,np,na,ks,nn]. */
int eap_anchor_query_f32(int b, int np, int nn, int na, int ks, const float *grouped_xyz,
                         const float *anchors, const float *kernel_pts, float *w,
                         eap_stream_t stream);
/* the double dispatch of grouping_cuda_kernel.cu:L510: sqrt, acos and the + 1e-6 in double. */
int eap_anchor_query_f64(int b, int np, int nn, int na, int ks, const double *grouped_xyz,
                         const double *anchors, const double *kernel_pts, double *w,
                         eap_stream_t stream);

/* initial_anchor_query: grouping_cuda.cpp:L138-158, kernel .cu:L117-167.
 * centers [b,3,nc], xyz [m,3], kernel_pts [ks,na,3] -> w, cnt [b,ks,nc,na]. */
int eap_initial_anchor_query_f32(int b, int nc, int m, int na, int ks, float radius, float sigma,
                                 const float *centers, const float *xyz, const float *kernel_pts,
                                 float *w, float *cnt, eap_stream_t stream);
/* the double dispatch of grouping_cuda_kernel.cu:L562: radius and sigma stay float arguments and are
 * widened where they are compared and divided by. */
int eap_initial_anchor_query_f64(int b, int nc, int m, int na, int ks, float radius, float sigma,
                                 const double *centers, const double *xyz, const double *kernel_pts,
                                 double *w, double *cnt, eap_stream_t stream);

/* ---- gathering (vgtk/vgtk/cuda/gathering_cuda.cpp) ---------------------------------------- */

/* gather_points_forward: gathering_cuda.cpp:L29-43. pts [b,c,n], idx [b,m] -> out f32 [b,c,m]. */
int eap_gather_points_fwd_f32(int b, int c, int n, int m, const float *pts, const int32_t *idx,
                              float *out, eap_stream_t stream);
/* the double dispatch of gathering_cuda_kernel.cu:L117: out stays f32 (gathering_cuda.cpp:L38-39),
 * every element converted once, round to nearest even. */
int eap_gather_points_fwd_f64(int b, int c, int n, int m, const double *pts, const int32_t *idx,
                              float *out, eap_stream_t stream);
/* gather_points_backward: gathering_cuda.cpp:L45-60. grad_out [b,c,m] -> grad_pts [b,c,n]. */
int eap_gather_points_bwd_f32(int b, int c, int n, int m, const float *grad_out,
                              const int32_t *idx, float *grad_pts, eap_stream_t stream);
int eap_gather_points_bwd_f64(int b, int c, int n, int m, const double *grad_out,
                              const int32_t *idx, double *grad_pts, eap_stream_t stream);
/* gather_points_backward (gathering_cuda.cpp:L45-60) as an ordered sum: grad_pts[b,c,q] = the grad_out[b,c,j] with idx[b,j] == q
 * added in ascending j, starting from zero.  rows, off, cnt int32 [b,n] = eap_inv_lists_rows and ent int32 [b,m] =
 * eap_inv_lists_entries (or _ws) of idx seen as [b,m,1] (n <= 16384, their limit).  grad_pts is fully written (zeros where nothing names
 * a row); no floating-point atomics, bit-identical run to run.  Regime name: gather_points_bwd_ordered. */
int eap_gather_points_bwd_ordered_f32(int b, int c, int n, int m, const float *grad_out, const int32_t *rows, const int32_t *off,
                                      const int32_t *cnt, const int32_t *ent, float *grad_pts, eap_stream_t stream);
int eap_gather_points_bwd_ordered_f64(int b, int c, int n, int m, const double *grad_out, const int32_t *rows, const int32_t *off,
                                      const int32_t *cnt, const int32_t *ent, double *grad_pts, eap_stream_t stream);

/* ---- zpconv (vgtk/vgtk/cuda/zpconv_cuda.cpp) ---------------------------------------------- */

/* Every zpconv entry names the regime that served the call (eap_last_kernel): zpconv_fwd_matrix, zpconv_fwd_rows,
 * zpconv_fwd_scalar, zp_hot_kernel, zpconv_bwd_products, zpconv_bwd_scatter, intra_zpconv, and the ordered backwards
 * (csrc/native_ordered.hip, taken on request only) zpconv_bwd_ordered and intra_zpconv_bwd_ordered.  Operands may sit at any
 * element-aligned address: a kernel that moves 16-byte words is selected only when every operand it touches that way is
 * 16-byte aligned (rows kernel: idx, w, feats, out; matrix forward: those and the workspace; product pipeline and on-chip
 * backward: idx, grad, gfeats and the workspace -- w is read 4 bytes per lane); the scalar kernels take the rest. */

/* inter_zpconv_forward: zpconv_cuda.cpp:L41-56, kernel zpconv_cuda_kernel.cu:L33-73.
 * idx,w [b,np,na,ks,ann], feats [b,c,nq,na] -> out [b,c,ks,np,na]. */
int eap_inter_zpconv_fwd_f32(int b, int np, int nq, int na, int ks, int ann, int c,
                             const int32_t *idx, const float *w, const float *feats, float *out,
                             eap_stream_t stream);
int eap_inter_zpconv_fwd_f64(int b, int np, int nq, int na, int ks, int ann, int c,
                             const int32_t *idx, const double *w, const double *feats,
                             double *out, eap_stream_t stream);
/* The same op with a scratch buffer of eap_inter_zpconv_fwd_workspace(b, np, ann) BYTES (16-byte aligned): the index is
 * checked on device for the pattern every reference caller produces (one neighbour list per point broadcast over
 * (a,k): spconv/functional.py:L232-249) and those clouds run on the matrix cores (csrc/zpconv_mfma.hip); any other
 * cloud, size or alignment falls through to eap_inter_zpconv_fwd_f32's kernels.  Same results either way. */
int64_t eap_inter_zpconv_fwd_workspace(int b, int np, int ann);
int eap_inter_zpconv_fwd_ws_f32(int b, int np, int nq, int na, int ks, int ann, int c,
                                const int32_t *idx, const float *w, const float *feats, float *out,
                                void *workspace, eap_stream_t stream);
/* inter_zpconv_backward: zpconv_cuda.cpp:L58-75, kernel .cu:L77-116.
 * grad [b,c,ks,np,na] -> gfeats [b,c,nq,na]. */
int eap_inter_zpconv_bwd_f32(int b, int np, int nq, int na, int ks, int ann, int c,
                             const int32_t *idx, const float *w, const float *grad, float *gfeats,
                             eap_stream_t stream);
int eap_inter_zpconv_bwd_f64(int b, int np, int nq, int na, int ks, int ann, int c,
                             const int32_t *idx, const double *w, const double *grad,
                             double *gfeats, eap_stream_t stream);
/* The same op without atomics, with a scratch buffer of eap_inter_zpconv_bwd_workspace(b, np, nq, na, ann, c) BYTES
 * (256-byte aligned; dominated by 4*b*np*na*ann*c for the per-(point, neighbour) products -- split the batch to bound
 * it): for clouds whose index is one neighbour list per point (checked on device) the products are formed in forward
 * order on the matrix cores and summed per support point over device-built inverse lists, in a fixed order
 * (csrc/zpconv_bwd.hip); any other cloud, size or alignment goes through eap_inter_zpconv_bwd_f32's scatter kernel. */
int64_t eap_inter_zpconv_bwd_workspace(int b, int np, int nq, int na, int ann, int c);
int eap_inter_zpconv_bwd_ws_f32(int b, int np, int nq, int na, int ks, int ann, int c,
                                const int32_t *idx, const float *w, const float *grad, float *gfeats,
                                void *workspace, eap_stream_t stream);
/* 1 when eap_inter_zpconv_bwd_ws_f32 serves these sizes with its product pipeline (given 16-byte aligned idx, grad, gfeats and
 * workspace), 0 when it would hand the whole call to the scatter kernel.  Host only. */
int eap_inter_zpconv_bwd_ws_takes(int np, int nq, int na, int ks, int ann, int c);
/* inter_zpconv_backward (zpconv_cuda.cpp:L58-75, kernel .cu:L77-116) as an ordered sum, for ANY 5-D index:
 * gfeats[b,c,q,a] = the products grad[b,c,k,p,a] * w[b,p,a,k,n] with idx[b,p,a,k,n] == q, each rounded once, added in ascending
 * entry number (p*ks + k)*ann + n, starting from zero.  The entry copies the index with the anchor axis next to the batch
 * ([b*na, np, ks*ann]), builds the inverse lists of those b*na "clouds" (eap_inv_lists_rows, eap_inv_lists_entries_ws) and walks
 * them; workspace: eap_inter_zpconv_bwd_ordered_workspace BYTES (about 8*b*na*np*ks*ann, twice the index, plus the list builders'
 * tables; 256-byte aligned) -- split the batch to bound it.  nq <= 16384, b*na <= 65535.  gfeats is fully written; no floating-point atomics, bit-identical run to run.
 * Regime name: zpconv_bwd_ordered. */
int64_t eap_inter_zpconv_bwd_ordered_workspace(int b, int np, int nq, int na, int ks, int ann);
int eap_inter_zpconv_bwd_ordered_f32(int b, int np, int nq, int na, int ks, int ann, int c,
                                     const int32_t *idx, const float *w, const float *grad, float *gfeats,
                                     void *workspace, eap_stream_t stream);
int eap_inter_zpconv_bwd_ordered_f64(int b, int np, int nq, int na, int ks, int ann, int c,
                                     const int32_t *idx, const double *w, const double *grad, double *gfeats,
                                     void *workspace, eap_stream_t stream);
/* The same op (zpconv_cuda.cpp:L58-75) with the scatter target held in LDS -- no per-(point, neighbour) intermediate
 * (csrc/zpconv_bwd_hot.hip): for clouds whose index is one neighbour list per point AND whose lists reference at most
 * eap_inter_zpconv_bwd_hot_rows() distinct support rows (large balls under the reference's first-nsample-in-index-order
 * ball query), every (cloud, anchor quad, 32 channels) accumulates its rows on chip and writes them once; sums in a fixed
 * order, no atomics on global memory.  status[i] (device, int32 [b]) = 0: cloud i done; 1: untouched apart from being
 * zeroed -- hand it to eap_inter_zpconv_bwd_ws_f32.  eap_inter_zpconv_bwd_hot_workspace returns 0 for shapes this
 * path does not take (ks != 24, ann != 64, na or c not multiples of 4 / 32); workspace 256-byte aligned. */
int eap_inter_zpconv_bwd_hot_rows(void);
int64_t eap_inter_zpconv_bwd_hot_workspace(int b, int np, int nq, int na, int ks, int ann, int c);
int eap_inter_zpconv_bwd_hot_f32(int b, int np, int nq, int na, int ks, int ann, int c,
                                 const int32_t *idx, const float *w, const float *grad, float *gfeats,
                                 void *workspace, int32_t *status, eap_stream_t stream);
/* intra_zpconv_forward: zpconv_cuda.cpp:L77-92, kernel .cu:L120-156.
 * idx [na_out,ann], w [na_out,ks,ann], feats [b,c,np,na_in] -> out [b,c,ks,np,na_out]. */
int eap_intra_zpconv_fwd_f32(int b, int np, int na_in, int na_out, int ks, int ann, int c,
                             const int32_t *idx, const float *w, const float *feats, float *out,
                             eap_stream_t stream);
int eap_intra_zpconv_fwd_f64(int b, int np, int na_in, int na_out, int ks, int ann, int c,
                             const int32_t *idx, const double *w, const double *feats,
                             double *out, eap_stream_t stream);
/* intra_zpconv_backward: zpconv_cuda.cpp:L94-110, kernel .cu:L160-195. */
int eap_intra_zpconv_bwd_f32(int b, int np, int na_in, int na_out, int ks, int ann, int c,
                             const int32_t *idx, const float *w, const float *grad, float *gfeats,
                             eap_stream_t stream);
int eap_intra_zpconv_bwd_f64(int b, int np, int na_in, int na_out, int ks, int ann, int c,
                             const int32_t *idx, const double *w, const double *grad,
                             double *gfeats, eap_stream_t stream);
/* intra_zpconv_backward (zpconv_cuda.cpp:L94-110, kernel .cu:L160-195) as an ordered sum, same operands:
 * gfeats[b,c,p,a'] = the products grad[b,c,k,p,a] * w[a,k,n] with idx[a,n] == a', each rounded once, added over a ascending, then k
 * ascending, then n ascending, starting from zero.  The table is inverted in LDS (4*(na_in + 1 + 2*na_out*ann) bytes <= 64 KB;
 * na_in <= 16384).  Meant for SMALL tables (the reference's are 60 x 12): every block of 32 points inverts the table again, each lane
 * scanning all of it, with a serial prefix over na_in -- at the largest sizes admitted that prelude dominates.  gfeats is fully written; no
 * floating-point atomics.  Regime name: intra_zpconv_bwd_ordered. */
int eap_intra_zpconv_bwd_ordered_f32(int b, int np, int na_in, int na_out, int ks, int ann, int c,
                                     const int32_t *idx, const float *w, const float *grad, float *gfeats,
                                     eap_stream_t stream);
int eap_intra_zpconv_bwd_ordered_f64(int b, int np, int na_in, int na_out, int ks, int ann, int c,
                                     const int32_t *idx, const double *w, const double *grad,
                                     double *gfeats, eap_stream_t stream);

/* ---- SO(3) inter convolution (vgtk/vgtk/so3conv/functional.py) ---------------------------- */

/* so3_prep: relative offsets and relative-rotation anchor of every (point, neighbour) pair --
 * so3conv/functional.py:L1061-1078 (gather + R_p R_n^T + rotate offsets) and the nearest-anchor
 * half of L1199-1204.
 * q_xyz [b,3,p], s_xyz [b,3,n], idx int32 [b,p,nn], pose [b,n,4,4] (q_pose [b,p,4,4]) or NULL
 * for identity poses, anchors [na,3,3]
 *  -> gx float4 [b,p,nn] = (gx,gy,gz, bit-cast int r) with g = R_rel (x_n - x_p) and
 *     r = argmax_g tr(R_rel A_g)  (r = index of the identity anchor when pose == NULL);
 *     nonident int32 [b] (optional): set to 1 for clouds where some r != identity_anchor. */
int eap_so3_prep_f32(int b, int p, int n, int nn, int na, const float *q_xyz, const float *s_xyz,
                     const int32_t *idx, const float *q_pose, const float *s_pose,
                     const float *anchors, int identity_anchor, float *gx, int32_t *nonident,
                     eap_stream_t stream);

/* so3_inter_weights: inter_so3conv_grouping_anchor, so3conv/functional.py:L2508-2549.
 * gx float4 [b,p,nn] (from so3_prep), rk [na,ks,3] = A_a kappa_k
 *  -> w [b,p,na,ks,nn] = relu(1 - |g - rk|^2 / sigma). */
int eap_so3_inter_weights_f32(int b, int p, int nn, int na, int ks, float sigma, const float *gx,
                              const float *rk, float *w, eap_stream_t stream);

/* so3_anchor_perm: the full index of so3conv/functional.py:L1199-1204,
 * perm[b,p,n,a] = mult[r[b,p,n]][a] as int64 (what torch.argmax returns). */
int eap_so3_anchor_perm(int b, int p, int nn, int na, const float *gx, const uint8_t *mult,
                        int64_t *perm, eap_stream_t stream);

/* so3_inter_group_fwd: fused kernel-weight + anchor-permutation + gather + weighted sum,
 * so3conv/functional.py:L1112-1261 (einsum 'bcpna,bpakn->bckpa' at L1261) without materialising
 * the [b,p,na,ks,nn] weights.
 * feats [b,c,n,na], idx [b,p,nn], gx float4 [b,p,nn], rk [na,ks,3], mult [na,na] (NULL = no
 * permutation, permute_modes == 0), nonident int32 [b] from so3_prep or NULL (clouds whose flag
 * is 0 skip the table) -> out [b,c,ks,p,na]. */
int eap_so3_inter_group_fwd_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                const float *feats, const int32_t *idx, const float *gx,
                                const float *rk, const uint8_t *mult, const int32_t *nonident,
                                float *out, eap_stream_t stream);
/* The implementation behind so3_inter_group_fwd for c < 16, exported for tests: lanes = anchors, register tile of
 * channels x kernel points. */
int eap_so3_inter_group_fwd_valu_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                     const float *feats, const int32_t *idx, const float *gx,
                                     const float *rk, const uint8_t *mult, float *out,
                                     eap_stream_t stream);

/* so3_inter_group_bwd: transpose of the above w.r.t. feats.
 * gout [b,c,ks,p,na] -> gfeats [b,c,n,na] (zero-initialised by the call, fp32 atomics). */
int eap_so3_inter_group_bwd_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                const float *gout, const int32_t *idx, const float *gx,
                                const float *rk, const uint8_t *mult, float *gfeats,
                                eap_stream_t stream);

/* Atomics-free variant of so3_inter_group_bwd (ks <= 24, na % 4 == 0): every block owns a private slab of
 * partial sums in `workspace` (eap_so3_inter_group_bwd_workspace floats, zeroed by the call) and
 * a second kernel reduces the slabs -- deterministic, and ~4x faster than fp32 row atomics. */
int64_t eap_so3_inter_group_bwd_workspace(int b, int c, int p, int n, int na);
int eap_so3_inter_group_bwd_slab_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                     const float *gout, const int32_t *idx, const float *gx,
                                     const float *rk, const uint8_t *mult, int identity_anchor,
                                     float *gfeats, float *workspace, eap_stream_t stream);

/* ---- anchor sets that are not a group (the 20- / 40-anchor subsets, so3conv/functional.py:L2641-2649) ---- */

/* so3_anchor_map: the anchor index of so3conv/functional.py:L1199-1204 searched per entry -- on a subset of the group the
 * arg-max depends on the actual R_rel and is no permutation, so no [na,na] table can stand for it.
 * idx int32 [b,p,nn], q_pose [b,p,4,4], s_pose [b,n,4,4] (the same tensor unless the conv is strided), anchors [na,3,3],
 * na % 4 == 0, na <= 64
 *  -> amap uint8 [b,p,nn,na] = argmax_j <R_rel^T A_a, A_j>_F with R_rel = R_p R_idx^T (the lowest j wins a tie);
 *     nontrivial int32 [b] = 1 for clouds where some entry's map is not the identity map (zeroed by the call). */
int eap_so3_anchor_map_f32(int b, int p, int n, int nn, int na, const int32_t *idx, const float *q_pose,
                           const float *s_pose, const float *anchors, uint8_t *amap, int32_t *nontrivial,
                           eap_stream_t stream);

/* so3_inter_group_fwd_map: so3conv/functional.py:L1221-1261 with the gather through the map,
 * out[b,c,k,p,a] = sum_n w(p,a,k,n) feats[b,c,idx_n,amap[b,p,n,a]]  (reference layout [b,c,ks,p,na]; weights from gx and
 * rk as eap_so3_inter_group_fwd_f32; na % 4 == 0, na <= 64, ks <= 32). */
int eap_so3_inter_group_fwd_map_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                    const float *feats, const int32_t *idx, const float *gx, const float *rk,
                                    const uint8_t *amap, float *out, eap_stream_t stream);

/* so3_inter_group_bwd_map: the transpose of the above w.r.t. feats (autograd of so3conv/functional.py:L1221-1261),
 * gfeats[b,c,q,a'] = sum_{(p,n): idx = q} sum_{a: amap(a) = a'} sum_k w(p,a,k,n) gout[b,c,k,p,a].
 * The map is many-to-one in q and in a: private slabs in `workspace` (eap_so3_inter_group_bwd_map_workspace floats,
 * zeroed by the call) accumulated in a fixed order and reduced by a second kernel -- no float atomics, bit-identical
 * run to run, lists that name a row twice included. */
int64_t eap_so3_inter_group_bwd_map_workspace(int b, int c, int p, int n, int na);
int eap_so3_inter_group_bwd_map_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                    const float *gout, const int32_t *idx, const float *gx, const float *rk,
                                    const uint8_t *amap, float *gfeats, float *workspace, eap_stream_t stream);

/* ---- the `use_2d` variant with really permuted residual indices (so3conv/functional.py:L1718-2130; csrc/so3_inter_res.hip) ---- */

/* so3_residual_index: rotated_anchor_idx of so3conv/functional.py:L1934-1938, one byte per entry.
 * idx int32 [b,p,nn], q_pose [b,p,4,4], s_pose [b,n,4,4], res [4,3,3] (the four residual rotations about y, L1921)
 *  -> shift uint8 [b,p,nn]: field z (bits 2z, 2z+1) = argmax_j tr(R_rel^T RES_z RES_j^T) with R_rel = R_p R_idx^T, compared with a
 *     strict >, so the lowest j wins a tie (torch.argmax); the four fields are a cyclic shift only where no trace ties;
 *     nontrivial int32 [b] = 1 for clouds where some entry's byte is not the identity byte 0xE4 (field z = z); zeroed by the call. */
int eap_so3_residual_index_f32(int b, int p, int n, int nn, const int32_t *idx, const float *q_pose,
                               const float *s_pose, const float *res, uint8_t *shift, int32_t *nontrivial,
                               eap_stream_t stream);

/* so3_inter_group_fwd_res: so3conv/functional.py:L1944-1957 (shadow row, gather of the neighbours, gather of the residual plane through
 * the index) and L2124 (the weighted sum) without the [b,p,nn,na,4,c] and [b,p,na,4,ks,nn] tensors,
 * out[b,c,k,p,a,z] = sum_n w(p,(a,z),k,n) feats[b,c,idx_n,a,shift_z(b,p,n)].
 * feats [b,c,n,na,4], idx int32 [b,p,nn] (an index >= n names the shadow row: skipped), gx float4 [b,p,nn] from so3_prep,
 * rk [na*4,ks,3] = A_a RES_z kappa_k, shift uint8 [b,p,nn] (ANY byte: many-to-one maps included) -> out [b,c,ks,p,na*4] (the
 * reference layout).  na <= 64, ks <= 32; feats and out 16-byte aligned. */
int eap_so3_inter_group_fwd_res_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                    const float *feats, const int32_t *idx, const float *gx, const float *rk,
                                    const uint8_t *shift, float *out, eap_stream_t stream);

/* so3_inter_group_bwd_res: the transpose of the above w.r.t. feats (autograd of so3conv/functional.py:L1944-1957 + L2124),
 * gfeats[b,c,q,a,s] = sum_{(p,n): idx = q} sum_{z: shift_z = s} sum_k w(p,(a,z),k,n) gout[b,c,k,p,a,z].
 * Many-to-one in q (and, on ties, in s): private slabs in `workspace` (eap_so3_inter_group_bwd_res_workspace floats, zeroed by the
 * call) accumulated in a fixed order and reduced by a second kernel -- no float atomics, bit-identical run to run, lists that name
 * a row twice included.  Same limits; gout and gfeats 16-byte aligned. */
int64_t eap_so3_inter_group_bwd_res_workspace(int b, int c, int p, int n, int na);
int eap_so3_inter_group_bwd_res_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                    const float *gout, const int32_t *idx, const float *gx, const float *rk,
                                    const uint8_t *shift, float *gfeats, float *workspace, eap_stream_t stream);

/* Which entry-list grouping kernel serves eap_so3_inter_group_fwd*_f32 / eap_so3_inter_group_inv*_f32 when no anchor
 * permutation is in play: 2 (default) = the fp32-MFMA kernel with two channel tiles per wave where the channel count fills
 * 64-channel blocks (csrc/so3_inter_lists2.hip), 1 = always the one-tile fp32-MFMA kernel (csrc/so3_inter_lists.hip);
 * 0 = query.  Returns the value in force.  1 and 2 agree bit for bit (tests compare them).  (Two measured-slower
 * experiments -- a 3 x bf16 split grouping kernel, a re-cut zpconv forward -- are recorded in profiles/; their source is in commit
 * 5d523ff.) */
int eap_so3_group_lists_tiles(int tiles);
/* Row end of the two-tile forward kernel writing the transposed intermediate: 1 (default) = MFMA operands exchanged so that a
 * lane holds four consecutive kernel points of a channel, 16-byte stores; 0 = dword stores in 96-byte runs.  Bit-identical
 * results.  Returns the previous setting; other values only query. */
int eap_so3_group_lists_store16(int on);
/* Clouds WITH anchor permutations on the two-tile kernel (csrc/so3_inter_lists2.hip, PERM; round 4): the operand's anchor
 * axis is COSET-MAJOR (eap_anchor_reorder_f32 with the `order` of vgtk.so3conv.functional._coset_tables), the block move of an
 * entry's permutation rides on the DMA source addresses, the in-block XOR is 8 selects per operand read, and everything that
 * depends on the entry's rotation alone is prepared once per entry:
 *   eap_so3_group_perm_lists2(on)      1 (default) / 0: switch for A/B runs and tests; returns the previous setting
 *   eap_so3_group_perm_lists2_takes    1 if this shape goes there (else the whole-row kernel, eap_so3_inter_group_inv_coset_f32)
 *   eap_so3_perm_entries_f32           ent_p int32 [b*per_cloud], ent_gx [b*per_cloud,4] (w = bits of the rotation's anchor r),
 *                                      nonident int32 [b] or NULL (clouds with flag 0 are skipped),
 *                                      code uint8 [na,16] (coset code table of the permutation table in force), anchors [na,3,3]
 *                                      or NULL (backward: offset vectors rotated by A_r)
 *                                      -> ent_pc uint32 [b*per_cloud,4,4] (byte offset of each 16-byte piece's source in a channel
 *                                         row of the cloud, per anchor group and piece), ent_gx2 [b*per_cloud,4] (w = in-block
 *                                         XOR bits of the 15 blocks; shadow neighbours get a dead offset vector)
 *   eap_so3_inter_group_inv_perm2_f32  Z of the re-associated backward (replaces autograd of so3conv/functional.py:L1199-1261
 *                                      for permuted clouds): gy [b,o,p,na] coset-major -> z [b,o,ks,rcap,na] coset-major */
int eap_so3_group_perm_lists2(int on);
int eap_so3_group_perm_lists2_takes(int channels, int na, int ks, int n_support);
int eap_so3_perm_entries_f32(int b, int per_cloud, int na, int n_support, const int32_t *ent_p, const float *ent_gx, const uint8_t *code,
                             const float *anchors, int identity_anchor, const int32_t *nonident, int32_t *ent_pc, float *ent_gx2,
                             eap_stream_t stream);
/* the forward with the same kernel: eap_so3_inter_group_fwd_t_f32's output (X^T, memory order) where the clouds WITH
 * permutations (nonident[b] != 0) read feats_c = feats with a coset-major anchor axis (eap_anchor_reorder_clouds_f32) and the
 * per-entry words of (idx, gx) (eap_so3_perm_entries_f32 with the multiplication table's code, anchors = NULL, the flags); the
 * other clouds take the plain kernel.  Replaces so3conv/functional.py:L1199-1261 for those clouds. */
int eap_so3_inter_group_fwd_perm2_t_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats,
                                        const float *feats_c, const int32_t *idx, const float *gx, const int32_t *ent_pc,
                                        const float *ent_gx2, const float *rk, const uint8_t *order, const int32_t *nonident,
                                        int store_order_columns, float *out, eap_stream_t stream);
/* eap_so3_inter_group_fwd_t_f32 (clouds without anchor permutations) with the COLUMNS of the transposed matrix in the order the
 * kernel's lanes hold them, so that every store instruction writes one contiguous 1 KB run (round 4; the intermediate is
 * scratch between the grouping and the contraction, and a contraction sums over the columns: it reads W[:, perm] beside it).
 * eap_so3_group_fwd_tp_takes: 1 if the shape is taken (whole 64-channel blocks, ks % 8 == 0); eap_so3_group_fwd_tp_columns
 * fills the HOST array perm [c*ks]: position j of a row holds column perm[j] = channel * ks + kernel point of the plain matrix. */
int eap_so3_group_fwd_tp_takes(int c, int na, int ks);
int eap_so3_group_fwd_tp_columns(int c, int ks, int32_t *perm);
int eap_so3_inter_group_fwd_tp_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma, const float *feats,
                                   const int32_t *idx, const float *gx, const float *rk, float *out, eap_stream_t stream);
int eap_so3_inter_group_inv_perm2_f32(int b, int o, int p, int nn, int na, int ks, int rcap, float sigma, const float *gy,
                                      const int32_t *rows, const int32_t *off, const int32_t *cnt, const int32_t *ent_pc,
                                      const float *ent_gx2, const float *rk, const uint8_t *order, float *z, eap_stream_t stream);

/* so3_inter_group_inv: the feature gradient of the whole inter convolution by re-association,
 *   dF[c,q,a'] = sum_{o,k} W[o,(c,k)] Z[o,k,q,a'],
 *   Z[o,k,q,a'] = sum_{(p,n): idx[p,n]=q} dY[o,p,a] w(p,a,k,n),  a = perm_n^-1(a')
 * i.e. the forward grouping applied to dY over INVERSE neighbour lists (autograd of
 * so3conv/functional.py:L1221-1261 + modules.py:L48-55 without ever forming dX = W^T dY).
 * gy [b,o,p,na]; the referenced support rows of each batch item are compacted to `rcap` slots:
 * rows [b,rcap] (support index or -1), off/cnt [b,rcap] (range of the row's entries in the
 * per-item sorted entry list), ent_p [b,p*nn] (query point of each entry), ent_gx float4
 * [b,p*nn] (its so3_prep word), rk [na,ks,3], multinv [na,na] (multinv[r][a'] = a, NULL = no
 * permutation), anchors [na,3,3] (the rotations the table was built from; needed with multinv: an
 * entry's offset vector is rotated by A_r once so that its weights are those of the accumulator's own
 * anchor)  ->  z [b,o,ks,rcap,na].  The caller finishes with eap_gemm_dma_f32. */
int eap_so3_inter_group_inv_f32(int b, int o, int p, int nn, int na, int ks, int rcap, float sigma,
                                const float *gy, const int32_t *rows, const int32_t *off,
                                const int32_t *cnt, const int32_t *ent_p, const float *ent_gx,
                                const float *rk, const uint8_t *multinv, const float *anchors,
                                int identity_anchor, float *z, eap_stream_t stream);
/* The same for clouds with anchor permutations, given the coset tables of `multinv` (order uint8 [64]: anchor at every position of
 * a coset-major ordering, blocks of 4 = left cosets of a Klein four-group of the anchor group; code uint8 [na,16], 4-byte
 * aligned: per permutation row and block `sigma | x << 4`): the LDS operand is kept in that order, so the four permuted anchors
 * of a block are one 16-byte read of block sigma + an index-XOR shuffle.  Same results to the last bit of the products summed
 * (the anchors are visited in another order only across waves). */
/* dst [rows, na] = src with its anchor axis re-ordered, dst[., i] = src[., order[i]]: for na = 4 mod 8 the entry below takes gy's
 * rows by DMA and expects them in coset-major order already. */
int eap_anchor_reorder_f32(int64_t rows, int na, const float *src, const uint8_t *order, float *dst, eap_stream_t stream);
/* The same for [b, rows_per_cloud, na] with a flag per cloud: clouds whose nonident[b] is 0 are skipped (dst left unwritten). */
int eap_anchor_reorder_clouds_f32(int b, int64_t rows_per_cloud, int na, const float *src, const uint8_t *order,
                                  const int32_t *nonident, float *dst, eap_stream_t stream);
int eap_so3_inter_group_inv_coset_f32(int b, int o, int p, int nn, int na, int ks, int rcap, float sigma,
                                      const float *gy, const int32_t *rows, const int32_t *off, const int32_t *cnt,
                                      const int32_t *ent_p, const float *ent_gx, const float *rk, const uint8_t *multinv,
                                      const float *anchors, int identity_anchor, const uint8_t *coset_order,
                                      const uint8_t *coset_code, float *z, eap_stream_t stream);

/* Inverse neighbour lists for so3_inter_group_inv, built on the device (the autograd transpose of the
 * gather at so3conv/functional.py:L1221-1252 needs, per referenced support row, the (point, slot) pairs
 * that reference it).  idx int32 [b,p,nn] with values in [0,n) (other values are ignored), n <= 16384.
 * eap_inv_lists_rows: counts [b,n] (scratch) -> rows [b,n] (referenced support rows, longest list first,
 *   ties by index; -1 past the end), cnt [b,n], off [b,n] (start of each row's entries in the per-cloud
 *   entry list), n_rows [b].
 * eap_inv_lists_fill: for the first `rcap` rows of every cloud (rows / off as written above, leading
 *   dimension n): ent_p int32 [b,p*nn] (query point of each entry, entries of a row in (p,slot) order),
 *   ent_gx float4 [b,p*nn] (its so3_prep word).  p*nn must be a multiple of 4. */
int eap_inv_lists_rows(int b, int p, int n, int nn, const int32_t *idx, int32_t *counts, int32_t *rows,
                       int32_t *off, int32_t *cnt, int32_t *n_rows, eap_stream_t stream);
int eap_inv_lists_fill(int b, int p, int n, int nn, int rcap, const int32_t *idx, const float *gx,
                       const int32_t *rows, const int32_t *off, int32_t *ent_p, float *ent_gx,
                       eap_stream_t stream);
/* Referenced rows of a feature tensor: dst [b,c,rcap,na] = src [b,c,n,na][:, :, rows[b,r], :] (zeros where
 * rows < 0), and the transpose dst [b,c,n,na] = 0; dst[:, :, rows[b,r], :] = src [b,c,rcap,na].
 * rows int32 with leading dimension rows_ld; na a multiple of 4. */
int eap_rows_gather_f32(int b, int c, int n, int na, int rcap, int rows_ld, const int32_t *rows,
                        const float *src, float *dst, eap_stream_t stream);
int eap_rows_scatter_f32(int b, int c, int n, int na, int rcap, int rows_ld, const int32_t *rows,
                         const float *src, float *dst, eap_stream_t stream);
/* The two movements above on the PACKED anchor-major axis of the dense layers' gradient tail (eap_so3_dense_product_packed_f32): element (a, r) of
 * cloud i at a live16[i] + r, live16[i] = eap_so3_dense_live16(n_rows[i], rp).  gather: src [b,c,n,na] -> dst [b,c,ld] (slots r >= n_rows[i] of the
 * last 16-row group: zeros; nothing written past na live16[i]); scatter: src [b,c_ld,ld] (the first c of each cloud's c_ld rows, live columns only)
 * -> dst [b,c,n,na], zero except the named rows.  na <= 64, rp % 16 == 0, ld >= na rp. */
int eap_rows_gather_packed_f32(int b, int c, int n, int na, int rp, int rows_ld, int64_t ld, const int32_t *rows, const int32_t *n_rows,
                               const float *src, float *dst, eap_stream_t stream);
int eap_rows_scatter_packed_f32(int b, int c, int c_ld, int n, int na, int rp, int rows_ld, int64_t ld, const int32_t *rows,
                                const int32_t *n_rows, const float *src, float *dst, eap_stream_t stream);

/* ---- the fused inter conv re-associated over its referenced rows as a dense product (csrc/so3_dense.hip) ----
 * Replaces, for clouds WITHOUT pose rotations whose neighbour lists name few support rows, the grouping einsum +
 * contraction of so3conv/functional.py:L1112-1261 + so3conv/modules.py:L48-55 (forward) and their autograd transpose
 * (backward).  With rows[b, 0..rp) the referenced support rows of cloud b (eap_inv_lists_rows; rp a multiple of 4, empty
 * slots = -1) and m[p,r] = 1 iff row r is in idx[b,p,:]:
 *     Wd[p,(k,r),a] = m[p,r] relu(1 - |x_row(r) - x_p - rk[a,k]|^2 / sigma)
 *     dir 0 (backward)  Z [b,o,k,a,r]   = sum_p      dY[b,o,p,a]     Wd[p,(k,r),a]
 *     dir 1 (forward)   Yt[b,a,o,p]     = sum_(k,r)  G [b,o,(k,r),a] Wd[p,(k,r),a]      (G = W F over the referenced rows)
 * on the fp16 matrix cores with two planes per operand and fp32 accumulation (the arithmetic of eap_gemm_f16x2_f32).  Inside, the
 * (k, r) axis runs in the DENSE INDEX order d = (r / 16) 16 ks + 16 k + r % 16; a cloud with n_rows[b] < rp referenced rows uses a
 * prefix of it, and with n_rows given the products stop there (dir 0 zeroes the slots past ceil16(n_rows[b]) in Z).
 * The weights are evaluated from the squared distance, in the reference's own order of operations (csrc/so3_dense.hip).
 *   eap_so3_dense_supported   p % 32 == 0, na % 4 == 0, na <= 64, ks % 2 == 0, rp % 16 == 0, rp <= 1024 (eap_so3_dense_max_rows), o % 128 == 0 (256-row
 *                             blocks when o % 256 == 0).  The product, table, split and operand entries take every such rp; the entries that take
 *                             `memb` come in two widths: the plain ones below (memb [b,p,16], int32 keys, rp <= 512) and the *_wide ones further down
 *                             (memb [b,p,32], int64 keys, rp <= 1024).  Up to 512 rows both give the same tables from the same membership bits.
 *   eap_so3_dense_member      slot_of int32 [b,n] (scratch), memb uint32 [b,p,16] (bit r of point p = m[p,r]; rp <= 512),
 *                             flags int32 [b]: 1 = a list names a row twice (padded short lists, grouping_cuda_kernel.cu:L98-107:
 *                             not representable by a 0/1 mask), 2 = a list names a row outside rows[:, :rp] -- such clouds
 *                             must take the list kernels
 *   eap_so3_dense_mask_words  uint64 words of the mask table of one direction; eap_so3_dense_masks fills it:
 *                             [b][64-column wave tile][k-step of 32][64 lanes] one bit per weight a lane of the product kernel generates
 *   eap_so3_dense_tables_f32  centre [b,4] (centroid of the support points), pt float4 [b, ceil32(p)] and
 *                             kr float4 [b, na, ceil32(ks rp)]: the two sides of the weight (centred coordinates), evaluated in float64;
 *                             row_rot (may be null) float [b, rows_ld, 9]: a rotation per row slot applied to the kernel offsets --
 *                             the query points of ONE rigid part of a posed cloud (R_rel^T of so3conv/functional.py:L1112-1160)
 *   eap_so3_dense_split_f32   src [b,m,l,na] -> scale [2][b,na,m] (power of two per row; the second copy as [b,m,na]) and the two fp16 planes of the scaled
 *                             rows in the product kernel's fragment order: 4 b na m ceil32(l) bytes
 *                             (rowmax uint32 [b,m,na], may be null: the rows' largest magnitudes as float bit patterns when the producer
 *                             of src already has them, eap_bn_act_bwd_apply_rowmax_f32; seg > 0: a row's l elements come in segments of seg elements seg_pitch floats apart -- G as a GEMM with
 *                             padded columns leaves it; colmap int32 [b,l], may be null: element i of a row is element colmap[b,i] of a source row of
 *                             seg_pitch floats, negative = zero -- the columns of dY that are the query points of one rigid part)
 *   eap_so3_dense_product_f32 the product (planes / scale of dY [b,o,p,na] for dir 0, of G [b,o,ks rp,na] for dir 1); dir 0 writes
 *                             Z with ldz >= na rp floats between its (o, k) rows (padding for the GEMMs that follow, not written)
 *   eap_so3_dense_untranspose_f32   Yt [b,na,o,p] -> Y [b,o,p,na]; psum / psq (may be null) float [o, b ceil(p/64)]: partial sums of
 *                             y - y[0,o,0,0] and of its square, the moments of the BatchNorm that follows (eap_bn_stats_f32's pivot)
 *   eap_so3_dense_untranspose_map_f32   the same into a Y [b,o,p_dst,na] that several launches fill: column pp of cloud b is point
 *                             map[b,pp] (int32 [b,p]; negative: padding, dropped) -- the rigid parts of posed clouds, one launch each
 *   eap_so3_dense_untranspose_map_stats_f32   ... with the moments of eap_so3_dense_untranspose_f32 (columns whose map entry is >= 0);
 *                             pivot_pos int32 [1] on the device: the column of cloud 0 that is point 0 (the pivot stays Y[0,o,0,0])
 *                             All four re-ordering entries (these three and eap_so3_dense_untranspose_bnact_f32) move a row of Y as na / 4
 *                             16-byte pieces through a tile of at most 64 anchors: na % 4 == 0, na <= 64, yt and y 16-byte aligned, else
 *                             hipErrorInvalidValue with the condition in eap_last_error(), before anything is launched
 * Occupancy-sorted query points (round 6).  The reference's ball query keeps the first nsample hits in index order
 * (grouping_cuda_kernel.cu:L68-113), so a point's list names rows of only 0.45-0.7 of a cloud's 16-row groups; with a cloud's query
 * points sorted by WHICH groups they touch the 0/1 mask of the product is block-sparse and whole k-steps drop out:
 *   eap_so3_dense_point_keys   memb [b,p,16] -> keys int32 [b,p], bit g = the list of p names a row slot of 16 g .. 16 g + 15; the host sorts
 *                             a cloud's points by it and builds memb / pt / the masks in that order (the order is a column map for
 *                             eap_so3_dense_split_f32 and eap_so3_dense_untranspose_map*_f32)
 *   eap_so3_dense_steps_words / eap_so3_dense_steps   from the mask table of a direction: int32 [b][column blocks of 256][k-steps + 1] =
 *                             count (>= 1) and the ascending k-steps in which the block generates a weight that is not masked out
 *                             (skip = 0: every k-step; dir 1 with n_rows: of the cloud's prefix)
 *   eap_so3_dense_product_steps_f32   eap_so3_dense_product_f32 whose column blocks run their listed k-steps only (steps may be null; lists
 *                             longer than 1024 k-steps are ignored: every k-step runs).  Skipped k-steps would have added exact zeros:
 *                             bit-equal to running them all in the same point order.  so3conv/functional.py:L1221-1261 */
int eap_so3_dense_supported(int p, int na, int ks, int rp, int o);
int eap_so3_dense_member(int b, int p, int n, int nn, int rp, int rows_ld, const int32_t *idx, const int32_t *rows,
                         const int32_t *n_rows, int32_t *slot_of, uint32_t *memb, int32_t *flags, eap_stream_t stream);
int64_t eap_so3_dense_mask_words(int b, int p, int ks, int rp, int dir);
int eap_so3_dense_masks(int b, int p, int ks, int rp, int dir, const uint32_t *memb, uint64_t *mask, eap_stream_t stream);
int eap_so3_dense_tables_f32(int b, int p, int n, int na, int ks, int rp, int rows_ld, float sigma, const float *q_xyz,
                             const float *s_xyz, const int32_t *rows, const float *rk, const float *row_rot, float *centre, float *pt,
                             float *kr, eap_stream_t stream);
int eap_so3_dense_split_f32(int b, int m, int l, int na, int seg, int64_t seg_pitch, int mapped, const int32_t *n_rows, const uint32_t *rowmax,
                            const int32_t *colmap, const float *src, float *scale, void *planes, eap_stream_t stream);
int eap_so3_dense_product_f32(int dir, int b, int o, int p, int na, int ks, int rp, int64_t ldz, float sigma, const int32_t *n_rows, const void *planes,
                              const float *scale,
                              const float *pt, const float *kr, const uint64_t *mask, float *out, eap_stream_t stream);
int eap_so3_dense_untranspose_f32(int b, int o, int p, int na, const float *yt, float *y, float *psum, float *psq, eap_stream_t stream);
int eap_so3_dense_untranspose_map_f32(int b, int o, int p, int na, int p_dst, const int32_t *map, const float *yt, float *y,
                                      eap_stream_t stream);
int eap_so3_dense_untranspose_map_stats_f32(int b, int o, int p, int na, int p_dst, const int32_t *map, const int32_t *pivot_pos, const float *yt,
                                            float *y, float *psum, float *psq, eap_stream_t stream);
/* conv + training-mode BatchNorm + leaky_relu as ONE node (round 6; `x = conv(x); feat = relu(norm(x.feats))`,
 * SPConvNets/utils/base_so3poseconv.py:L205-222, and its autograd): the forward's re-ordering pass applies the normalisation on the way out
 * (eap_so3_dense_untranspose_bnact_f32; the moments come from eap_bn_stats_f32 over Yt viewed as [b na, o, p]); the backward never writes
 * the gradient behind the BatchNorm: eap_bn_act_bwd_reduce_fromy_f32 (csrc/bn_act.hip) reduces sum(g), sum(g xhat) and leaves per-row bounds,
 * eap_so3_dense_split_bn_f32 forms gx = k1 g - k2 - k3 xhat while it splits it into the product's planes.  Both recover the
 * pre-activation from the layer's OUTPUT (leaky_relu with a positive slope is invertible): the conv output is not kept. */
int eap_so3_dense_split_bn_f32(int b, int m, int l, int l_src, int na, const uint32_t *rowbound, const int32_t *colmap, const float *grad,
                               const float *act, const float *coef, float slope, float *scale, void *planes, eap_stream_t stream);
int eap_so3_dense_untranspose_bnact_f32(int b, int o, int p, int na, int p_dst, const int32_t *map, const float *yt, const float *bn_scale,
                                        const float *bn_shift, float slope, float *y, eap_stream_t stream);
/* the forward's stored operand G[o,(k,r),a] = sum_c W[o,c,k] F[c,r,a] made and written as the product's planes by one kernel (round 6; before:
 * a GEMM that wrote G in fp32 and eap_so3_dense_split_f32 that read it back): W3 float [o ks][c], Ft float [b][na][rp][c] (referenced feature
 * rows, empty slots zero), bound float [b][na][o] >= max |G| of the output row, n_rows [b] (may be null) -> scale [b][na][o], planes.
 * so3conv/functional.py:L1221-1261 + so3conv/modules.py:L48-55 re-associated (csrc/so3_dense.hip header) */
int eap_so3_dense_gplanes_supported(int o, int c, int na, int ks, int rp);
int eap_so3_dense_gplanes_f32(int b, int o, int c, int na, int ks, int rp, const float *W3, const float *Ft, const int32_t *n_rows,
                              const float *bound, float *scale, void *planes, eap_stream_t stream);
int eap_so3_dense_point_keys(int b, int p, const uint32_t *memb, int32_t *keys, eap_stream_t stream);
int64_t eap_so3_dense_steps_words(int b, int p, int ks, int rp, int dir);
int eap_so3_dense_steps(int b, int p, int ks, int rp, int dir, int skip, const int32_t *n_rows, const uint64_t *mask, int32_t *steps,
                        eap_stream_t stream);
int eap_so3_dense_product_steps_f32(int dir, int b, int o, int p, int na, int ks, int rp, int64_t ldz, float sigma, const int32_t *n_rows,
                                    const void *planes, const float *scale, const float *pt, const float *kr, const uint64_t *mask,
                                    const int32_t *steps, float *out, eap_stream_t stream);
/* the backward product (dir 0) with PACKED rows of Z: column (a, r) of cloud i at a live16[i] + r, live16[i] = eap_so3_dense_live16(n_rows[i], rp)
 * = ceil16(min(n_rows[i], rp)) -- the cloud's na live16[i] live columns are one prefix of every (o, k) row (pitch ldz >= na rp as above); nothing
 * behind the prefix is written or zeroed.  n_rows is required.  Consumers: eap_gemm_f16x2_splitk_tail_f32, eap_gemm_bf16x3_reduce_tail_f32. */
int eap_so3_dense_product_packed_f32(int b, int o, int p, int na, int ks, int rp, int64_t ldz, float sigma, const int32_t *n_rows,
                                     const void *planes, const float *scale, const float *pt, const float *kr, const uint64_t *mask,
                                     const int32_t *steps, float *out, eap_stream_t stream);
/* host arithmetic: the row slots of a cloud with n_rows referenced rows in a batch of rp slots, in whole 16-row groups (0 without rows) */
int eap_so3_dense_live16(int n_rows, int rp);
/* Clouds that reference up to 1024 support rows: 64 groups of 16 rows, 32 membership words per point, a 64-bit group key.
 *   eap_so3_dense_max_rows          the largest rp any entry takes (1024)
 *   eap_so3_dense_member_wide       eap_so3_dense_member with memb uint32 [b,p,32] (bit i of word w of point p = m[p, 32 w + i]); rp <= 1024;
 *                                   flag 2 = more than rp referenced rows
 *   eap_so3_dense_point_keys_wide   memb uint32 [b,p,32] -> keys int64 [b,p], bit g < 64 = the list of p names a row slot of 16 g .. 16 g + 15
 *   eap_so3_dense_masks_wide        memb uint32 [b,p,32], rp <= 1024 -> the mask table of eap_so3_dense_masks (same layout, eap_so3_dense_mask_words)
 *   eap_so3_dense_steps_wide        eap_so3_dense_steps for rp <= 1024 (same layout, eap_so3_dense_steps_words)
 * Everything else (tables, split, operand, product, re-ordering) is the same entry at either width. */
int eap_so3_dense_max_rows(void);
int eap_so3_dense_member_wide(int b, int p, int n, int nn, int rp, int rows_ld, const int32_t *idx, const int32_t *rows,
                              const int32_t *n_rows, int32_t *slot_of, uint32_t *memb, int32_t *flags, eap_stream_t stream);
int eap_so3_dense_point_keys_wide(int b, int p, const uint32_t *memb, int64_t *keys, eap_stream_t stream);
int eap_so3_dense_masks_wide(int b, int p, int ks, int rp, int dir, const uint32_t *memb, uint64_t *mask, eap_stream_t stream);
int eap_so3_dense_steps_wide(int b, int p, int ks, int rp, int dir, int skip, const int32_t *n_rows, const uint64_t *mask, int32_t *steps,
                             eap_stream_t stream);
/* The five words the host reads before it picks a layer's kernels (csrc/list_probe.hip), after eap_inv_lists_rows and
 * eap_so3_dense_member[_wide]:
 *   out[0] = max_b n_rows[b];  out[1] = max_b nonident[b] (1 when nonident is null);
 *   out[2] = max_b dflags[b] (1 when memb and dflags are null) + 1 per given pose tensor rot_a / rot_b [blocks,4,4] with a 3x3 block that
 *            is not exactly the identity + 1 when rot_cloud [b,3,3] has max |R R^T - I| > 1e-6 in float64;
 *   out[3] = (int32)(float(max_b #{non-zero 16-bit halves of memb[b]}) * float(16 / p)), memb uint32 [b,p,words], words 16 or 32 (0 without);
 *   out[4] = 1 when a channel has norm_w != 0 and |norm_b| > ratio |norm_w| (0 when norm_w and norm_b are null).
 * work: int32 [eap_so3_dense_probe_workspace(b)] scratch.  memb and the pose tensors 16-byte aligned. */
int64_t eap_so3_dense_probe_workspace(int b);
int eap_so3_dense_probe(int b, int p, int words, const int32_t *n_rows, const int32_t *nonident, const int32_t *dflags,
                        const uint32_t *memb, const float *rot_a, int64_t blocks_a, const float *rot_b, int64_t blocks_b,
                        const float *rot_cloud, const float *norm_w, const float *norm_b, int channels, float ratio,
                        int32_t *work, int32_t *out, eap_stream_t stream);

/* ---- SO(3) intra convolution -------------------------------------------------------------- */

/* so3_intra_group_fwd: intra_so3conv_grouping, so3conv/functional.py:L2553-2602.
 * feats [b,c,p,na], intra_idx int32 [na,t] -> out [b,c,t,p,na] = feats[b,c,p,intra_idx[a,t]]. */
int eap_so3_intra_group_fwd_f32(int b, int c, int p, int na, int t, const float *feats,
                                const int32_t *intra_idx, float *out, eap_stream_t stream);
/* transpose: gout [b,c,t,p,na] -> gfeats [b,c,p,na] (deterministic, inverse index). */
int eap_so3_intra_group_bwd_f32(int b, int c, int p, int na, int t, const float *gout,
                                const int32_t *intra_idx, float *gfeats, eap_stream_t stream);

/* ---- dense contraction (BasicSO3Conv.forward, so3conv/modules.py:L48-55) ------------------- */

/* Operand contract of every GEMM entry below (pinned by tests/test_gpu_gemm_contract.py on buffers whose padding holds NaN):
 *   - a leading dimension may exceed the logical width, a batch stride the size of an item, and a base may point anywhere
 *     inside a larger allocation (subject to the alignment each entry or its `_supported` predicate states);
 *   - nothing outside the logical elements of an input influences a result: rows, columns and k-tails a tile does not own are
 *     selected as zero (or re-read from a valid row and discarded), never loaded from the padding and multiplied by zero;
 *   - nothing outside [M, N] of each item of C is written: not the padding of a row (ldc > N), not the gap between two items,
 *     not a word before the base or after the last row.  A residual is read at pitch ldc, inside [M, N] only. */

/* Batched fp32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32), row-major:
 *   C_z[M,N] = op(A_z)[M,K] * op(B_z)[K,N]       z = 0..batch-1
 * transA = 0: A_z is [M,K] with leading dimension lda; 1: A_z is stored [K,M].  Same for B.
 * stride* are element offsets between consecutive batch items (0 = shared operand).
 * BasicSO3Conv:  C = y [b][O, P*A], A = W [O, C*K] (strideA 0), B = x [b][C*K, P*A]. */
int eap_gemm_f32(int transA, int transB, int M, int N, int K, const float *A, int64_t lda,
                 int64_t strideA, const float *B, int64_t ldb, int64_t strideB, float *C,
                 int64_t ldc, int64_t strideC, int batch, eap_stream_t stream);

/* Split-K / batch-reduced GEMM for the weight gradient:
 *   C[M,N] = sum_z sum_k op(A_z)[M,k] * op(B_z)[k,N]
 * `workspace` holds batch*splits partial [M,N] slabs (eap_gemm_f32_reduce_workspace floats);
 * the reduction over slabs is a second deterministic kernel. */
int64_t eap_gemm_f32_reduce_workspace(int M, int N, int K, int batch);
int eap_gemm_f32_reduce(int transA, int transB, int M, int N, int K, const float *A, int64_t lda,
                        int64_t strideA, const float *B, int64_t ldb, int64_t strideB, float *C,
                        int64_t ldc, int batch, float *workspace, eap_stream_t stream);

/* C_z[M,N] = A[M,K] * B_z[N,K]^T (the forward contraction of BasicSO3Conv.forward, vgtk/vgtk/so3conv/modules.py:L48-55,
 * with the grouped tensor kept transposed: both operands k-contiguous, A shared by the batch) with fp32 operands, fp32
 * accumulation and fp32-accurate products on the bf16 matrix cores: every operand value is split exactly into three bf16
 * values on the fly and each product taken as the six largest of the nine partial products (the dropped ones are below
 * the rounding of one fp32 product) -- csrc/gemm_bf16x3.hip.  Needs M >= 128, N >= 256, M and N multiples of 128, K % 16 == 0, lda / ldb /
 * strideB multiples of 4, 16-byte aligned bases: eap_gemm_bf16x3_f32_supported tells (1 / 0). */
int eap_gemm_bf16x3_f32_supported(int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb,
                                  int64_t strideB);
int eap_gemm_bf16x3_f32(int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t strideB,
                        float *C, int64_t ldc, int64_t strideC, int batch, eap_stream_t stream);
/* 1 (default): for K >= 1024 the operand shared by the batch (the weights) is split once per call into a stream-ordered
 * scratch buffer (hipMallocAsync on the launch stream, 8 bytes per element, released after the product) instead of once per
 * k-tile by every workgroup; 2: for every shape; 0: never (split inside the k-loop like the other operand).  Bit-identical
 * results.  Returns the previous setting; any other argument only queries. */
int eap_gemm_bf16x3_presplit(int on);
/* the same product with B_z row-major [K, N] ("NN": W [O, C] times x_z [C, P*A], the pointwise contraction behind every
 * 1 x 1 conv of the blocks and heads -- torch.matmul / nn.Conv2d(1) in SPConvNets/utils/base_so3conv.py) */
int eap_gemm_bf16x3_nn_f32_supported(int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb,
                                     int64_t strideB);
int eap_gemm_bf16x3_nn_f32(int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t strideB,
                           float *C, int64_t ldc, int64_t strideC, int batch, eap_stream_t stream);
/* The two products above with a per-row epilogue: C = leaky_relu(scale[row] * (A B) + shift[row], slope) (+ residual [batch][M][ldc],
 * may be null): an inference-mode nn.BatchNorm2d + activation (+ the separable block's skip sum,
 * SPConvNets/utils/base_so3poseconv.py:L214-221, L319-328) folded into the contraction.  transB = 1: B k-contiguous (as
 * eap_gemm_bf16x3_f32), 0: B row-major (as eap_gemm_bf16x3_nn_f32); same operand requirements. */
int eap_gemm_bf16x3_ep_f32(int transB, int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t strideB,
                           float *C, int64_t ldc, int64_t strideC, int batch, const float *scale, const float *shift, float slope,
                           const float *residual, int64_t strideRes, eap_stream_t stream);
/* C[M,N] = sum_z A_z[M,K] B_z[N,K]^T on the split kernel (the weight gradient of the pointwise contraction, dW = sum over the
 * clouds of dY_z x_z^T): every (item, k-slab) pair writes its partial into `workspace` (eap_gemm_bf16x3_reduce_workspace
 * floats, 16-byte aligned), a second kernel sums them in a fixed order. */
int eap_gemm_bf16x3_reduce_f32_supported(int M, int N, int K, const float *A, int64_t lda, int64_t strideA, const float *B,
                                         int64_t ldb, int64_t strideB, int64_t ldc);
int64_t eap_gemm_bf16x3_reduce_workspace(int M, int N, int K, int batch);
int eap_gemm_bf16x3_reduce_f32(int M, int N, int K, const float *A, int64_t lda, int64_t strideA, const float *B, int64_t ldb,
                               int64_t strideB, float *C, int64_t ldc, int batch, float *workspace, eap_stream_t stream);
/* the same over a PACKED contraction axis: item z contracts over its first ncols[z] elements (int32 device words, clamped to 0 .. K); nothing
 * past them is read in A_z or B_z, a last partial k-tile is zero-filled, an item or k-slab without live elements adds zeros.  Slab count and
 * workspace as eap_gemm_bf16x3_reduce_f32; an item's slabs share ITS live prefix in equal runs of whole k-tiles. */
int eap_gemm_bf16x3_reduce_tail_f32(int M, int N, int K, const float *A, int64_t lda, int64_t strideA, const float *B, int64_t ldb,
                                    int64_t strideB, float *C, int64_t ldc, int batch, const int32_t *ncols, float *workspace,
                                    eap_stream_t stream);
/* eap_so3_intra_conv_f32 on the split kernel (nt = 12; o, p*na multiples of 128; c*nt a multiple of 16) */
int eap_so3_intra_conv_bf16x3_f32_supported(int b, int o, int c, int p, int na, int nt);
int eap_so3_intra_conv_bf16x3_f32(int b, int o, int c, int p, int na, int nt, const float *W, const float *feats,
                                  const int32_t *intra_idx, float *out, eap_stream_t stream);
/* The same contractions (torch.matmul in BasicSO3Conv.forward, vgtk/vgtk/so3conv/modules.py:L48-55; the 1 x 1 convs; the intra
 * conv, so3conv/functional.py:L2553-2602) with TWO fp16 planes per operand instead of three bf16 planes: three matrix
 * instructions per k-tile instead of six (round 4).  Every ROW of A and every COLUMN of B_z is first multiplied by a power of
 * two that puts its largest magnitude (or a bound on it) at 2^14..2^15 -- the scales come off again per output row and column
 * in the epilogue --, then split x = h + l, h = fp16(x), l = fp16(x - h), round to nearest: |x - h - l| <= 2^-23 |x| (rms
 * 2^-25 |x|) for elements down to 2^-17 of that magnitude, <= 2^-40 of it below; the products h h' + h l' + l h' are exact in
 * the fp32 accumulator, l l' (<= 2^-22 |x x'|) is dropped.  tests/test_gpu_split_planes.py bounds the error against fp64 by that
 * of the fp32-MFMA kernel on the same operands, per output element.  The magnitudes are device words holding the bit pattern
 * of a non-negative float (unsigned maxima: order-independent), so nothing waits for the host:
 *   eap_absmax_rows_f32        x [batch][rows][cols] (row pitch ld, item stride `stride`; cols / ld / stride multiples of 4, 16-byte
 *                              aligned) -> out [batch][rows]: largest magnitude of every row
 *   eap_absmax_colgroups_f32   the same tensor -> out [batch][cols / grp]: largest magnitude over the rows and over each group of grp
 *                              consecutive columns (grp a multiple of 4 dividing cols)
 *   eap_so3_grouped_bound_f32  a bound on the inter conv's grouped tensor per point, without a pass over it: X[c,k,p,a] is a sum over
 *                              the nn neighbours of a feature times a weight in [0, 1] (so3conv/functional.py:L1112-1261), so
 *                              |X[.,.,p,.]| <= sum_n point_max[idx[p,n]] with point_max [b][n_sup] = eap_absmax_colgroups_f32 of
 *                              feats [b][c][n_sup*na] in groups of na; idx int32 [b,p,nn] (entries >= n_sup: no neighbour) -> out [b][p]
 *   eap_gemm_f16x2_f32         C_z = A B_z, trans_b = 1: B_z [N,K] k-contiguous (operands as eap_gemm_bf16x3_f32_supported says), 0: B_z
 *                              [K,N] row-major (eap_gemm_bf16x3_nn_f32_supported); abs_a [M] = eap_absmax_rows_f32 of A; abs_b
 *                              [batch][N / grp_b]: float(word) * mult_b >= the largest magnitude in those grp_b columns of C's operand
 *                              B_z; scale / shift / slope / residual: the row epilogue of eap_gemm_bf16x3_ep_f32, or scale = shift = NULL
 *   eap_so3_intra_conv_f16x2_f32   eap_so3_intra_conv_bf16x3_f32 likewise: abs_w [o] of W's rows, abs_f [b][p] = per-point maxima of feats
 *                              (eap_absmax_colgroups_f32 in groups of na: a column gathers 12 anchors of its point) */
int eap_absmax_rows_f32(const float *x, int batch, int rows, int cols, int64_t ld, int64_t stride, int32_t *out_bits, eap_stream_t stream);
int eap_absmax_colgroups_f32(const float *x, int batch, int rows, int cols, int64_t ld, int64_t stride, int grp, int32_t *out_bits,
                             eap_stream_t stream);
int eap_so3_grouped_bound_f32(int b, int p, int nn, int n_sup, const int32_t *point_max_bits, const int32_t *idx, int32_t *out_bits,
                              eap_stream_t stream);
int eap_gemm_f16x2_f32(int trans_b, int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t strideB,
                       float *C, int64_t ldc, int64_t strideC, int batch, const int32_t *abs_a, const int32_t *abs_b, int grp_b, float mult_b,
                       const float *scale, const float *shift, float slope, const float *residual, int64_t strideRes,
                       eap_stream_t stream);
/* eap_gemm_f16x2_f32 with trans_b = 0 and no epilogue for ONE 128-row tile and a long contraction (M = 128, K >= 1024: the dense layers'
 * feature gradient), the contraction cut into `slabs` runs of whole k-tiles so that (item, slab) pairs fill the device: every pair
 * writes an [M,N] partial to workspace [slab][item][M,N], the partials are summed in slab order (no atomics, bit-identical from run to
 * run; a summation order other than the one-slab kernel's).  slabs = 1 is eap_gemm_f16x2_f32 bit for bit and needs no workspace.
 *   eap_gemm_f16x2_splitk_slabs      the count the entry picks for slabs = 0: the smallest divisor of K / 16 leaving slabs of >= 16 k-tiles
 *                                    with column tiles x batch x slabs >= 4 x cus (cus <= 0: the current device's CUs), at most 64 -- and 1
 *                                    unless that cuts rounds x k-tiles per workgroup (one workgroup per CU) by a quarter at least
 *   eap_gemm_f16x2_splitk_workspace  floats of workspace for a slab count (0 for one slab)
 * More than one slab: strideC = M ldc, ldc % 4 == 0, C and workspace 16-byte aligned. */
int eap_gemm_f16x2_splitk_slabs(int M, int N, int K, int batch, int cus);
int64_t eap_gemm_f16x2_splitk_workspace(int M, int N, int batch, int slabs);
int eap_gemm_f16x2_splitk_f32(int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t strideB,
                              float *C, int64_t ldc, int64_t strideC, int batch, const int32_t *abs_a, const int32_t *abs_b, int grp_b,
                              float mult_b, int slabs, float *workspace, int64_t workspace_floats, eap_stream_t stream);
/* the same over PACKED columns: item z has ncols[z] live columns (int32 device words, multiples of 4, clamped to 0 .. N).  A column tile that
 * starts at or past them returns before any load, the last live tile masks its loads and stores, the sum of the slabs stops there: nothing
 * past ncols[z] is read in B_z or abs_b or written in C_z.  The live columns get the bits of eap_gemm_f16x2_splitk_f32. */
int eap_gemm_f16x2_splitk_tail_f32(int M, int N, int K, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t strideB,
                                   float *C, int64_t ldc, int64_t strideC, int batch, const int32_t *abs_a, const int32_t *abs_b, int grp_b,
                                   float mult_b, int slabs, float *workspace, int64_t workspace_floats, const int32_t *ncols,
                                   eap_stream_t stream);
int eap_so3_intra_conv_f16x2_f32(int b, int o, int c, int p, int na, int nt, const float *W, const float *feats,
                                 const int32_t *intra_idx, float *out, const int32_t *abs_w, const int32_t *abs_f, eap_stream_t stream);


/* The same GEMMs with both operands fed by global -> LDS DMA through a three-stage ring (csrc/gemm_dma_f32.hip);
 * conventions of eap_gemm_f32 / eap_gemm_f32_reduce.  Needs K % 16 == 0, leading dimensions and batch strides
 * multiples of 4, 16-byte aligned bases, and a multiple of 4 rows for an operand whose rows are contiguous
 * (transA = 1: M % 4 == 0; transB = 0: N % 4 == 0); eap_gemm_dma_f32_supported tells (1 / 0). */
int eap_gemm_dma_f32_supported(int transA, int transB, int M, int N, int K, const float *A, int64_t lda,
                               int64_t strideA, const float *B, int64_t ldb, int64_t strideB);
int eap_gemm_dma_f32(int transA, int transB, int M, int N, int K, const float *A, int64_t lda, int64_t strideA,
                     const float *B, int64_t ldb, int64_t strideB, float *C, int64_t ldc, int64_t strideC,
                     int batch, eap_stream_t stream);
int64_t eap_gemm_dma_f32_reduce_workspace(int M, int N, int K, int batch);
int eap_gemm_dma_f32_reduce(int transA, int transB, int M, int N, int K, const float *A, int64_t lda,
                            int64_t strideA, const float *B, int64_t ldb, int64_t strideB, float *C, int64_t ldc,
                            int batch, float *workspace, eap_stream_t stream);
/* C[M,N] = sum_z A_z[M,K] B_z[N,K]^T for a SMALL output and a long contraction (M <= 64, N <= 32, K >= 4096; both operands
 * k-contiguous, 16-byte aligned, pitches and strides multiples of 4 floats): the first layer's weight gradient
 * dW[64, 24] = sum_b dY_b X_b^T (textbook backward of so3conv/modules.py:L48-55 at C = 1).  A streaming reduction -- 16-byte
 * loads straight into the MFMA operand registers, per-wave partial sums added in a fixed order (bit-reproducible); the tiled
 * kernels pad this product to 5 % useful work.  workspace: eap_gemm_skinny_reduce_workspace floats. */
int eap_gemm_skinny_reduce_f32_supported(int M, int N, int K, const float *A, int64_t lda, int64_t strideA, const float *B,
                                         int64_t ldb, int64_t strideB);
int64_t eap_gemm_skinny_reduce_workspace(int M, int N, int K, int batch);
int eap_gemm_skinny_reduce_f32(int M, int N, int K, const float *A, int64_t lda, int64_t strideA, const float *B, int64_t ldb,
                               int64_t strideB, float *C, int64_t ldc, int batch, float *workspace, eap_stream_t stream);

/* ---- blocked intermediate: the forward's grouped tensor X with coalesced row-end stores --------
 * X_blocked[b][p][a/4][c][k][4] holds the same numbers as X[b][c][k][p][a].  The grouping kernels
 * write 384 contiguous bytes per (channel, anchor quad) instead of 16-byte pieces 983 KB apart, and
 * the contraction GEMMs read it as a B operand "blocked by 4" along P*A.  Internal to the fused
 * conv (vgtk.so3conv.functional._InterConv); the reference-layout entries above stay as they are. */
int eap_so3_inter_group_fwd_can_block(int c, int n, int na, int ks, int has_mult, int has_flag);
int eap_so3_inter_group_fwd_xb_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                   const float *feats, const int32_t *idx, const float *gx,
                                   const float *rk, const uint8_t *mult, const int32_t *nonident,
                                   float *out, eap_stream_t stream);
/* same, output transposed: out[b][p*na + a][c*ks + k] (a plain row-major [P*A, C*K] matrix) */
int eap_so3_inter_group_fwd_t_f32(int b, int c, int p, int n, int nn, int na, int ks, float sigma,
                                  const float *feats, const int32_t *idx, const float *gx,
                                  const float *rk, const uint8_t *mult, const int32_t *nonident,
                                  float *out, eap_stream_t stream);
/* eap_gemm_f32 / eap_gemm_f32_reduce with B blocked by 4: element (row r of b_block_rows, position x)
 * at (x >> 2) * b_block_rows * 4 + r * 4 + (x & 3); b_block_rows = K (transB = 0) or N (transB = 1). */
int eap_gemm_f32_xb(int transA, int transB, int M, int N, int K, const float *A, int64_t lda,
                    int64_t strideA, const float *B, int64_t b_block_rows, int64_t strideB, float *C,
                    int64_t ldc, int64_t strideC, int batch, eap_stream_t stream);
int eap_gemm_f32_reduce_xb(int transA, int transB, int M, int N, int K, const float *A, int64_t lda,
                           int64_t strideA, const float *B, int64_t b_block_rows, int64_t strideB,
                           float *C, int64_t ldc, int batch, float *workspace, eap_stream_t stream);

/* Intra SO(3) conv, forward, as an implicit GEMM (no [b,c,t,p,na] gathered tensor):
 * out[b,o,p,a] = sum_{c,t} W[o, c*nt + t] * feats[b, c, p, intra_idx[a*nt + t]]
 * (so3conv/functional.py:L2553-2602 intra_so3conv_grouping + so3conv/modules.py:L48-55 BasicSO3Conv).
 * W [o, c*nt], feats [b,c,p,na], intra_idx int32 [na,nt] (na a multiple of 4, <= 64; nt <= 16), out [b,o,p,na]. */
int eap_so3_intra_conv_f32(int b, int o, int c, int p, int na, int nt, const float *W, const float *feats,
                           const int32_t *intra_idx, float *out, eap_stream_t stream);

/* ---- SO(3) intra convolution on the (na, nr) anchor axis of `use_2d` ------------------------------------------
 * IntraSO3Conv2D (so3conv/modules.py:L350-373): the anchor axis is na icosahedral anchors times nr in-plane residual rotations, the
 * residual innermost, and the 12-tap gather acts on the na-axis alone (intra_so3conv_grouping_2D, so3conv/functional.py:L2606-2627).
 * Limits of every entry below: nr = 4 (the residuals of one anchor are one 16-byte quad), na <= 64, nt <= 16 (nt = 12 on the split
 * kernel); anything else returns hipErrorInvalidValue before a pointer is touched; an empty problem returns 0. */

/* so3_intra_group2d_fwd: intra_so3conv_grouping_2D, so3conv/functional.py:L2606-2627.
 * feats [b,c,p,na,nr], intra_idx int32 [na,t] -> out [b,c,t,p,na,nr] = feats[b,c,p,intra_idx[a,t],r]; feats and out 16-byte aligned. */
int eap_so3_intra_group2d_fwd_f32(int b, int c, int p, int na, int nr, int t, const float *feats, const int32_t *intra_idx, float *out,
                                  eap_stream_t stream);
/* transpose: gout [b,c,t,p,na,nr] -> gfeats [b,c,p,na,nr], every element the sum of the quads that read it, in table order
 * (no float atomics: bit-identical run to run). */
int eap_so3_intra_group2d_bwd_f32(int b, int c, int p, int na, int nr, int t, const float *gout, const int32_t *intra_idx, float *gfeats,
                                  eap_stream_t stream);
/* The layer as an implicit GEMM (no [b,c,t,p,na,nr] gathered tensor):
 * out[b,o,p,a,r] = sum_{c,t} W[o, c*nt + t] * feats[b, c, p, intra_idx[a*nt + t], r]
 * (so3conv/functional.py:L2606-2627 intra_so3conv_grouping_2D + so3conv/modules.py:L48-55 BasicSO3Conv).
 * W [o, c*nt], feats [b,c,p,na,nr], intra_idx int32 [na,nt], out [b,o,p,na,nr]. */
int eap_so3_intra_conv2d_f32(int b, int o, int c, int p, int na, int nr, int nt, const float *W, const float *feats,
                             const int32_t *intra_idx, float *out, eap_stream_t stream);
/* the same on the split kernel (nt = 12; o and p*na*nr multiples of 128; c*nt a multiple of 16; W 16-byte aligned), three bf16 planes or
 * two fp16 planes: abs_w [o] = eap_absmax_rows_f32 of W, abs_f [b][p] = eap_absmax_colgroups_f32 of feats [b][c][p*na*nr] in groups of
 * na*nr (a column gathers 12 quads of its point). */
int eap_so3_intra_conv2d_split_supported(int b, int o, int c, int p, int na, int nr, int nt);
int eap_so3_intra_conv2d_bf16x3_f32(int b, int o, int c, int p, int na, int nr, int nt, const float *W, const float *feats,
                                    const int32_t *intra_idx, float *out, eap_stream_t stream);
int eap_so3_intra_conv2d_f16x2_f32(int b, int o, int c, int p, int na, int nr, int nt, const float *W, const float *feats,
                                   const int32_t *intra_idx, float *out, const int32_t *abs_w, const int32_t *abs_f, eap_stream_t stream);

/* ---- chamfer distance (extensions/chamfer_dist) ------------------------------------------- */

/* chamfer.forward: chamfer_cuda.cpp:L22-25, chamfer.cu:L15-171.
 * xyz1 [b,n,3], xyz2 [b,m,3] -> dist1 [b,n], dist2 [b,m], idx1 int32 [b,n], idx2 int32 [b,m]. */
int eap_chamfer_fwd_f32(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1,
                        float *dist2, int32_t *idx1, int32_t *idx2, eap_stream_t stream);
/* the same in float64 (chamfer_cuda.cpp:L22-25, chamfer.cu:L15-171 with the scalar type changed, as the header of the reference's
 * extensions/chamfer_dist/test.py asks for): one rounding per operation, (dx*dx + dy*dy) + dz*dz, first minimum wins. */
int eap_chamfer_fwd_f64(int b, int n, int m, const double *xyz1, const double *xyz2, double *dist1,
                        double *dist2, int32_t *idx1, int32_t *idx2, eap_stream_t stream);
/* chamfer.backward: chamfer_cuda.cpp:L27-34, chamfer.cu:L173-231.
 * -> gxyz1 [b,n,3], gxyz2 [b,m,3] (zero-initialised by the call).  A scatter with float atomicAdd, as the reference's: a point that
 * several points of the other cloud pick is summed in an order that differs between runs (eap_chamfer_bwd_ordered_* does not). */
int eap_chamfer_bwd_f32(int b, int n, int m, const float *xyz1, const float *xyz2,
                        const int32_t *idx1, const int32_t *idx2, const float *g1, const float *g2,
                        float *gxyz1, float *gxyz2, eap_stream_t stream);
/* chamfer.backward (chamfer_cuda.cpp:L27-34, chamfer.cu:L173-231) as a gather with a fixed summation order: no atomics, bit-identical
 * run to run, every output element written once (no zero-initialisation).  With v1[i] = (g1[i]*2) * (xyz1[i] - xyz2[idx1[i]]) and
 * v2[j] = (g2[j]*2) * (xyz2[j] - xyz1[idx2[j]]):
 *   gxyz1[b,i] = ((0 + v1[i]) + sum over j ascending with idx2[b,j] == i of (-v2[j]))
 *   gxyz2[b,j] = ((0 + sum over i ascending with idx1[b,i] == j of (-v1[i])) + v2[j])
 * -- the order of a serial run of the reference's two kernel launches.  An index outside its cloud contributes nothing and is not
 * dereferenced.  O(n * m) index compares per direction (the forward's loop shape). */
int eap_chamfer_bwd_ordered_f32(int b, int n, int m, const float *xyz1, const float *xyz2,
                                const int32_t *idx1, const int32_t *idx2, const float *g1, const float *g2,
                                float *gxyz1, float *gxyz2, eap_stream_t stream);
int eap_chamfer_bwd_ordered_f64(int b, int n, int m, const double *xyz1, const double *xyz2,
                                const int32_t *idx1, const int32_t *idx2, const double *g1, const double *g2,
                                double *gxyz1, double *gxyz2, eap_stream_t stream);

/* The reconstruction distances over the orbit (SPConvNets/models/unsup_seg_so3_pose_conv_pn_38_multi_stage.py:L1341-1361 per slot with
 * its membership mask, L429-440 for the global alignment without one) as a shared-target search: g = b*s groups (s slots per cloud, the
 * cloud of group i is i / s) of a candidate clouds of m points, recon [g,a,m,3], all compared with the group's ONE input cloud, ori
 * [g/s,3,n] planar; member uint8 [g,n] flags the points of the group's slot, NULL = every point is in (the masked outputs are then not
 * written and may be NULL).  Squared distances as eap_chamfer_fwd_*: (dx*dx + dy*dy) + dz*dz, one rounding per operation, first
 * minimum wins.
 *   r2o_all [g,a,m], r2o_all_idx int32 [g,a,m]   min over the n points and its index
 *   r2o_in  [g,a,m], r2o_in_idx  int32 [g,a,m]   the same over the flagged points; (99999, -1) where the group has none
 *   o2r_all [g,a,n], o2r_idx     int32 [g,a,n]   min over the m points of candidate cloud (g,a) and its index
 *   o2r_in  [g,a,n]                              member ? o2r_all : 99999
 * a, m, n, s >= 1, s divides g, every tensor below 2^31 elements; g <= 0 returns at once. */
int eap_orbit_chamfer_fwd_f32(int g, int s, int a, int m, int n, const float *recon, const float *ori, const uint8_t *member,
                              float *r2o_all, int32_t *r2o_all_idx, float *r2o_in, int32_t *r2o_in_idx, float *o2r_all,
                              int32_t *o2r_idx, float *o2r_in, eap_stream_t stream);
int eap_orbit_chamfer_fwd_f64(int g, int s, int a, int m, int n, const double *recon, const double *ori, const uint8_t *member,
                              double *r2o_all, int32_t *r2o_all_idx, double *r2o_in, int32_t *r2o_in_idx, double *o2r_all,
                              int32_t *o2r_idx, double *o2r_in, eap_stream_t stream);
/* The gradient of those maps with respect to recon (...pn_38_multi_stage.py:L1341-1361, L429-440: what autograd sends through the
 * reference's min / mean), a gather with a fixed summation order: no atomics, bit-identical run to run, grecon [g,a,m,3] written once.
 *   grecon[g,a,j] = ((0 + own_all) + own_in) + sum over i ascending with o2r_idx[g,a,i] == j of
 *                   (2 * (g_o2r_all[g,a,i] + member[g,i] * g_o2r_in[g,a,i])) * (recon[g,a,j] - ori[i])
 *   own_x = (2 * g_r2o_x[g,a,j]) * (recon[g,a,j] - ori[r2o_x_idx[g,a,j]])
 * An index outside its range (the -1 of an empty slot) contributes nothing and is not dereferenced.  member NULL: the masked index
 * and gradients are not read and may be NULL.  The input cloud gets no gradient from this entry. */
int eap_orbit_chamfer_bwd_f32(int g, int s, int a, int m, int n, const float *recon, const float *ori, const uint8_t *member,
                              const int32_t *r2o_all_idx, const int32_t *r2o_in_idx, const int32_t *o2r_idx, const float *g_r2o_all,
                              const float *g_r2o_in, const float *g_o2r_all, const float *g_o2r_in, float *grecon, eap_stream_t stream);
int eap_orbit_chamfer_bwd_f64(int g, int s, int a, int m, int n, const double *recon, const double *ori, const uint8_t *member,
                              const int32_t *r2o_all_idx, const int32_t *r2o_in_idx, const int32_t *o2r_idx, const double *g_r2o_all,
                              const double *g_r2o_in, const double *g_o2r_all, const double *g_o2r_in, double *grecon, eap_stream_t stream);

/* ---- block-layer epilogue: BatchNorm2d (batch statistics) + leaky_relu ------------------------- */
/* SPConvNets/utils/base_so3poseconv.py:L214-221 (`feat = self.norm(x.feats); feat = self.relu(feat)`),
 * SURVEY.md 8(f) row 1.  x, y, gy, gx: [b, c, n] (n = P*A, a multiple of 4), contiguous.
 * Reductions are returned as per-block partials [c][b][eap_bn_act_segments(n)] for the caller to
 * sum in a fixed order (deterministic). */
int eap_bn_act_segments(int64_t n);
/* partial sums of (x - pivot_c) and (x - pivot_c)^2, pivot_c = x[0, c, 0] */
int eap_bn_stats_f32(int b, int c, int64_t n, const float *x, float *psum, float *psq, eap_stream_t stream);
/* y = leaky_relu(x * scale[c] + shift[c], slope) */
int eap_bn_act_fwd_f32(int b, int c, int64_t n, float slope, const float *x, const float *scale,
                       const float *shift, float *y, eap_stream_t stream);
/* y = leaky_relu(x * scale[c] + shift[c], slope) + res: the separable block's skip-add
 * (SPConvNets/utils/base_so3poseconv.py:L319-328) in the same pass; res [b, c, n] */
int eap_bn_act_add_fwd_f32(int b, int c, int64_t n, float slope, const float *x, const float *scale,
                           const float *shift, const float *res, float *y, eap_stream_t stream);
/* partial sums of g and g * xhat,  g = gy * (x*scale+shift > 0 ? 1 : slope),  xhat = (x - mean) * invstd */
int eap_bn_act_bwd_reduce_f32(int b, int c, int64_t n, float slope, const float *gy, const float *x,
                              const float *scale, const float *shift, const float *mean,
                              const float *invstd, float *pg, float *pgx, eap_stream_t stream);
/* gx = scale[c] * g - k2[c] - xhat * k3[c] */
int eap_bn_act_bwd_apply_f32(int b, int c, int64_t n, float slope, const float *gy, const float *x,
                             const float *scale, const float *shift, const float *mean,
                             const float *invstd, const float *k2, const float *k3, float *gx,
                             eap_stream_t stream);
/* eap_bn_act_bwd_apply_f32 for rows of [points][na] that ALSO leaves max |gx| per (cloud, channel, anchor) in rowmax uint32 [b,c,na]
 * (float bit patterns): what eap_so3_dense_split_f32 takes instead of its own pass over the gradient. */
int eap_bn_act_bwd_apply_rowmax_f32(int b, int c, int64_t n, int na, float slope, const float *gy, const float *x,
                                    const float *scale, const float *shift, const float *mean, const float *invstd,
                                    const float *k2, const float *k3, float *gx, uint32_t *rowmax, eap_stream_t stream);
/* the reduction pass of the BatchNorm + leaky_relu backward from the layer's OUTPUT y' (see the conv + BatchNorm node above): partials of sum(g),
 * sum(g xhat) [c][b * eap_bn_act_fromy_blocks(n, na)] and the largest |g|, |xhat| per (cloud, channel, anchor) [b,c,na] (float bit patterns) */
int eap_bn_act_fromy_blocks(int64_t n, int na);
int eap_bn_act_bwd_reduce_fromy_f32(int b, int c, int64_t n, int na, float slope, const float *gy, const float *y, const float *beta,
                                    const float *inv_gamma, float *pg, float *pgx, uint32_t *gmax, uint32_t *xmax, eap_stream_t stream);

/* Per-cloud statistics over a point subset: the pose heads run their unary stacks once per cloud on the cloud's member
 * points (`for i_bz in range(bz): ...` SPConvNets/models/..pn_38_multi_stage.py:L706-830, the head's BatchNorm2d layers
 * SPConvNets/utils/base_so3conv.py: SO3OutBlockRTWithMaskSep), i.e. BatchNorm statistics per (cloud, channel) over the
 * members.  Batched form: a row is [points][na], mask [b, points] holds 0 / 1; scale, shift, mean, invstd, k2, k3 are
 * [b, c]; every point is normalised, the statistics and the backward's two correction terms see members only. */
/* partial sums [c][b][segments] of mask * (x - pivot_c) and mask * (x - pivot_c)^2, pivot_c = x[0, c, 0] */
int eap_bn_stats_masked_f32(int b, int c, int64_t n, int na, const float *x, const float *mask, float *psum, float *psq,
                            eap_stream_t stream);
/* y = leaky_relu(x * scale[b,c] + shift[b,c], slope) */
int eap_bn_act_cloud_fwd_f32(int b, int c, int64_t n, float slope, const float *x, const float *scale, const float *shift,
                             float *y, eap_stream_t stream);
/* partial sums of g and g * xhat over ALL points of the row, statistics per (cloud, channel) */
int eap_bn_act_cloud_bwd_reduce_f32(int b, int c, int64_t n, float slope, const float *gy, const float *x, const float *scale,
                                    const float *shift, const float *mean, const float *invstd, float *pg, float *pgx,
                                    eap_stream_t stream);
/* gx = scale[b,c] * g - mask * (k2[b,c] + xhat * k3[b,c]);  mask may be null (all ones) */
int eap_bn_act_cloud_bwd_apply_f32(int b, int c, int64_t n, int na, float slope, const float *gy, const float *x,
                                   const float *scale, const float *shift, const float *mean, const float *invstd,
                                   const float *k2, const float *k3, const float *mask, float *gx, eap_stream_t stream);

/* ---- pointwise contraction with 1-4 output channels (csrc/narrow_contract.hip) --------------------------------- */
/* y[b,o,n] = sum_c W[o,c] x[b,c,n], o <= 4, c <= 2048, n a multiple of 4: the last layer of the pose head's dense translation
 * branch (nn.Conv2d(c, 3 * num_heads, 1), SPConvNets/models/model_utils.py:L537-552) and the attention logit of
 * InvPPOutBlockOurs (nn.Conv2d(c, 1, 1), SPConvNets/utils/base_so3conv.py:L905-912) as streaming passes over x. */
int eap_narrow_contract_supported(int b, int o, int c, int64_t n);
int eap_narrow_contract_fwd_f32(int b, int o, int c, int64_t n, const float *W, const float *x, float *y, eap_stream_t stream);
/* dx[b,c,n] = sum_o W[o,c] g[b,o,n] */
int eap_narrow_contract_dx_f32(int b, int o, int c, int64_t n, const float *W, const float *g, float *dx, eap_stream_t stream);
/* dW[o,c] = sum_{b,n} g[b,o,n] x[b,c,n] as eap_narrow_contract_dw_slabs(n) * b partials [slab][b][o][c] for the caller to sum
 * in order (deterministic) */
int eap_narrow_contract_dw_slabs(int64_t n);
int eap_narrow_contract_dw_f32(int b, int o, int c, int64_t n, const float *g, const float *x, float *partial, eap_stream_t stream);

/* ---- first inter conv layer + training-mode BatchNorm + leaky_relu without the conv output (csrc/narrow_conv.hip) -------- */
/* y[b,o,n] = sum_k W[o,k] x[b,k,n] with ck = C*K <= 32 contraction indices (the 1 -> 64 layer: ck = 24; vgtk/vgtk/so3conv/modules.py:L48-55
 * followed by `feat = relu(norm(x.feats))`, SPConvNets/utils/base_so3poseconv.py:L205-222) is recomputed from the grouped input x [b, ck, n]
 * (reference layout, n = P*A) in every pass instead of being stored.  Every entry refuses, before any device call: ck outside 1..32, o not a
 * multiple of 32, n not a multiple of 4 (or >= 2^25), x / gy / y (and scale / shift of the forward) not 16-byte aligned.
 * Reductions come as per-block partials [o][b * eap_narrow_conv_segments(n)] for the caller to sum in a fixed order (deterministic). */
int eap_narrow_conv_segments(int64_t n);
/* partial sums of (y - pivot_o) and (y - pivot_o)^2; pivot [o] (written) = y[0, o, 0], a function of the data alone */
int eap_narrow_conv_stats_f32(int b, int o, int ck, int64_t n, const float *W, const float *x, float *pivot, float *psum, float *psq,
                              eap_stream_t stream);
/* y' [b,o,n] = leaky_relu(scale[o] * y + shift[o], slope) */
int eap_narrow_conv_bnact_fwd_f32(int b, int o, int ck, int64_t n, float slope, const float *W, const float *x, const float *scale,
                                  const float *shift, float *y, eap_stream_t stream);
/* partial sums of g and g * xhat as eap_bn_act_bwd_reduce_f32 leaves them, from gy = dL/dy' and the recomputed y */
int eap_narrow_conv_bwd_reduce_f32(int b, int o, int ck, int64_t n, float slope, const float *gy, const float *x, const float *W,
                                   const float *scale, const float *shift, const float *mean, const float *invstd, float *pg, float *pgx,
                                   eap_stream_t stream);
/* dW [o, ck] = sum_{b,n} gx x^T, gx = scale g - k2 - xhat k3 (eap_bn_act_bwd_apply_f32's formula) formed in registers; partial: scratch of
 * b * eap_narrow_conv_segments(n) slabs of o * ck floats, added in slab order (no float atomics) */
int eap_narrow_conv_bwd_dw_f32(int b, int o, int ck, int64_t n, float slope, const float *gy, const float *x, const float *W,
                               const float *scale, const float *shift, const float *mean, const float *invstd, const float *k2,
                               const float *k3, float *partial, float *dW, eap_stream_t stream);

/* ---- the per-channel bookkeeping of the conv + BatchNorm + leaky_relu nodes (csrc/norm_fold.hip) ------------------------ */
/* Between the big kernels of a node stand a few thousand float64 operations on [o], [b,o,na] and [b,p] tensors; written as tensor expressions
 * they are 10 - 35 launches per site.  Each entry below is that arithmetic in one launch (two where a reduction follows a reduction), operation
 * for operation; sums over partials are taken in float64 by one wave per channel in a fixed order (lane l adds partials l, l + 64, ..., then a
 * fixed tree): deterministic.  Every entry refuses a null pointer, a non-positive size and a size beyond the launch limits before it launches
 * (hipErrorInvalidValue, the condition in eap_last_error()).  float64 scalars travel as their bit patterns (`*_bits`): the vocabulary has no double.
 *
 * eap_norm_fold_train_f32 replaces TrainEpilogue.moments without an exchange (batch_moments, update_running_stats, affine_from_moments of
 * vgtk/so3conv/blocks.py = nn.BatchNorm2d's training forward, SPConvNets/utils/base_so3poseconv.py:L214-221): ps, pq float [o, parts] partial sums
 * of (y - pivot) and its square, pivot[ch * pivot_stride], count elements per channel, gamma, beta [o] -> scale, shift float [o]
 * (y' = scale y + shift), mean, invstd double [o], beta_copy, inv_gamma float [o] (0 where gamma == 0); running_mean / running_var float [o]
 * updated in place with the unbiased variance (both null: none kept). */
int eap_norm_fold_train_f32(int o, int parts, int64_t pivot_stride, int64_t count, int64_t eps_bits, int64_t momentum_bits, const float *ps,
                            const float *pq, const float *pivot, const float *gamma, const float *beta, float *running_mean, float *running_var,
                            float *scale, float *shift, double *mean, double *invstd, float *beta_copy, float *inv_gamma, eap_stream_t stream);
/* replaces the sums and coefficients at the top of _backward_dense / _backward_narrow (vgtk/so3conv/functional.py): pg, pgx float [o, parts] partial
 * sums of g and g xhat, k1 [o] the forward's scale -> dgamma = sum g xhat, dbeta = sum g, k2 = k1 sum g / count, k3 = k1 sum g xhat / count (float [o]).
 * The dense node also hands beta, inv_gamma [o] and the row maxima gmax, xmax float [b,o,na] and gets coef float [5,o] = k1, k2, k3, beta, inv_gamma,
 * bound [b,o,na] = |k1| gmax + |k2| + |k3| xmax and colmax [b,na] = max over o of bound (a second launch); the narrow node passes these seven null. */
int eap_norm_fold_bwd_f32(int o, int parts, int b, int na, int64_t count, const float *pg, const float *pgx, const float *k1, const float *beta,
                          const float *inv_gamma, const float *gmax, const float *xmax, float *dgamma, float *dbeta, float *k2, float *k3, float *coef,
                          float *bound, float *colmax, eap_stream_t stream);
/* replaces the z_bound block of _backward_dense: words float [b, ldz / 4], word (a rp + r) / 4 = the largest of its four columns'
 * colmax[b,a] * clamp(cnt[b,r], 0, p) (cnt int32, rows cnt_stride apart; 0 for r >= n_rows[b]), zero from na rp / 4 on.  rp % 4 == 0, ldz % 4 == 0. */
int eap_so3_dense_zbound_f32(int b, int na, int rp, int p, int ldz, int64_t cnt_stride, const float *colmax, const int32_t *cnt,
                             const int32_t *n_rows, float *words, eap_stream_t stream);
/* the same words for packed Z: word w of cloud i bounds columns 4 w .. 4 w + 3 = (a, r0 .. r0 + 3), a = 4 w / live16[i], r0 = 4 w % live16[i]; zero from
 * na live16[i] / 4 on.  Also writes ncols int32 [b] = na live16[i], the live prefix the tail products take.  rp % 16 == 0, ldz % 4 == 0. */
int eap_so3_dense_zbound_packed_f32(int b, int na, int rp, int p, int ldz, int64_t cnt_stride, const float *colmax, const int32_t *cnt,
                                    const int32_t *n_rows, float *words, int32_t *ncols, eap_stream_t stream);
/* replaces the reductions in front of eap_so3_dense_gplanes_f32: bound float [b,na,o] = max_{c,r} |fc4[b,c,r,a]| x (max_k sum_c |W3[(o,k),c]| x 1.0001)
 * from W3 [o ks, c] and fc4 [b,c,rp,na]; fpart float [b,c,na] and wsum float [o] are scratch (written).  na <= 128.  Two launches. */
int eap_so3_dense_gplanes_bound_f32(int b, int o, int c, int na, int ks, int rp, const float *W3, const float *fc4, float *fpart, float *wsum,
                                    float *bound, eap_stream_t stream);
/* replaces what DenseGeometry did behind its sort: order int64 [b,p] (a permutation per cloud), memb [b,p,words] (words = 16 or 32, 16-byte aligned),
 * q_xyz float [b,3,p] -> order32 int32 [b,p], memb_out and xyz_out gathered through it, pivot_pos int32 [1] = the j with order[0,j] == 0 */
int eap_so3_dense_point_order(int b, int p, int words, const int64_t *order, const uint32_t *memb, const float *q_xyz, int32_t *order32,
                              uint32_t *memb_out, float *xyz_out, int32_t *pivot_pos, eap_stream_t stream);

/* ---- heads on the backbone's [b,c,n,na] feature map ------------------------ */
/* Anchor attention pooling, InvPPOutBlockOurs.forward (SPConvNets/utils/base_so3conv.py:L905-912):
 * conf[b,n,a] = softmax_a(logits[b,n,a] * temperature), out[b,c,n] = sum_a x[b,c,n,a] conf[b,n,a].  na % 4 == 0, <= 64.
 * Backward: dx [b,c,n,na], dlogits [b,n,na] from g [b,c,n].
 * x, logits, conf (may be null), dx and dlogits are moved by 16-byte words and must be 16-byte aligned (refused otherwise); out and g
 * are not.  A logit of -inf is a masked anchor (confidence 0); NaN in x or the logits spreads to what it touches, as in torch. */
int eap_anchor_attn_pool_fwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                 float *out, float *conf, eap_stream_t stream);
int eap_anchor_attn_pool_bwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                 const float *g, float *dx, float *dlogits, eap_stream_t stream);
/* Masked point averages of every slot in one pass (SO3OutBlockRTWithMaskSep, SPConvNets/models/model_utils.py:L470-484,
 * L549-552): out[b,s,c,a] = inv_den[b,s] * sum_n mask[b,s,n] x[b,c,n,a];  ns <= 8.  Backward w.r.t. x.
 * x and out (forward), g and dx (backward) are moved by 16-byte words and must be 16-byte aligned (refused otherwise); mask and inv_den
 * are not.  Sums: a NaN in x reaches every slot of its (cloud, channel, anchor), whatever the mask (0 * NaN). */
int eap_slot_masked_mean_fwd_f32(int b, int ns, int c, int n, int na, const float *x, const float *mask,
                                 const float *inv_den, float *out, eap_stream_t stream);
int eap_slot_masked_mean_bwd_f32(int b, int ns, int c, int n, int na, const float *g, const float *mask,
                                 const float *inv_den, float *dx, eap_stream_t stream);
/* The pose heads' 'max' pooling on a point subset, `(x * mask).max(2)` (SPConvNets/models/model_utils.py:L79-80, L470-484):
 * out[b,c,a] = max_p mask[b,p] * x[b,c,p,a], arg[b,c,a] = the lowest point index attaining it (int32); one pass over x.
 * Backward: dx[b,c,p,a] = (p == arg[b,c,a]) * mask[b,p] * g[b,c,a], written for every point.
 * NaN: a product mask[b,p] * x[b,c,p,a] that is NaN (member or not: 0 * NaN, 0 * inf) makes out[b,c,a] NaN, as torch's max does, and
 * arg[b,c,a] the lowest such point; otherwise the maximum at its lowest point, -0.0 and +0.0 being equal.
 * x, out, arg (forward), g, arg, dx (backward) are moved by 16-byte words and must be 16-byte aligned (refused otherwise); mask is not. */
int eap_masked_max_fwd_f32(int b, int c, int n, int na, const float *x, const float *mask, float *out, int32_t *arg,
                           eap_stream_t stream);
int eap_masked_max_bwd_f32(int b, int c, int n, int na, const float *g, const int32_t *arg, const float *mask, float *dx,
                           eap_stream_t stream);
/* The same three pairs for wide anchor rows (the same kernels of csrc/heads.hip compiled with 64 lanes per row instead of 16): na % 4 == 0, 4 <= na <= 256 -- the 60 x 4 = 240 anchors of a `use_2d`
 * feature map.  Parameter lists, definitions, NaN / -inf / tie rules and alignment demands are those of the entries without _wide above;
 * one wavefront owns a point's anchor row (lane = 16-byte quad), the anchor reductions are 6 shuffle steps, the point sums of the slot
 * mean are chains of ceil(n / 4) fused multiply-adds folded over 4 waves in a fixed order.  No atomics, bit-identical run to run.  Other
 * anchor counts are refused ("multiple of 4, at most 256"), as are more than 8 slots and a 16-byte operand off its boundary.
 * Anchor attention pooling over the na * 4 anchors, InvPPOutBlock2DOurs.forward (SPConvNets/utils/base_so3conv.py:L994-1001), and
 * InvPPOutBlockOurs.forward (L905-912) on a `use_2d` map: */
int eap_anchor_attn_pool_wide_fwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                      float *out, float *conf, eap_stream_t stream);
int eap_anchor_attn_pool_wide_bwd_f32(int b, int c, int n, int na, float temperature, const float *x, const float *logits,
                                      const float *g, float *dx, float *dlogits, eap_stream_t stream);
/* Masked point averages of every slot, SO3OutBlockRTWithMaskSep (SPConvNets/models/model_utils.py:L470-484, L549-552): */
int eap_slot_masked_mean_wide_fwd_f32(int b, int ns, int c, int n, int na, const float *x, const float *mask,
                                      const float *inv_den, float *out, eap_stream_t stream);
int eap_slot_masked_mean_wide_bwd_f32(int b, int ns, int c, int n, int na, const float *g, const float *mask,
                                      const float *inv_den, float *dx, eap_stream_t stream);
/* The pose heads' 'max' pooling on a point subset (SPConvNets/models/model_utils.py:L79-80, L470-484); n <= 0 is refused forward, as by
 * eap_masked_max_fwd_f32: */
int eap_masked_max_wide_fwd_f32(int b, int c, int n, int na, const float *x, const float *mask, float *out, int32_t *arg,
                                eap_stream_t stream);
int eap_masked_max_wide_bwd_f32(int b, int c, int n, int na, const float *g, const int32_t *arg, const float *mask, float *dx,
                                eap_stream_t stream);
/* The last unary layer of InvOutBlockOursWithMask with the point average behind it, fused (SPConvNets/utils/base_so3conv.py:L1076-1107:
 * `F.relu(norm(linear(x)))`, the mask, PointnetSO3ConvOurs' 1x1 `embed` -- linear, so the average moves in front of it -- and the plain or
 * soft-mask weighted mean over the points).  x [b,c,n,na] the raw contraction output; scale, shift, mean, invstd, k2, k3 [b,c]; w [b,n] point
 * weights (data: 0/1 membership or soft weights); inv_den [b]; na % 4 == 0, <= 64; x, out, g, gx 16-byte aligned.  Fixed summation order.
 *   out[b,c,a] = inv_den[b] * sum_p w[b,p] * leaky_relu(x[b,c,p,a] * scale[b,c] + shift[b,c], slope);  the activated map is never written */
int eap_bn_act_cloud_mean_fwd_f32(int b, int c, int n, int na, float slope, const float *x, const float *scale, const float *shift,
                                  const float *w, const float *inv_den, float *out, eap_stream_t stream);
/* (base_so3conv.py:L1076-1107, backward) with gg = (pre > 0 ? 1 : slope) * w[b,p] * inv_den[b] * g[b,c,a], never written: the sums of gg and
 * gg * xhat over a (cloud, channel) row as eap_bn_act_cloud_mean_parts(n) partials each, pg, pgx [b, c, parts], for the caller to add in float64 */
int eap_bn_act_cloud_mean_parts(int n);
int eap_bn_act_cloud_mean_bwd_reduce_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                         const float *shift, const float *mean, const float *invstd, const float *w, const float *inv_den,
                                         float *pg, float *pgx, eap_stream_t stream);
/* (base_so3conv.py:L1076-1107, backward) gx[b,c,p,a] = scale[b,c] * gg - stat_mask[b,p] * (k2[b,c] + xhat * k3[b,c]);  stat_mask [b,n] may be
 * null (all ones) */
int eap_bn_act_cloud_mean_bwd_apply_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                        const float *shift, const float *mean, const float *invstd, const float *k2, const float *k3,
                                        const float *w, const float *inv_den, const float *stat_mask, float *gx, eap_stream_t stream);
/* The same three entries and their parts query for wide anchor rows (the same kernels of csrc/heads.hip compiled with 64 lanes per row instead of 16): na % 4 == 0, 4 <= na <= 256 -- InvOutBlockOursWithMask
 * on the 240-anchor map of a `use_2d` backbone (SPConvNets/utils/base_so3conv.py:L1076-1107; PointnetSO3ConvOurs keeps tot_anchors [240,3,3] for
 * it, L1173-1176, L1196).  Parameter lists and definitions are those of the entries without _wide above.  One wavefront owns a point's anchor
 * row (lane = 16-byte quad); a wave takes every 4th point, 4 rows in flight into 4 accumulators (fp32 chains of ceil(n / 16) terms), folded as
 * a tree, over the 4 waves in wave order (forward) or over the wave by 6 shuffle steps (reduction: eap_bn_act_cloud_mean_wide_parts(n) = 4
 * partials per (cloud, channel), one per wave).  No atomics, bit-identical run to run; the activated map and its gradient are never written.
 * Refused before any device call (hipErrorInvalidValue, the condition in eap_last_error()): n <= 0, other anchor counts ("multiple of 4, at
 * most 256"), a null pointer other than stat_mask, x / out / g / gx off a 16-byte boundary, sizes beyond the launch limits.  b <= 0 or c <= 0
 * returns 0 without touching a pointer. */
int eap_bn_act_cloud_mean_wide_fwd_f32(int b, int c, int n, int na, float slope, const float *x, const float *scale, const float *shift,
                                       const float *w, const float *inv_den, float *out, eap_stream_t stream);
int eap_bn_act_cloud_mean_wide_parts(int n);
int eap_bn_act_cloud_mean_wide_bwd_reduce_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                              const float *shift, const float *mean, const float *invstd, const float *w, const float *inv_den,
                                              float *pg, float *pgx, eap_stream_t stream);
int eap_bn_act_cloud_mean_wide_bwd_apply_f32(int b, int c, int n, int na, float slope, const float *g, const float *x, const float *scale,
                                             const float *shift, const float *mean, const float *invstd, const float *k2, const float *k3,
                                             const float *w, const float *inv_den, const float *stat_mask, float *gx, eap_stream_t stream);

/* ---- SlotAttention's per-point passes (SPConvNets/utils/slot_attention_spec_v2.py:L132-193; csrc/slot_attention.hip) -------- */
/* The per-slot LayerNorm (L149), to_k / to_v (L153-154) and the einsums (L167, L175) are linear in z[n,:] = (x[:,n] - mean[n]) * rstd[n], the same
 * for every slot, so the [b,s,n,d] key and value tensors are never formed.  x float [b,d,n] channel-major; mean, rstd [b,n]; any n >= 1, d >= 1,
 * 1 <= s <= 8 (hipErrorInvalidValue otherwise, the argument named in eap_last_error(), before any device call).  16-byte words are moved where
 * n % 4 == 0 and the per-point tensors of the entry are 16-byte aligned, scalars otherwise.  No atomics; sums in a fixed order.
 *
 * (L149, nn.LayerNorm's statistics) mean[b,n], rstd[b,n] = 1 / sqrt(var + ln_eps) over the d channels of a point, two passes */
int eap_slot_attn_stats_f32(int b, int d, int n, float ln_eps, const float *x, float *mean, float *rstd, eap_stream_t stream);
/* (L167-169) attn[b,s,n] = softmax over s of (z[n] . u[b,s,:] + c0[b,s]), + eps;  u [b,s,d], c0 [b,s] */
int eap_slot_attn_scores_fwd_f32(int b, int s, int d, int n, float eps, const float *x, const float *mean, const float *rstd, const float *u,
                                 const float *c0, float *attn, eap_stream_t stream);
/* (L172-175) psum[b,part,s,d+1], part < eap_slot_attn_pool_parts(n): partial sums over 1024 points each of w[b,s,n] z[n,:] (columns 0 .. d-1) and of
 * w[b,s,n] (column d), for the caller to add over the parts in float64.  w: attn forward; the gradient of the scores backward, whose sums are
 * dL/du and dL/dc0 */
int eap_slot_attn_pool_parts(int n);
int eap_slot_attn_pool_f32(int b, int s, int d, int n, const float *x, const float *mean, const float *rstd, const float *w, float *psum,
                           eap_stream_t stream);
/* (L167-175, backward) gattn = gattn_in[b,s,n] (may be null) + z[n] . gmsum[b,s,:] + gwsum[b,s];  p = attn - eps;
 * gdots[b,s,n] = p * (gattn - sum over s of p * gattn) */
int eap_slot_attn_scores_bwd_f32(int b, int s, int d, int n, float eps, const float *x, const float *mean, const float *rstd, const float *attn,
                                 const float *gmsum, const float *gwsum, const float *gattn, float *gdots, eap_stream_t stream);
/* (L149, backward) gz[n,:] = sum over the j <= 16 rows of rows[b,j,n] * vecs[b,j,:] (never written);
 * gx[b,c,n] = rstd[n] * (gz[n,c] - mean_c gz[n,:] - z[n,c] * mean_c (gz[n,:] z[n,:])) */
int eap_slot_attn_input_grad_f32(int b, int j, int d, int n, const float *x, const float *mean, const float *rstd, const float *rows,
                                 const float *vecs, float *gx, eap_stream_t stream);

/* ---- PointnetSO3Conv / PointnetSO3PoseConv: the 1x1 embed fused with the max over the points (csrc/pointnet_max.hip) -------- */
/* (vgtk/vgtk/so3conv/modules.py:L393-413) With W = embed.weight [o, c+3], W_f = W[:, :c], W_x = W[:, c:], the two small tables the caller makes
 * of it, wt [c,o] = W_f transposed (a half-wave reads 32 consecutive output channels) and v[o,na,3] = A_a W_x[o,:], and xc = xyz - centre[b]:  y[b,o,n,a] = sum_c W_f[o,c] feats[b,c,n,a] + v[o,a,:] . xc[b,:,n] + bias[o]   (never written),
 *   out[b,o,a] = max of y over the points with member[b,n] != 0,   arg[b,o,a] = the lowest such point attaining it (int32).
 * feats float [b,c,n,na], xyz [b,3,n], centre [b,3], member [b,n] (0 / 1; null: every point), bias [o] (null: none); na % 4 == 0, <= 64; o <= 2048.
 * A point that is no member never wins; a cloud without a member gives -inf and arg -1.  NaN as eap_masked_max_fwd_f32: a member's y that is NaN
 * makes out NaN and arg the lowest such point; -0.0 and +0.0 are equal.  Products on the fp32 MFMA, fp32 accumulation in ascending c; the points
 * are cut into eap_pointnet_max_parts(n) groups whose partial results pval, parg [b, parts, o, na] (workspace, written and read by the entry) are
 * folded in ascending order: no atomics, bit-identical run to run.  Every operand is moved by 4-byte words: any element-aligned address is taken.
 * Sizes first (c, o, n <= 0, na: hipErrorInvalidValue with the operand named), then null pointers, before anything is queued; b <= 0
 * returns 0 without touching a pointer. */
int eap_pointnet_max_parts(int n);
int eap_pointnet_max_fwd_f32(int b, int c, int o, int n, int na, const float *feats, const float *xyz, const float *centre, const float *member,
                             const float *wt, const float *v, const float *bias, float *pval, int32_t *parg, float *out, int32_t *arg,
                             eap_stream_t stream);
/* (modules.py:L393-413, backward to the features and coordinates) from g [b,o,na] and arg: per (cloud, anchor) the channels are grouped by their
 * point and each group is summed in ascending o:  dfeats[b,cc,n,a] = sum_{o: arg[b,o,a] = n} W[o,cc] g[b,o,a] for cc < c, and the same sum over
 * column c + i of W into dcoords[b,i,n,a] (the gradient of A_a^T xc, i < 3).  Only the named points are written: the caller zero-fills dfeats
 * [b,c,n,na] and dcoords [b,3,n,na]; one of the two may be null (not wanted).  arg outside [0, n) is skipped.  ldw >= c + 3. */
int eap_pointnet_max_bwd_data_f32(int b, int c, int o, int n, int na, const float *g, const int32_t *arg, const float *w, int ldw, float *dfeats,
                                  float *dcoords, eap_stream_t stream);
/* (modules.py:L393-413, backward to embed.weight and embed.bias) dwp[b,o,:] float [b, o, c+4] = sum over the anchors, ascending, of
 * g[b,o,a] * [feats[b,:,p,a] ; A_a^T xc[b,:,p] ; 1] at p = arg[b,o,a]: columns 0 .. c+2 the weight gradient, column c+3 the bias gradient, one
 * partial per cloud for the caller to add in float64.  anchors float [na,3,3]. */
int eap_pointnet_max_bwd_weight_f32(int b, int c, int o, int n, int na, const float *g, const int32_t *arg, const float *feats, const float *xyz,
                                    const float *centre, const float *anchors, float *dwp, eap_stream_t stream);

/* ---- the SO(3) conv layers in float64 (csrc/so3_f64.hip, csrc/so3_intra.hip) ------------------------------------------------ */
/* The reference's Python path is dtype-generic: InterSO3PoseConv(...).double() runs so3conv/functional.py:L1025-1261 in float64.  These
 * entries are that regime, chosen by the dtype of the tensors (vgtk.so3conv.functional, _InterConvF64 / _IntraConvF64 / _ContractF64).
 * float64 scalars (sigma) travel as their bit patterns (`*_bits`).  Every entry checks its sizes against the launch limits BEFORE it
 * touches a pointer (at most 64 anchors, 32 kernel points, 65535 clouds, p * nn < 2^31: hipErrorInvalidValue, the reason in
 * eap_last_error()); b <= 0 returns 0 without a launch.
 *
 * so3_prep_f64: so3conv/functional.py:L1061-1078 and the nearest-anchor half of L1199-1204, twin of eap_so3_prep_f32.
 * q_xyz [b,3,p], s_xyz [b,3,n], idx int32 [b,p,nn], poses [b,.,4,4] or both NULL, anchors [na,3,3]
 *  -> g double [b,p,nn,3] = R_rel (float(x_n) - x_p): the neighbour's coordinates pass through float32 as the reference's group_nd
 *     returns them (gathering_cuda.cpp:L38-39), the subtraction and everything after it in float64; the shadow point sits at 1e4;
 *     r int32 [b,p,nn] = argmax_g tr(R_rel A_g), first maximum (identity_anchor without poses); nonident int32 [b] (optional). */
int eap_so3_prep_f64(int b, int p, int n, int nn, int na, const double *q_xyz, const double *s_xyz, const int32_t *idx,
                     const double *q_pose, const double *s_pose, const double *anchors, int identity_anchor, double *g, int32_t *r,
                     int32_t *nonident, eap_stream_t stream);
/* so3_inter_weights_f64: inter_so3conv_grouping_anchor, so3conv/functional.py:L2508-2549, twin of eap_so3_inter_weights_f32.
 * g [b,p,nn,3], rk [na,ks,3] -> w [b,p,na,ks,nn] = relu(1 - |g - rk|^2 / sigma) in the operation order of the torch expression. */
int eap_so3_inter_weights_f64(int b, int p, int nn, int na, int ks, int64_t sigma_bits, const double *g, const double *rk, double *w,
                              eap_stream_t stream);
/* so3_inter_group_fwd_f64: so3conv/functional.py:L1221-1261, twin of eap_so3_inter_group_fwd_f32.
 * feats [b,c,n,na], mult uint8 [na,na] or NULL -> out [b,c,ks,p,na] = sum_n feats[b,c,idx_n,mult[r_n][a]] w(p,a,k,n); the weights are
 * evaluated in registers; an index outside [0, n) (the shadow row) contributes nothing. */
int eap_so3_inter_group_fwd_f64(int b, int c, int p, int n, int nn, int na, int ks, int64_t sigma_bits, const double *feats,
                                const int32_t *idx, const double *g, const int32_t *r, const double *rk, const uint8_t *mult, double *out,
                                eap_stream_t stream);
/* inv_lists_entries: the second half of the inverse neighbour lists of eap_inv_lists_rows, index only: for every referenced row slot
 * the entry numbers p * nn + n that name it, ascending, at ent[b, off .. off + cnt) -- ent int32 [b, p*nn].  Any p * nn; n <= 16384. */
int eap_inv_lists_entries(int b, int p, int n, int nn, const int32_t *idx, const int32_t *rows, const int32_t *off, int32_t *ent,
                          eap_stream_t stream);
/* inv_lists_entries_ws: what eap_inv_lists_entries writes, bit for bit, by a stable counting sort in chunks of 8192 entries
 * (csrc/native_ordered.hip): the index is read twice whatever the number of rows, where eap_inv_lists_entries reads a cloud's entries
 * twice per referenced row -- the builder for many short lists (the ordered backwards of the point gather and of the inter zpconv).
 * workspace: eap_inv_lists_entries_workspace BYTES (4 * b * ceil(p*nn / 8192) * n, 256-byte rounded), 4-byte aligned.  n <= 16384,
 * b <= 65535. */
int64_t eap_inv_lists_entries_workspace(int b, int p, int n, int nn);
int eap_inv_lists_entries_ws(int b, int p, int n, int nn, const int32_t *idx, const int32_t *rows, const int32_t *off, int32_t *ent,
                             void *workspace, eap_stream_t stream);
/* so3_inter_group_bwd_f64: the autograd of so3conv/functional.py:L1221-1261 w.r.t. feats, twin of eap_so3_inter_group_bwd_f32.
 * gout [b,c,ks,p,na]; rows, off, cnt int32 [b,n] (eap_inv_lists_rows), ent (eap_inv_lists_entries); multinv uint8 [na,na] = the
 * row-wise inverse of mult, or NULL -> gfeats [b,c,n,na] (fully written).  One workgroup per referenced row and 16 channels sums the
 * row's entries in entry order, each entry over k in index order: no floating-point atomics, bit-identical run to run. */
int eap_so3_inter_group_bwd_f64(int b, int c, int p, int n, int nn, int na, int ks, int64_t sigma_bits, const double *gout,
                                const int32_t *rows, const int32_t *off, const int32_t *cnt, const int32_t *ent, const double *g,
                                const int32_t *r, const double *rk, const uint8_t *multinv, double *gfeats, eap_stream_t stream);
/* so3_intra_group_{fwd,bwd}_f64: intra_so3conv_grouping, so3conv/functional.py:L2553-2602, and its transpose -- twins of
 * eap_so3_intra_group_fwd_f32 / eap_so3_intra_group_bwd_f32 (the same kernels at 8 bytes per element). */
int eap_so3_intra_group_fwd_f64(int b, int c, int p, int na, int t, const double *feats, const int32_t *intra_idx, double *out,
                                eap_stream_t stream);
int eap_so3_intra_group_bwd_f64(int b, int c, int p, int na, int t, const double *gout, const int32_t *intra_idx, double *gfeats,
                                eap_stream_t stream);
/* BasicSO3Conv.forward (so3conv/modules.py:L48-55) and its autograd in float64 on v_mfma_f64_16x16x4_f64: conventions and operand
 * contract of eap_gemm_f32 (leading dimensions, batch strides, any 8-byte aligned base; rows, columns and k past an operand are
 * selected as zero, nothing outside [M, N] of C is written).  eap_gemm_f64_reduce: C[M,N] = (C if accumulate else 0) + P_0 + P_1 + ...
 * with P_z = op(A_z) op(B_z) accumulated from zero and added in item order -- a batch cut into slabs (accumulate = 1 from the second
 * on) gives the bits of one call; no workspace. */
int eap_gemm_f64(int transA, int transB, int M, int N, int K, const double *A, int64_t lda, int64_t strideA, const double *B,
                 int64_t ldb, int64_t strideB, double *C, int64_t ldc, int64_t strideC, int batch, eap_stream_t stream);
int eap_gemm_f64_reduce(int transA, int transB, int M, int N, int K, const double *A, int64_t lda, int64_t strideA, const double *B,
                        int64_t ldb, int64_t strideB, double *C, int64_t ldc, int batch, int accumulate, eap_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EAP_HIP_H */
