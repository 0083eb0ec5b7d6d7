// csrc/group_lists.h -- the walk over entry lists that the one-tile and the two-tile grouping kernel share
// (csrc/so3_inter_lists.hip, csrc/so3_inter_lists2.hip): which rows and entries a workgroup owns, the per-entry terms of a
// chunk, and the launchers' operand checks.  Constants, geometry, DMA mapping, k-step and row end are each kernel's own.
#pragma once
#include <stdio.h>

#include "common.h"
#include "kernel_weight.h"

namespace group_lists {

#ifdef __HIPCC__
// ---- block -> (run of rows, anchor group, slice) ---------------------------------------------------------------------
// A grid is (nrun * AG, channel slices, clouds); slice = channel slice + gridDim.y * cloud.  Workgroups go to the 8 XCDs
// round-robin by linear id: an XCD gets whole slices when their number allows it (its CUs then share one window of the
// features in their own L2), else a contiguous range of rows (whole output lines in one L2).
__device__ __forceinline__ void block_map(int nrun, int AG, int &run, int &ag, int &sl) {
    const int ny = gridDim.y, nsl = ny * gridDim.z, per_slice = nrun * AG;
    int qd;
    sl = blockIdx.y + ny * blockIdx.z;
    if ((nsl & 7) == 0) {
        const unsigned lin = blockIdx.x + (unsigned)per_slice * (blockIdx.y + (unsigned)ny * blockIdx.z);
        const unsigned j = lin >> 3;
        sl = (int)((lin & 7u) + 8u * (j / (unsigned)per_slice));
        qd = (int)(j % (unsigned)per_slice);
    } else {
        qd = xcd_point(blockIdx.x, per_slice);
    }
    run = qd / AG;
    ag = qd - run * AG;
}

// ---- the entries of a workgroup ---------------------------------------------------------------------------------------
// LISTS = true : rows / off / cnt describe variable-length entry lists (backward), one list per workgroup;
// LISTS = false: row r of cloud bi owns entries [(bi*R + r)*nn, +nn) (forward: its neighbours), and a workgroup takes
// rows_blk consecutive rows from r_begin: they are contiguous in idx / gx, and with nn a multiple of the chunk the flat
// chunk sequence never straddles two rows (rows_per_block below).
struct Entries {
    int n_ent;          // entries of the workgroup
    size_t e0;          // its first entry
    int nchunk_row;     // chunks of NBK entries per row
    int nchunk;         // ... and of the workgroup
};
template <bool LISTS, int NBK>
__device__ __forceinline__ Entries entries(int bi, int R, int r_begin, int rows_blk, int nn, int ent_stride,
                                           const int32_t *__restrict__ rows, const int32_t *__restrict__ off, const int32_t *__restrict__ cnt) {
    Entries en;
    if (LISTS) {
        const int q = rows[(size_t)bi * R + r_begin];
        en.n_ent = q >= 0 ? cnt[(size_t)bi * R + r_begin] : 0;
        en.e0 = (size_t)bi * ent_stride + (q >= 0 ? off[(size_t)bi * R + r_begin] : 0);
        en.nchunk_row = (en.n_ent + NBK - 1) / NBK;
    } else {
        en.n_ent = rows_blk * nn;
        en.e0 = ((size_t)bi * R + r_begin) * nn;
        en.nchunk_row = (nn + NBK - 1) / NBK;
    }
    en.nchunk = LISTS ? en.nchunk_row : rows_blk * en.nchunk_row;
    return en;
}

// ---- per-entry terms of a chunk ---------------------------------------------------------------------------------------
// Lane e (mod NBK) evaluates the per-entry term of entry e of chunk ch, whose offset vectors and feature rows sit in slot
// gslot of the rings s_g / s_p; the k-steps fetch theirs by ds_bpermute.  Entries past the end of the list get the dead
// value (weight 0), and with SHADOW so do the entries whose feature row is not one of the PF rows (the forward's shadow
// neighbours, when their offset vector does not say so itself).
template <int NBK, bool SHADOW>
__device__ __forceinline__ int chunk_bases(const float4 *s_g, const int *s_p, int gslot, int ch, int lane, int n_ent, int PF, float inv_sigma) {
    const int e = lane & (NBK - 1);
    const float4 g = s_g[gslot * NBK + e];
    // (kernel_weight::entry_base written out: through the call hipcc squares and sums the three terms in another order)
    const float b = 1.0f - inv_sigma * (g.x * g.x + g.y * g.y + g.z * g.z);
    bool dead = ch * NBK + e >= n_ent;
    if (SHADOW) dead = dead || (unsigned)s_p[gslot * NBK + e] >= (unsigned)PF;
    return __float_as_int(dead ? kernel_weight::DEAD : b);
}
#endif

// ---- host side --------------------------------------------------------------------------------------------------------
// forward: a workgroup streams through a run of consecutive rows (the next row's entries and first chunk are in flight
// during the current row's last chunk) when no chunk straddles two rows
inline int rows_per_block(bool lists, int nn, int nbk) { return lists ? 1 : ((nn % nbk) == 0 ? 8 : 1); }

// what the kernels' 32-bit offsets ask of the operands; cb = channels per workgroup, kernel = the name in the error text
inline int check_operands(const char *kernel, int cb, int PF, int na, int fpitch, int ks, int R) {
    char rows[96];
    snprintf(rows, sizeof(rows), "%d feature rows of a cloud exceed the 32-bit request offsets", cb);
    const char *what = nullptr;
    if (fpitch < na || (fpitch & 3) != 0) what = "the feature row pitch must be a multiple of 4, at least the anchor count";
    else if ((long long)cb * PF * fpitch * 4 >= (1ll << 32) || PF >= (1 << 24) || fpitch * 4 >= (1 << 24)) what = rows;
    else if (((long long)ks * R * na * 4 + (long long)cb * R * na + 64) * 4 >= (1ll << 31) || (long long)cb * ks * 4 >= (1ll << 31))
        what = "output rows too far apart for 32-bit store offsets";
    if (!what) return 0;
    char buf[192];
    snprintf(buf, sizeof(buf), "%s: %s", kernel, what);
    return eap::bad_arg(buf);
}

}  // namespace group_lists
