"""Shared by tests/test_orbit_chamfer_host.py and tests/test_gpu_orbit_chamfer.py: the shapes, the seeded inputs and the two comparators of
the orbit chamfer node (extensions.chamfer_dist.OrbitChamferFunction, csrc/orbit_chamfer.hip).  The package does not import this file.

    composition        what orbit_reconstruction_distances computed before it had a node of its own: two calls of a pairwise chamfer on
                       [B*S*A]-batches that repeat the input cloud, the second with the points outside the slot moved to (1e4, 1e4, 1e4)
                       and its minima clamped to 99999.  `pair(a [b,n,3], c [b,m,3]) -> (d_ac [b,n], d_ca [b,m])` is the pairwise chamfer:
                       ChamferFunction.apply on the device, torch_pair below on the host.
    stage0_expression  ...pn_38_multi_stage.py:L432-440, the global alignment as the reference writes it.
"""
import functools

import torch

MASKED_DISTANCE = 99999.0

# tag -> (B, S, A, M, N), the smallest that reach every edge of the kernels (256 lanes per block, 1024-entry tiles):
#   empty_slot  S = 3 with the last slot left empty: cloud = g // S, the (99999, -1) pair and the zero gradient
#   edges       M crosses a 256-lane block by 4, N crosses a 1024-entry tile by 6 (and A*M = 520 a third block)
#   stage0      one group per cloud and no mask: the global alignment
SHAPES = {'empty_slot': (2, 3, 3, 5, 33), 'edges': (1, 2, 2, 260, 1030), 'stage0': (2, 1, 4, 16, 40)}
MASKED = ('empty_slot', 'edges')
REPRODUCIBLE = (1, 2, 2, 5, 1030)            # hundreds of input points name each of the five reconstruction points
MEMORY = (2, 2, 60, 64, 4096)
TIES = (1, 2, 2, 520, 2060)                  # the second half of either cloud repeats the first: every duplicate sits in a later block / tile


def seeded(shape, dtype=torch.float64, last_slot_empty=False, seed=9):
    """-> (transformed_pts [B,S,A,M,3], ori_pts [B,3,N], hard_one_hot_labels [B,N,S]) on the host: randn * 0.3, labels from randint"""
    b, s, a, m, n = shape
    gen = torch.Generator().manual_seed(seed)
    recon = torch.randn(b, s, a, m, 3, dtype=torch.float64, generator=gen) * 0.3
    ori = torch.randn(b, 3, n, dtype=torch.float64, generator=gen) * 0.3
    slot = torch.randint(0, s - 1 if last_slot_empty else s, (b, n), generator=gen)
    labels = torch.nn.functional.one_hot(slot, s).double()
    return recon.to(dtype), ori.to(dtype), labels.to(dtype)


@functools.lru_cache(maxsize=None)
def inputs(tag, dtype=torch.float64):
    """the seeded inputs of SHAPES[tag] (shared: leave them unchanged)"""
    return seeded(SHAPES[tag], dtype, last_slot_empty=(tag == 'empty_slot'))


def tied(dtype):
    """seeded(TIES) with the second half of the input cloud (labels included) and of every reconstruction a copy of the first"""
    recon, ori, labels = seeded(TIES, dtype)
    m, n = TIES[3], TIES[4]
    recon[:, :, :, m // 2:] = recon[:, :, :, :m // 2]
    ori[:, :, n // 2:] = ori[:, :, :n // 2]
    labels[:, n // 2:] = labels[:, :n // 2]
    return recon, ori, labels


def torch_pair(a, c):
    """the pairwise chamfer in plain torch (any device): squared distance of every point to the nearest of the other cloud"""
    d = (a[:, :, None, :] - c[:, None, :, :]).square().sum(-1)
    return d.min(2)[0], d.min(1)[0]


def composition(pair, transformed_pts, ori_pts, hard_one_hot_labels):
    """-> the four returns of orbit_reconstruction_distances, see the module docstring"""
    b, s, a, m, _ = transformed_pts.shape
    n = ori_pts.shape[2]
    recon = transformed_pts.reshape(b * s * a, m, 3)
    ori = ori_pts.transpose(1, 2)
    ori_all = ori[:, None, None].expand(b, s, a, n, 3).reshape(b * s * a, n, 3)
    r2o_all, o2r_all = pair(recon, ori_all)
    in_slot = hard_one_hot_labels.transpose(1, 2) >= 0.5
    far = torch.full_like(ori, 1e4)
    ori_masked = torch.where(in_slot[..., None], ori[:, None].expand(b, s, n, 3), far[:, None].expand(b, s, n, 3))
    ori_masked = ori_masked[:, :, None].expand(b, s, a, n, 3).reshape(b * s * a, n, 3)
    r2o_masked, _ = pair(recon, ori_masked)
    r2o_masked = r2o_masked.clamp(max=MASKED_DISTANCE)
    o2r_all = o2r_all.view(b, s, a, n)
    o2r_masked = torch.where(in_slot[:, :, None].expand(b, s, a, n), o2r_all, o2r_all.new_full((), MASKED_DISTANCE))
    return o2r_all, r2o_all.view(b, s, a, m).mean(-1), r2o_masked.view(b, s, a, m).mean(-1), o2r_masked


def composition_maps(forward, transformed_pts, ori_pts, hard_one_hot_labels):
    """the same two calls through `forward(a, c) -> (d_ac, d_ca, i_ac, i_ca)` (chamfer.forward), for the per-point values and indices
    -> (r2o_all, r2o_all_idx, r2o_masked (clamped), r2o_masked_idx, o2r_all, o2r_idx), each [B*S, A, M or N]"""
    b, s, a, m, _ = transformed_pts.shape
    n = ori_pts.shape[2]
    recon = transformed_pts.reshape(b * s * a, m, 3).contiguous()
    ori = ori_pts.transpose(1, 2)
    ori_all = ori[:, None, None].expand(b, s, a, n, 3).reshape(b * s * a, n, 3).contiguous()
    r2o_all, o2r_all, i_r2o, i_o2r = forward(recon, ori_all)
    in_slot = hard_one_hot_labels.transpose(1, 2) >= 0.5
    far = torch.full_like(ori, 1e4)
    ori_masked = torch.where(in_slot[..., None], ori[:, None].expand(b, s, n, 3), far[:, None].expand(b, s, n, 3))
    ori_masked = ori_masked[:, :, None].expand(b, s, a, n, 3).reshape(b * s * a, n, 3).contiguous()
    r2o_masked, _, i_masked, _ = forward(recon, ori_masked)
    g = b * s
    return (r2o_all.view(g, a, m), i_r2o.view(g, a, m), r2o_masked.clamp(max=MASKED_DISTANCE).view(g, a, m), i_masked.view(g, a, m),
            o2r_all.view(g, a, n), i_o2r.view(g, a, n))


def stage0_expression(pair, transformed_glb_recon_pts, ori_pts):
    """...pn_38_multi_stage.py:L432-440 (safe_transpose = transpose().contiguous()) -> (chamfer_recon_to_ori [B,A], chamfer_ori_to_recon [B,A])"""
    bz, cur_kanchor = transformed_glb_recon_pts.shape[:2]
    npoints = ori_pts.shape[2]
    expanded_ori_pts = ori_pts.transpose(-1, -2).contiguous().unsqueeze(1).contiguous().repeat(1, cur_kanchor, 1, 1)
    chamfer_recon_to_ori, chamfer_ori_to_recon = pair(
        transformed_glb_recon_pts.contiguous().view(bz * cur_kanchor, transformed_glb_recon_pts.size(-2), 3),
        expanded_ori_pts.contiguous().view(bz * cur_kanchor, npoints, 3))
    chamfer_recon_to_ori = chamfer_recon_to_ori.contiguous().view(bz, cur_kanchor, -1).mean(dim=-1)
    chamfer_ori_to_recon = chamfer_ori_to_recon.contiguous().view(bz, cur_kanchor, -1).mean(dim=-1)
    return chamfer_recon_to_ori, chamfer_ori_to_recon
