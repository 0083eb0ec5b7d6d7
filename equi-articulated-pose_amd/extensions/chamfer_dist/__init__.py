"""extensions.chamfer_dist -- ChamferFunction / ChamferDistance with the reference's interface
(extensions/chamfer_dist/__init__.py:L13-45), computed by the HIP kernels in csrc/chamfer.hip.  float32 or float64: every result
comes back in the width of the clouds.  The backward is bit-identical run to run in float64, and in float32 under
torch.use_deterministic_algorithms(True) (chamfer.backward).

Above them the model's two reconstruction-distance blocks over the orbit, each one node on csrc/orbit_chamfer.hip (OrbitChamferFunction):
orbit_reconstruction_distances (per slot, ...pn_38_multi_stage.py:L1341-1361) and global_orbit_distances (L429-440).  Their backward is
bit-identical run to run at both widths, whatever the global setting."""
import torch

import chamfer


class ChamferFunction(torch.autograd.Function):
    """(a [B,N,3], b [B,M,3]) -> (squared distance of every a-point to its nearest b-point [B,N], and the converse [B,M]);
    the nearest-neighbour indices are kept for the backward (csrc/chamfer.hip)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        a, b = xyz1.contiguous(), xyz2.contiguous()
        d_ab, d_ba, nearest_ab, nearest_ba = chamfer.forward(a, b)
        ctx.save_for_backward(a, b, nearest_ab, nearest_ba)
        return d_ab, d_ba

    @staticmethod
    def backward(ctx, g_ab, g_ba):
        a, b, nearest_ab, nearest_ba = ctx.saved_tensors
        return tuple(chamfer.backward(a, b, nearest_ab, nearest_ba, g_ab, g_ba))


class OrbitChamferFunction(torch.autograd.Function):
    """(recon [G,A,M,3], ori [B,3,N] planar with G = B*S, member uint8 [G,N] or None) -> the squared nearest-neighbour distances of every
    candidate cloud (g, a) against the cloud of its group, g // S (chamfer.orbit_forward, csrc/orbit_chamfer.hip):
        with member     (r2o_all [G,A,M], r2o_in [G,A,M], o2r_all [G,A,N], o2r_in [G,A,N])      `in`: over the flagged points / 99999 outside
        member = None   (r2o_all [G,A,M], o2r_all [G,A,N])
    The three index maps are kept for the backward, an ordered gather into recon's gradient; ori gets none."""

    @staticmethod
    def forward(ctx, recon, ori, member):
        recon, ori = recon.contiguous(), ori.contiguous()
        r2o_all, r2o_all_idx, r2o_in, r2o_in_idx, o2r_all, o2r_idx, o2r_in = chamfer.orbit_forward(recon, ori, member)
        ctx.save_for_backward(recon, ori, member, r2o_all_idx, r2o_in_idx, o2r_idx)
        return (r2o_all, o2r_all) if member is None else (r2o_all, r2o_in, o2r_all, o2r_in)

    @staticmethod
    def backward(ctx, *grads):
        recon, ori, member, r2o_all_idx, r2o_in_idx, o2r_idx = ctx.saved_tensors
        g_r2o_all, g_r2o_in, g_o2r_all, g_o2r_in = (grads[0], None, grads[1], None) if member is None else grads
        return chamfer.orbit_backward(recon, ori, member, r2o_all_idx, r2o_in_idx, o2r_idx, g_r2o_all, g_r2o_in, g_o2r_all, g_o2r_in), None, None


class ChamferDistance(torch.nn.Module):
    """mean(d_ab) + mean(d_ba) (or the two raw distance maps).  ignore_zeros: for a single pair of clouds, points whose
    coordinates sum to zero (padding) are dropped first, as the reference does."""

    def __init__(self, ignore_zeros=False):
        super().__init__()
        self.ignore_zeros = ignore_zeros

    @staticmethod
    def _without_padding(cloud):
        keep = cloud.sum(dim=2).ne(0)                  # [1, n]
        return cloud[keep].unsqueeze(0)

    def forward(self, xyz1, xyz2, return_raw=False):
        if self.ignore_zeros and xyz1.size(0) == 1:
            xyz1, xyz2 = self._without_padding(xyz1), self._without_padding(xyz2)
        d_ab, d_ba = ChamferFunction.apply(xyz1, xyz2)
        return (d_ab, d_ba) if return_raw else d_ab.mean() + d_ba.mean()


MASKED_DISTANCE = 99999.0     # the constant the reference writes into masked entries of the distance tensor


def orbit_reconstruction_distances(transformed_pts, ori_pts, hard_one_hot_labels):
    """The slot/orbit reconstruction distances of the reference's orbit selection
    (SPConvNets/models/unsup_seg_so3_pose_conv_pn_38_multi_stage.py:L1341-1361) WITHOUT its
    `dist_recon_ori [B, S, A, M, N]` tensor (4 GB at B=8, S=2, A=60, M=256, N=4096): a 60-way batched
    chamfer on the chamfer kernels (csrc/chamfer.hip), SURVEY.md 8(f) row 2.

    transformed_pts [B,S,A,M,3]  per-slot, per-anchor reconstructions
    ori_pts         [B,3,N]      the input cloud (the width of transformed_pts: float32 or float64)
    hard_one_hot_labels [B,N,S]  0/1 point-to-slot assignment
    ->  (minn_dist_ori_to_recon_all_pts [B,S,A,N],  min over M of the unmasked distances
         minn_dist_recon_to_ori_all_pts [B,S,A],    mean over M of the min over N, unmasked
         minn_dist_recon_to_ori         [B,S,A],    the same with points outside the slot masked
         minn_dist_ori_to_recon         [B,S,A,N])  min over M with masked points set to 99999
    Gradients flow to transformed_pts exactly as through the reference's min / mean.

    One node, OrbitChamferFunction (csrc/orbit_chamfer.hip): the input cloud is read in place, membership is a flag per point, one scan
    keeps the unmasked and the masked minimum, and the backward is a gather in a fixed order (the same bits every run).  Only when
    ori_pts itself needs a gradient (the node gives it none) does the composition of two ChamferFunction calls below run instead; the
    forward values of the two are the same bits."""
    if ori_pts.requires_grad and torch.is_grad_enabled():
        return _orbit_reconstruction_distances_composed(transformed_pts, ori_pts, hard_one_hot_labels)
    if transformed_pts.dim() != 5 or transformed_pts.shape[-1] != 3 or ori_pts.dim() != 3:
        raise RuntimeError(f'orbit_reconstruction_distances: transformed_pts [B,S,A,M,3] and ori_pts [B,3,N], not {tuple(transformed_pts.shape)} '
                           f'and {tuple(ori_pts.shape)}')
    b, s, a, m, _ = transformed_pts.shape
    n = ori_pts.shape[2]
    if tuple(ori_pts.shape) != (b, 3, n) or tuple(hard_one_hot_labels.shape) != (b, n, s):
        raise RuntimeError(f'orbit_reconstruction_distances: ori_pts [B,3,N] and hard_one_hot_labels [B,N,S] for B = {b}, S = {s}, not '
                           f'{tuple(ori_pts.shape)} and {tuple(hard_one_hot_labels.shape)}')
    member = (hard_one_hot_labels.transpose(1, 2) >= 0.5).to(torch.uint8).contiguous().view(b * s, n)      # [G,N]
    r2o_all, r2o_in, o2r_all, o2r_in = OrbitChamferFunction.apply(transformed_pts.reshape(b * s, a, m, 3), ori_pts, member)
    return (o2r_all.view(b, s, a, n), r2o_all.view(b, s, a, m).mean(-1), r2o_in.view(b, s, a, m).mean(-1), o2r_in.view(b, s, a, n))


def global_orbit_distances(transformed_glb_recon_pts, ori_pts):
    """The global alignment's distances (...pn_38_multi_stage.py:L429-440): every one of the A posed reconstructions of a cloud against
    that cloud, with no mask -- the reference's `repeat(1, cur_kanchor, 1, 1)` of the cloud and its [B*A]-batch chamfer, without the copies.

    transformed_glb_recon_pts [B,A,M,3], ori_pts [B,3,N]  ->  (chamfer_recon_to_ori [B,A], chamfer_ori_to_recon [B,A]): the means of
    L438-440, the same bits as that expression through ChamferFunction.  (ori_pts needing a gradient: that expression itself runs.)"""
    if transformed_glb_recon_pts.dim() != 4 or transformed_glb_recon_pts.shape[-1] != 3 or ori_pts.dim() != 3 or \
            tuple(ori_pts.shape[:2]) != (transformed_glb_recon_pts.shape[0], 3):
        raise RuntimeError(f'global_orbit_distances: transformed_glb_recon_pts [B,A,M,3] and ori_pts [B,3,N], not '
                           f'{tuple(transformed_glb_recon_pts.shape)} and {tuple(ori_pts.shape)}')
    b, a, m, _ = transformed_glb_recon_pts.shape
    n = ori_pts.shape[2]
    if ori_pts.requires_grad and torch.is_grad_enabled():
        expanded = ori_pts.transpose(1, 2).unsqueeze(1).contiguous().repeat(1, a, 1, 1)
        r2o, o2r = ChamferFunction.apply(transformed_glb_recon_pts.contiguous().view(b * a, m, 3), expanded.view(b * a, n, 3))
    else:
        r2o, o2r = OrbitChamferFunction.apply(transformed_glb_recon_pts, ori_pts, None)
    return r2o.contiguous().view(b, a, -1).mean(dim=-1), o2r.contiguous().view(b, a, -1).mean(dim=-1)


def _orbit_reconstruction_distances_composed(transformed_pts, ori_pts, hard_one_hot_labels):
    """orbit_reconstruction_distances as two calls of the pairwise ChamferFunction on expanded copies of the cloud, the second with the
    points outside the slot moved out of reach: the path that carries a gradient to ori_pts."""
    b, s, a, m, _ = transformed_pts.shape
    n = ori_pts.shape[2]
    recon = transformed_pts.reshape(b * s * a, m, 3)
    ori = ori_pts.transpose(1, 2)                                                   # [B,N,3]
    ori_all = ori[:, None, None].expand(b, s, a, n, 3).reshape(b * s * a, n, 3)
    r2o_all, o2r_all = ChamferFunction.apply(recon, ori_all)                         # [B',M], [B',N]
    in_slot = hard_one_hot_labels.transpose(1, 2) >= 0.5                             # [B,S,N]
    # masked: points outside the slot are moved out of reach; the reference's 99999 entries are what
    # an empty slot's minimum sees, hence the clamp
    far = torch.full_like(ori, 1e4)                                                  # (ori's width, like the 99999 below)
    ori_masked = torch.where(in_slot[..., None], ori[:, None].expand(b, s, n, 3), far[:, None].expand(b, s, n, 3))
    ori_masked = ori_masked[:, :, None].expand(b, s, a, n, 3).reshape(b * s * a, n, 3)
    r2o_masked, _ = ChamferFunction.apply(recon, ori_masked)
    r2o_masked = r2o_masked.clamp(max=MASKED_DISTANCE)
    o2r_all = o2r_all.view(b, s, a, n)
    o2r_masked = torch.where(in_slot[:, :, None].expand(b, s, a, n), o2r_all, o2r_all.new_full((), MASKED_DISTANCE))
    return (o2r_all, r2o_all.view(b, s, a, m).mean(-1), r2o_masked.view(b, s, a, m).mean(-1), o2r_masked)
