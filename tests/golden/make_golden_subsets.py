"""tests/golden/make_golden_subsets.py -- golden vectors of InterSO3PoseConv(kanchor = 20 / 40, permute_modes = 1) with per-point
poses (so3conv/modules.py:L222-322 -> so3conv/functional.py:L1025-1261, and the articulation-state branch L1420-1520), produced by
RUNNING THE REFERENCE on CPU in the build container (tests/golden/ref_import.py).  The 20- and 40-anchor sets are subsets of the 60
icosahedral rotations (select_anchor, L2641-2649), not groups: the per-entry anchor index argmax_j tr(R_rel^T A_a A_j^T) (L1199-1204) is
no table lookup and in general no permutation.  Data only.

  inter_pose_subsets.npz   per anchor count: one rotation per point, one rotation per rigid part, one rotation per point in
                           articulation-state mode; outputs + autograd gradients + the anchor index recomputed with the oracle's
                           expression (and, as `*_trace_gap`, the smallest float64 gap between the best and the second-best trace)

Re-run:  python tests/golden/make_golden_subsets.py"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import make_golden as MG  # noqa: E402  (imports the reference through ref_import)
from make_golden import poses, save  # noqa: E402
from make_golden_extra import synth_clouds  # noqa: E402
from oracle import so3_ref  # noqa: E402

vgtk, sptk, L, zptk = MG.vgtk, MG.sptk, MG.L, MG.zptk

RADIUS, SIGMA = 0.2, 0.02


def anchor_index(ball_idx, pose, anchors):
    """-> (the oracle's rotated_anchor_index int64 [b,p,nn,na] in float64, the smallest gap between the two largest traces)"""
    rot = pose[:, :, :3, :3].double()
    grouped = so3_ref.batched_index_select_other(rot, ball_idx.long(), dim=1)
    rel = torch.matmul(rot.unsqueeze(2), grouped.transpose(3, 4).contiguous())
    A = anchors.double()
    idx = so3_ref.rotated_anchor_index(rel, A)
    traces = torch.einsum('bpnji,ajk,cik->bpnac', rel, A, A)          # <R_rel^T A_a, A_c>_F
    top = traces.topk(2, dim=-1).values
    assert torch.equal(traces.argmax(-1), idx)
    return idx, float((top[..., 0] - top[..., 1]).min())


def main():
    gen = torch.Generator().manual_seed(4242)
    B, P, C, O, NNB = 2, 40, 4, 4, 8
    base, part, _ = synth_clouds.laptop_batch(23, B, P)
    xyz = torch.from_numpy(base)
    # articulation states as tests/golden/make_golden_artmode.py builds them: state 1 = the lid points moved by a small rigid motion
    moved = xyz.clone()
    lid = torch.from_numpy(part).bool()
    Rz = torch.tensor([[0.9553, -0.2955, 0.0], [0.2955, 0.9553, 0.0], [0.0, 0.0, 1.0]])
    for b in range(B):
        moved[b][:, lid[b]] = Rz @ xyz[b][:, lid[b]] + torch.tensor([[0.02], [0.0], [0.01]])
    xyz_states = torch.stack([xyz, moved], 1).contiguous()                # [b, ns, 3, p]
    seg = torch.from_numpy(part).long()
    out = {'xyz': xyz, 'xyz_states': xyz_states, 'seg': seg}
    for na in (20, 40):
        for tag, mode, art in (('random', 'random', False), ('parts', 'parts', False), ('art_random', 'random', True)):
            key = f'k{na}_{tag}'
            torch.manual_seed(2913)
            conv = sptk.InterSO3PoseConv(C, O, 1, 1, RADIUS, SIGMA, NNB, kanchor=na, permute_modes=1, use_art_mode=art)
            pose = poses(gen, B, P, mode)
            feats = torch.randn(B, C, P, na, generator=gen).requires_grad_(True)
            with contextlib.redirect_stdout(io.StringIO()):
                if art:
                    _, inter_w, _, y = conv(zptk.SphericalPointCloudPose(xyz_states, feats, None, pose), seg=seg)
                else:
                    _, inter_w, _, y = conv(zptk.SphericalPointCloudPose(xyz, feats, None, pose))
            assert tuple(y.feats.shape) == (B, O, P, na)
            gy = torch.randn(y.feats.shape, generator=gen)
            gfe, gW = torch.autograd.grad(y.feats, [feats, conv.basic_conv.W], gy)
            if art:
                per_state = torch.stack([so3_ref.ball_query(xyz_states[:, s].contiguous(), xyz_states[:, s].contiguous(), RADIUS, NNB)[0].long()
                                         for s in range(xyz_states.shape[1])], 1)                       # [b, ns, p, nn]
                ball_idx = per_state.gather(1, seg.view(B, 1, P, 1).expand(B, 1, P, NNB)).squeeze(1)
            else:
                ball_idx = so3_ref.ball_query(xyz, xyz, RADIUS, NNB)[0].long()
            idx, gap = anchor_index(ball_idx, pose, conv.anchors)
            print(f'{key}: smallest trace gap {gap:.3e}, non-identity entries {float((idx != torch.arange(na)).any(-1).float().mean()):.2f}')
            out.update({f'{key}_W': conv.basic_conv.W, f'{key}_pose': pose, f'{key}_feats': feats, f'{key}_out': y.feats, f'{key}_gy': gy,
                        f'{key}_gfeats': gfe, f'{key}_gW': gW, f'{key}_inter_w_sample': inter_w[:, ::8, ::7, ::5],
                        f'{key}_rotated_anchor_idx': idx.to(torch.uint8), f'{key}_trace_gap': np.float64(gap)})
            out[f'k{na}_anchors'], out['kernels'] = conv.anchors, conv.kernels
    save('inter_pose_subsets.npz', **out)


if __name__ == '__main__':
    main()
