"""tests/golden/make_golden_dense_wide.py -- golden vectors for a layer whose clouds reference MORE THAN 512 support rows (the wide
tables of csrc/so3_dense.hip: 32 membership words per point, a 64-bit group key), produced by RUNNING THE REFERENCE on CPU in the build
container (through tests/golden/ref_import.py).  Data only.

  dense_wide_identity_o128.npz  InterSO3PoseConv 8 -> 128, 2 x 1024 points (synth_clouds.laptop_batch(7, 2, 1024)), nsample 32, radius 0.12,
                                sigma 0.5 radius^2, identity poses: every ball holds >= 32 points (no padded list), a cloud's lists name
                                535-543 of its rows (512 < rows <= 1024) and a list touches ~14.5 of their 34 groups of 16 -> the DEFAULT
                                decision takes the dense product in both directions (bound: 16 groups)

Reference path: so3conv/modules.py:L222-322 -> so3conv/functional.py:L1025-1261 -> so3conv/modules.py:L48-55, autograd for the gradients.

Size.  At 1024 points the layer's input alone is 3.9 MB and its output 63 MB; a committed file stays under 1 MiB.  So
  * feats and the factors of the output gradient are NOT stored: both sides draw them from torch's CPU generator with the seeds stored in
    the file (`seed_feats`, `seed_gy`; torch.randn in the order of `draw` below), and the file carries float64 checksums of them
    (`feats_check`, `gy_check`: sum, sum of squares and the first 8 values) so that a generator that drew something else fails the test
    there, not at the comparison;
  * the output gradient is rank 2 as in make_golden_dense.py, gy[b,o,p,a] = u1[b,o] v1[b,p,a] + u2[b,o] v2[b,p,a];
  * the output is stored on every 16th channel at every 31st point (`out_channels16`, points POINTS = 0, 31, 62, ...) and on all
    channels at every 256th point (`out_points256`); grad_feats at every 31st point (`grad_feats_points31`) -- every such entry still
    sums over all the lists that name the point; grad_W whole;
  * the poses are identities and are not stored.

Re-run:  python tests/golden/make_golden_dense_wide.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference through ref_import)
from make_golden import save  # noqa: E402
from make_golden_dense import rank2_grad  # noqa: E402

sptk, L, zptk, synth_clouds = MG.sptk, MG.L, MG.zptk, MG.synth_clouds
B, P, C, O, NN = 2, 1024, 8, 128, 32
RADIUS = 0.12
SIGMA = 0.5 * RADIUS * RADIUS
SEED_FEATS, SEED_GY = 71024, 71025


def draw(seed_feats, seed_gy, b, c, o, p, na=60):
    """the layer's input and the four factors of its output gradient (CPU generator; the test repeats exactly these calls)"""
    gen = torch.Generator().manual_seed(int(seed_feats))
    feats = torch.randn(b, c, p, na, generator=gen)
    gen = torch.Generator().manual_seed(int(seed_gy))
    u1, u2 = torch.randn(b, o, generator=gen), torch.randn(b, o, generator=gen)
    v1, v2 = torch.randn(b, p, na, generator=gen), torch.randn(b, p, na, generator=gen)
    return feats, u1, v1, u2, v2


def check(*ts):
    """float64 [sum, sum of squares, first 8 values] of the tensors laid end to end"""
    v = torch.cat([t.detach().double().flatten() for t in ts])
    return np.concatenate([[float(v.sum()), float((v * v).sum())], v[:8].numpy()])


def main():
    xyz = torch.from_numpy(synth_clouds.laptop_batch(7, B, P)[0])
    torch.manual_seed(2913)
    conv = sptk.InterSO3PoseConv(C, O, 1, 1, RADIUS, SIGMA, NN, kanchor=60, permute_modes=1)
    pose = torch.eye(4).repeat(B, P, 1, 1)
    feats, u1, v1, u2, v2 = draw(SEED_FEATS, SEED_GY, B, C, O, P)
    feats.requires_grad_(True)
    # what makes the case a wide dense one, from the reference's own ball query (= the oracle's C restatement): no padded list, and more
    # than 512 but at most 1024 referenced rows in every cloud
    idx = MG.vgtk.cuda.grouping.ball_query(xyz, xyz, RADIUS, NN).numpy()
    d = (xyz[:, :, :, None] - xyz[:, :, None, :]).norm(dim=1)
    assert int((d < RADIUS).sum(-1).min()) >= NN, 'a ball with fewer than nsample points: its list would be padded'
    assert all(len(np.unique(idx[b, p])) == NN for b in range(B) for p in range(P))
    rows = [len(np.unique(idx[b])) for b in range(B)]
    assert all(512 < r <= 1024 for r in rows), rows
    inter_idx, inter_w, sample_idx, y = conv(zptk.SphericalPointCloudPose(xyz, feats, None, pose))
    gy = rank2_grad(u1, v1, u2, v2)
    gfe, gW = torch.autograd.grad(y.feats, [feats, conv.basic_conv.W], gy)
    assert idx.max() < 32768
    save('dense_wide_identity_o128.npz', xyz=xyz, W=conv.basic_conv.W, anchors=conv.anchors, kernels=conv.kernels,
         radius=np.float32(RADIUS), sigma=np.float32(SIGMA), nn=np.int32(NN), permute_modes=np.int32(1),
         referenced_rows=np.asarray(rows, np.int32), ball_idx=idx.astype(np.int16),
         seed_feats=np.int64(SEED_FEATS), seed_gy=np.int64(SEED_GY), in_channels=np.int32(C),
         feats_check=check(feats), gy_check=check(u1, v1, u2, v2),
         out_channels16=y.feats[:, ::16, ::31], out_points256=y.feats[:, :, ::256],
         grad_feats_points31=gfe[:, :, ::31], grad_W=gW)
    size = os.path.getsize(os.path.join(HERE, 'dense_wide_identity_o128.npz'))
    assert size < 1024 * 1024, size


if __name__ == '__main__':
    main()
