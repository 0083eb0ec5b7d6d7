"""tests/golden/make_golden_f64.py -- golden vectors of the SO(3) conv layers in FLOAT64, produced by RUNNING THE REFERENCE classes with
.double() on the CPU (tests/golden/ref_import.py; the reference is only in the build container).  Data only.

  so3_f64.npz   shared inputs (random float64 coordinates, features and per-point rotations -- not float32 numbers widened; cloud 0 has one
                random rotation per point, cloud 1 identity poses) and per case W, output, dF, dW (inter_w of the first 4 points: below):
                  pm1     InterSO3PoseConv(3, 5, 1, 1, 0.3, 0.05, 8, kanchor=60, permute_modes=1), B = 2, P = 40
                  pm0     the same with permute_modes=0
                  nopose  InterSO3Conv(3, 5, 1, 1, 0.3, 0.05, 8)
                  k20     InterSO3PoseConv(..., kanchor=20, permute_modes=0)
                  intra   IntraSO3Conv(3, 5)

The file has to stay under 1 MB and float64 noise does not compress, so
  * the cases share their inputs (`xyz`, `pose`, `feats`, `gy`; the 20-anchor case takes every third anchor of them -- its anchor set IS
    every third of the 60 --, the intra case the same features and cotangent); the cotangent `gy` is drawn in float32 and stored so
    (the gradients are linear in it; the test widens it);
  * output and dF are stored at the points listed in `points` (every fourth one; every cloud, channel and anchor is there); dW is a sum over
    all points and is stored whole;
  * `ball_idx` int32 [2,40,8]: the neighbour lists of every inter case (the oracle's ball query on the float64 coordinates);
  * inter_w of the first 4 points is stored once per distinct geometry: `inter_w_posed` [2,4,60,24,8] is what pm1 AND pm0 returned (the
    weights do not depend on the permutation; asserted below), k20 returned its anchors ::3 (asserted), and `inter_w_nopose0` [4,60,24,8] is
    cloud 0 of the pose-free case, whose cloud 1 (identity poses) returned `inter_w_posed[1]` (asserted).

Re-run:  python tests/golden/make_golden_f64.py"""
import contextlib
import io
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import make_golden as MG  # noqa: E402  (imports the reference through ref_import)
from make_golden import save  # noqa: E402
from oracle import so3_ref  # noqa: E402

sptk, zptk = MG.sptk, MG.zptk

B, P, C, O, NNB = 2, 40, 3, 5, 8
RADIUS, SIGMA = 0.3, 0.05


def rand_rot64(gen, *shape):
    q = torch.randn(*shape, 4, generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return R.view(*shape, 3, 3)


def main():
    gen = torch.Generator().manual_seed(6464)
    xyz = torch.rand(B, 3, P, generator=gen, dtype=torch.float64) * 0.8
    pose = torch.eye(4, dtype=torch.float64).repeat(B, P, 1, 1)
    pose[0, :, :3, :3] = rand_rot64(gen, P)
    feats60 = torch.randn(B, C, P, 60, generator=gen, dtype=torch.float64)
    gy32 = torch.randn(B, O, P, 60, generator=gen, dtype=torch.float32)
    gy60 = gy32.double()
    points = torch.arange(0, P, 4)
    assert not torch.equal(xyz.float().double(), xyz) and not torch.equal(feats60.float().double(), feats60)
    ball_idx = so3_ref.ball_query(xyz, xyz, RADIUS, NNB)[0]          # the neighbour lists every inter case uses (float64 comparison)
    assert int((ball_idx[:, :, 1:] == ball_idx[:, :, :1]).sum()) > 0   # (some lists are repeat-padded)
    out = {'xyz': xyz, 'pose': pose, 'feats': feats60, 'gy': gy32, 'points': points, 'ball_idx': ball_idx}
    inter_w = {}

    def run(key, conv, cloud, feats, gy):
        conv = conv.double()
        feats = feats.clone().requires_grad_(True)
        cloud = cloud(feats)
        with contextlib.redirect_stdout(io.StringIO()):
            res = conv(cloud)
        y = res.feats if key == 'intra' else res[3].feats
        assert y.dtype == torch.float64 and tuple(y.shape) == tuple(gy.shape)
        gF, gW = torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)
        assert gF.dtype == torch.float64 and gW.dtype == torch.float64
        out.update({f'{key}_W': conv.basic_conv.W, f'{key}_out': y[:, :, points], f'{key}_gfeats': gF[:, :, points], f'{key}_gW': gW})
        if key != 'intra':
            assert res[1].dtype == torch.float64
            inter_w[key] = res[1][:, :4].detach()
            assert res[0] is None or torch.equal(res[0].int(), ball_idx)      # (InterSO3Conv hands its lists back)
            out[f'{key}_anchors'], out['kernels'] = conv.anchors, conv.kernels
        else:
            out['intra_idx'] = conv.intra_idx

    posed = lambda f: zptk.SphericalPointCloudPose(xyz, f, None, pose)
    plain = lambda f: zptk.SphericalPointCloud(xyz, f, None)
    torch.manual_seed(6464)
    run('pm1', sptk.InterSO3PoseConv(C, O, 1, 1, RADIUS, SIGMA, NNB, kanchor=60, permute_modes=1), posed, feats60, gy60)
    run('pm0', sptk.InterSO3PoseConv(C, O, 1, 1, RADIUS, SIGMA, NNB, kanchor=60, permute_modes=0), posed, feats60, gy60)
    run('nopose', sptk.InterSO3Conv(C, O, 1, 1, RADIUS, SIGMA, NNB), plain, feats60, gy60)
    run('k20', sptk.InterSO3PoseConv(C, O, 1, 1, RADIUS, SIGMA, NNB, kanchor=20, permute_modes=0), posed,
        feats60[..., ::3].contiguous(), gy60[..., ::3].contiguous())
    run('intra', sptk.IntraSO3Conv(C, O), plain, feats60, gy60)
    assert torch.equal(inter_w['pm0'], inter_w['pm1']) and torch.equal(inter_w['k20'], inter_w['pm1'][:, :, ::3])
    assert torch.equal(inter_w['nopose'][1], inter_w['pm1'][1])
    out.update({'inter_w_posed': inter_w['pm1'], 'inter_w_nopose0': inter_w['nopose'][0]})
    save('so3_f64.npz', **out)
    size = os.path.getsize(os.path.join(HERE, 'so3_f64.npz'))
    assert size < 1000000, size


if __name__ == '__main__':
    main()
