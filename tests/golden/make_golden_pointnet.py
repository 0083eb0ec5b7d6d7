"""tests/golden/make_golden_pointnet.py -- golden vectors of the pointnet aggregation by RUNNING THE REFERENCE classes PointnetSO3Conv and
PointnetSO3PoseConv (vgtk/vgtk/so3conv/modules.py:L376-449) on CPU in the build container (through tests/golden/ref_import.py, like
make_golden.py): the concatenation [feats ; A^T (xyz - mean)], nn.Conv2d, torch.max over the points, and autograd through all of it.

  pointnet_max.npz   (B, C, O, N) = (2, 5, 7, 37), kanchor 60 and 20, both classes.  Per anchor count `k`: the inputs k_xyz, k_feats and the
                     cotangent k_g (shared by the two classes); per class (`conv`, `pose`): the state_dict (k_conv_state_*), the output
                     k_conv_out [B,O,A] and the gradients of <g, out> to feats, xyz, embed.weight and embed.bias.  Data only.

Re-run:  python tests/golden/make_golden_pointnet.py"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference through ref_import)
from make_golden import save  # noqa: E402

B, C, O, N = 2, 5, 7, 37


def main():
    out = {}
    for ka in (60, 20):
        gen = torch.Generator().manual_seed(4100 + ka)
        xyz = torch.randn(B, 3, N, generator=gen) * 0.4 + 0.2
        feats = torch.randn(B, C, N, ka, generator=gen)
        g = torch.randn(B, O, ka, generator=gen)
        out.update({f'{ka}_xyz': xyz, f'{ka}_feats': feats, f'{ka}_g': g})
        for tag, make in (('conv', lambda: MG.sptk.PointnetSO3Conv(C, O, kanchor=ka)), ('pose', lambda: MG.sptk.PointnetSO3PoseConv(C, O, kanchor=ka))):
            torch.manual_seed(77 + ka + (100 if tag == 'pose' else 0))
            net = make()
            with torch.no_grad():
                net.embed.bias.uniform_(-0.5, 0.5)
            x, f = xyz.clone().requires_grad_(True), feats.clone().requires_grad_(True)
            res = net(MG.zptk.SphericalPointCloud(x, f, None))
            assert tuple(res.shape) == (B, O, ka)
            grads = torch.autograd.grad((res * g).sum(), [f, x, net.embed.weight, net.embed.bias])
            out.update({f'{ka}_{tag}_state_{n}': v.clone() for n, v in net.state_dict().items()})
            out.update({f'{ka}_{tag}_out': res, f'{ka}_{tag}_grad_feats': grads[0], f'{ka}_{tag}_grad_xyz': grads[1],
                        f'{ka}_{tag}_grad_weight': grads[2], f'{ka}_{tag}_grad_bias': grads[3]})
    save('pointnet_max.npz', **out)


if __name__ == '__main__':
    main()
