"""tests/golden/make_golden_intra2d.py -- golden vectors of IntraSO3Conv2D (so3conv/modules.py:L350-373 ->
intra_so3conv_grouping_2D, so3conv/functional.py:L2606-2627, + BasicSO3Conv, modules.py:L48-55), produced by RUNNING THE REFERENCE on
CPU in the build container (tests/golden/ref_import.py).  The anchor axis is 60 x 4 with the residual innermost; the 12-tap gather
acts on the 60-axis.  Pins that axis order against the reference itself, not against a restatement of it.  Data only.

  intra_2d.npz   feats [1,3,6,240], W [5,36], intra_idx [60,12], out [1,5,6,240], gy, and the autograd gradients gfeats, gW

Re-run:  python tests/golden/make_golden_intra2d.py"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference through ref_import)
from make_golden import save  # noqa: E402

sptk, zptk = MG.sptk, MG.zptk


def main():
    gen = torch.Generator().manual_seed(2406)
    B, C, O, P = 1, 3, 5, 6
    torch.manual_seed(2913)
    conv = sptk.IntraSO3Conv2D(C, O)
    feats = torch.randn(B, C, P, 240, generator=gen).requires_grad_(True)
    y = conv(zptk.SphericalPointCloud(torch.zeros(B, 3, P), feats, None)).feats
    assert tuple(y.shape) == (B, O, P, 240)
    gy = torch.randn(y.shape, generator=gen)
    gfe, gW = torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)
    save('intra_2d.npz', feats=feats, W=conv.basic_conv.W, intra_idx=conv.intra_idx.int(), out=y, gy=gy, gfeats=gfe, gW=gW)


if __name__ == '__main__':
    main()
