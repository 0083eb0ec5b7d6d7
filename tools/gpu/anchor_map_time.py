"""One inter conv layer with a rotation per point, forward + backward: 2 x 4096 points, 64 -> 128 channels, 64 neighbours --
on the 20-anchor set (the 'anchor map' regime: csrc/so3_anchor_map.hip, csrc/so3_inter_map.hip) and, beside it, on the 60-anchor group
(the permuted list kernels).  Meant to run under `rocprofv3 --kernel-trace --stats` (tools/gpu/anchor_map_trace.sh)."""
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
for p in (ROOT, os.path.join(ROOT, 'equi-articulated-pose_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
import synth_clouds  # noqa: E402
import vgtk.so3conv as sptk  # noqa: E402
import vgtk.so3conv.functional as L  # noqa: E402
import vgtk.spconv as zptk  # noqa: E402

STEPS = 4


def rotations(gen, n):
    q = torch.randn(n, 4, generator=gen)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(n, 3, 3)


def main():
    dev = torch.device('cuda:0')
    B, P, c, o = 2, 4096, 64, 128
    _, _, radius, sigma = synth_clouds.backbone_layers(4096)[1]
    xyz = torch.from_numpy(synth_clouds.laptop_batch(0, B, P)[0]).to(dev)
    gen = torch.Generator().manual_seed(11)
    pose = torch.eye(4).repeat(B, P, 1, 1)
    pose[:, :, :3, :3] = rotations(gen, B * P).view(B, P, 3, 3)
    pose = pose.to(dev)
    for na in (20, 60):
        torch.manual_seed(2913)
        conv = sptk.InterSO3PoseConv(c, o, 1, 1, radius, sigma, 64, kanchor=na, permute_modes=1).to(dev)
        feats = torch.randn(B, c, P, na, generator=gen).to(dev).requires_grad_(True)
        gy = torch.randn(B, o, P, na, generator=gen).to(dev)
        for step in range(STEPS + 1):
            if step == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            L.BACKWARD_LOG = []
            y = conv(zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
            torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)
            log, L.BACKWARD_LOG = L.BACKWARD_LOG, None
        torch.cuda.synchronize()
        print(f'{na} anchors: {B} x {P} points, {c} -> {o}, 64 neighbours, a rotation per point: backward regime {log[0]["regime"]!r}, '
              f'{(time.perf_counter() - t0) / STEPS * 1e3:.2f} ms per forward + backward (wall, {STEPS} steps after one warm-up)', flush=True)


if __name__ == '__main__':
    main()
