"""tools/use2d_permuted_time.py -- one `use_2d` inter conv layer whose poses really permute the residual index, forward + backward: 2 x 512
points, 64 -> 128 channels, 64 neighbours, r = 0.16, sigma = 0.0128, one rotation per rigid part + 7 points with a rotation of their own.
Three variants: default routing (the 'residual map' kernels, csrc/so3_inter_res.hip; on a tree without them the tensor form), the tensor
form (FORCE_GENERAL_2D), and the same cloud with permute_modes=0 (four fused convolutions: the floor).  Per variant: time per forward +
backward from device events, median and range of 5 timed groups after a warm-up, and the peak of allocated memory above the inputs.
Run it in the parent's tree and in this one alternately on one machine to compare them (record: profiles/use2d_residual_map.txt)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'equi-articulated-pose_amd'))
import torch  # noqa: E402
import synth_clouds  # noqa: E402
import vgtk.so3conv as sptk  # noqa: E402
import vgtk.so3conv.functional as L  # noqa: E402
import vgtk.spconv as zptk  # noqa: E402

GROUPS, WARMUP = 5, 2
B, P, C, O, NN, RADIUS, SIGMA = 2, 512, 64, 128, 64, 0.16, 0.0128


def quat_to_R(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(*q.shape[:-1], 3, 3)


def main():
    dev = torch.device('cuda:0')
    xyz_np, lab, _ = synth_clouds.laptop_batch(95, B, P)
    gen = torch.Generator().manual_seed(79)
    R = quat_to_R(torch.randn(B, 2, 4, generator=gen))
    pose = torch.eye(4).repeat(B, P, 1, 1)
    for b in range(B):
        pose[b, :, :3, :3] = R[b][torch.from_numpy(lab[b]).long()]
    pose[0, [3, 5, 64, 65, 127, 255, P - 1], :3, :3] = quat_to_R(torch.randn(7, 4, generator=gen))
    xyz, pose = torch.from_numpy(xyz_np).to(dev), pose.to(dev)
    feats = torch.randn(B, C, P, 240, generator=gen).to(dev).requires_grad_(True)
    gy = torch.randn(B, O, P, 240, generator=gen).to(dev)
    for name, pm, forced, steps in (('default routing', 1, False, 10), ('tensor form', 1, True, 3), ('permute_modes=0', 0, False, 10)):
        L.FORCE_GENERAL_2D = forced
        torch.manual_seed(2913)
        conv = sptk.InterSO3PoseConv(C, O, 1, 1, RADIUS, SIGMA, NN, kanchor=60, permute_modes=pm, use_2d=True).to(dev)

        def step():
            y = conv(zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
            return torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)

        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        L.FORWARD_LOG = []
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        log, L.FORWARD_LOG = L.FORWARD_LOG, None
        peak = torch.cuda.max_memory_allocated() - base
        times = []
        for _ in range(GROUPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / steps)
        regimes = sorted({str(e.get('regime', 'fused convolution')) for e in log}) or ['tensor ops']
        print(json.dumps({'variant': name, 'regime': regimes, 'ms_median': round(statistics.median(times), 3), 'ms_min': round(min(times), 3),
                          'ms_max': round(max(times), 3), 'steps_per_group': steps, 'groups': GROUPS, 'peak_mb': round(peak / 2 ** 20, 1),
                          'shape': f'{B} x {P} points, {C} -> {O}, {NN} neighbours'}), flush=True)
    L.FORCE_GENERAL_2D = False


if __name__ == '__main__':
    main()
