"""tools/pointnet_max_time.py -- PointnetSO3Conv's embed + max over the points fused (vgtk.so3conv.pointnet_max over csrc/pointnet_max.hip)
against the composition the package had: so3_contract of the feature half of the weights + the rank-3 coordinate term + bias + torch.max,
which is PointnetSO3ConvOurs' max path (vgtk/so3conv/heads.py), on feats [16, 256, N, 60] -> [16, 256, 60], N = 2048 and 4096.

  python tools/pointnet_max_time.py [--out profiles/pointnet_max.txt]     one fresh process per N, each under its own `timeout`; stops at the
                                                                          first that fails
  python tools/pointnet_max_time.py --case N                              one N in this process -> one JSON line

Per case: both variants in the same process, ALTERNATING over ROUNDS rounds of STEPS steps after WARMUP steps each, timed with device events:
forward alone and forward + backward (gradients to feats, xyz, embed.weight, embed.bias); median and range over the rounds; the fp32-MFMA
floor of the products (2 B O C N A flop at 157.3 TFLOP/s) beside them.  Peak memory: torch.cuda.max_memory_allocated above what is
allocated before the step (the inputs), forward alone and forward + backward."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, O, A = 16, 256, 256, 60
ROUNDS, STEPS, WARMUP = 5, 10, 3


def case(n):
    sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, 'equi-articulated-pose_amd'))
    import torch
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(2410)
    feats = torch.randn(B, C, n, A, generator=gen, device=dev).requires_grad_(True)
    xyz = (torch.randn(B, 3, n, generator=gen, device=dev) * 0.3).requires_grad_(True)
    g = torch.randn(B, O, A, generator=gen, device=dev)
    torch.manual_seed(5)
    old = sptk.PointnetSO3ConvOurs(C, O, kanchor=A).to(dev)              # the composition, unchanged
    new = sptk.PointnetSO3Conv(C, O, kanchor=A).to(dev)
    new.embed.load_state_dict(old.embed.state_dict())
    variants = {'composed': (old, lambda: old(zptk.SphericalPointCloud(xyz, feats, None))),
                'fused': (new, lambda: new(zptk.SphericalPointCloud(xyz, feats, None)))}

    def step(name, backward):
        net, fn = variants[name]
        if not backward:
            with torch.no_grad():
                return fn()
        return torch.autograd.grad(fn(), [feats, xyz, net.embed.weight, net.embed.bias], g)

    with torch.no_grad():
        a_, b_ = variants['fused'][1](), variants['composed'][1]()
    agree = float((a_ - b_).abs().max() / b_.abs().max())
    del a_, b_
    flop = 2.0 * B * O * C * n * A
    out = {'shape': [B, C, O, n, A], 'feats_gb': round(B * C * n * A * 4 / 1e9, 3), 'map_gb': round(B * O * n * A * 4 / 1e9, 3),
           'fused_vs_composed_max_rel': agree, 'rounds': ROUNDS, 'steps': STEPS, 'fp32_mfma_floor_ms': round(flop / 157.3e12 * 1e3, 3)}
    times = {(v, k): [] for v in variants for k in ('fwd', 'fwd_bwd')}
    for name in variants:                                 # peak memory of one forward and of one forward + backward, and the warm-up
        for backward in (False, True):
            for _ in range(WARMUP):
                step(name, backward)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(name, backward)
            torch.cuda.synchronize()
            out[f'{name}_{"fwd_bwd" if backward else "fwd"}_peak_above_inputs_gb'] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)
    for _ in range(ROUNDS):
        for kind, backward in (('fwd', False), ('fwd_bwd', True)):
            for name in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(STEPS):
                    step(name, backward)
                e1.record()
                torch.cuda.synchronize()
                times[(name, kind)].append(e0.elapsed_time(e1) / STEPS)
    for name in variants:
        for kind in ('fwd', 'fwd_bwd'):
            ms = times[(name, kind)]
            out[f'{name}_{kind}'] = {'ms_median': round(statistics.median(ms), 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3)}
    for kind in ('fwd', 'fwd_bwd'):
        out[f'speedup_{kind}'] = round(out[f'composed_{kind}']['ms_median'] / out[f'fused_{kind}']['ms_median'], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', type=int)
    ap.add_argument('--points', type=int, nargs='+', default=[2048, 4096])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'pointnet_max.txt'))
    a = ap.parse_args()
    if a.case:
        return case(a.case)
    lines = ['tools/pointnet_max_time.py: embed + max over the points on feats [16, 256, N, 60] -> [16, 256, 60], fused (csrc/pointnet_max.hip) against '
             'the composition so3_contract + rank-3 term + torch.max; ms per step from device events; speedup = composed / fused']
    for n in a.points:
        cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--case', str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            lines.append(f'N = {n}: exit status {r.returncode}; nothing further was started')
            break
        lines.append(r.stdout.strip().splitlines()[-1])
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    return 0 if len(lines) == 1 + len(a.points) and 'exit status' not in lines[-1] else 1


if __name__ == '__main__':
    sys.exit(main())
