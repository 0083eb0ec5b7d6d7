"""tools/inv_slot_head_wide_time.py -- the sibling of tools/inv_slot_head_time.py for the 240-anchor map of a `use_2d` backbone: the last unary
layer of InvOutBlockOursWithMask behind its contraction (BatchNorm2d with per-cloud statistics over the member points + ReLU + the mean over the
members) and the per-cloud norm of the pose heads' unary stacks, on y [B, c, P, A] = [4, 256, 2048, 240] float32 (2.01 GB, the shape of
profiles/head_pooling_wide.txt).

  python tools/inv_slot_head_wide_time.py [--out profiles/inv_slot_head_wide.txt]      the measurement in one fresh child process under `timeout`
  python tools/inv_slot_head_wide_time.py --case                                       the measurement in this process -> one JSON line

Two groups, every form of a group in the same process, ALTERNATING over ROUNDS rounds of STEPS steps after WARMUP steps each, timed with device
events, statistics pass included; forward alone and forward + backward (gradient to y, gamma, beta, bias):
  norm + point mean   fused     vgtk/so3conv/heads.py _norm_act_point_mean over csrc/heads.hip at Q = 64 eap_bn_act_cloud_mean_wide_*
                      torch     _norm_act_point_mean_torch, the expression that ran at 240 anchors before the wide kernels
                      composed  _subset_batchnorm_act (csrc/bn_act.hip eap_bn_act_cloud_*) + slot_masked_mean (csrc/heads.hip at Q = 64)
  per-cloud norm      kernels   _subset_batchnorm_act
                      torch     _subset_batchnorm_act_torch
Per form: median and range over the rounds, and the peak of torch.cuda.max_memory_allocated above what is allocated before a forward + backward
step (y and the small operands).  Verdict per comparison, the routing rule of the package: the kernels keep a route where their SLOWEST round
lies below the comparator's FASTEST round."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, P, A = 4, 256, 2048, 240
ROUNDS, STEPS, WARMUP = 5, 10, 3


def case():
    sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, 'equi-articulated-pose_amd'))
    import torch
    import vgtk.so3conv.heads as H
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(2406)
    y = (torch.randn(B, C, P, A, generator=gen, device=dev) * 1.7 + 0.4).requires_grad_(True)
    bias = torch.randn(C, generator=gen, device=dev).requires_grad_(True)
    mask = (torch.rand(B, P, generator=gen, device=dev) > 0.1).float()
    inv_den = 1.0 / mask.sum(1)
    g_mean = torch.randn(B, C, A, generator=gen, device=dev)
    g_map = torch.randn(B, C, P, A, generator=gen, device=dev)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    assert H._anchor_rows_wide(A)
    groups = {
        'norm + point mean': (g_mean, {
            'torch': lambda: H._norm_act_point_mean_torch(y, bias, mask, inv_den, mask, bn, 0.0),
            'composed': lambda: H.slot_masked_mean(H._subset_batchnorm_act(y, bias, mask, bn, 0.0), mask.view(B, 1, P))[:, 0],
            'fused': lambda: H._norm_act_point_mean(y, bias, mask, inv_den, mask, bn, 0.0)}),
        'per-cloud norm': (g_map, {
            'torch': lambda: H._subset_batchnorm_act_torch(y, bias, mask, bn, 0.0),
            'kernels': lambda: H._subset_batchnorm_act(y, bias, mask, bn, 0.0)}),
    }

    def step(fn, g, backward):
        if not backward:
            with torch.no_grad():
                return fn()
        return torch.autograd.grad(fn(), [y, bias, bn.weight, bn.bias], g)

    out = {'shape': [B, C, P, A], 'tensor_gb': round(B * C * P * A * 4 / 1e9, 3), 'device': torch.cuda.get_device_name(0), 'rounds': ROUNDS,
           'steps': STEPS, 'groups': {}}
    for title, (g, variants) in groups.items():
        res = {}
        with torch.no_grad():
            vals = {name: fn() for name, fn in variants.items()}
        ref = vals['torch']
        res['max_rel_to_torch'] = {name: float((v - ref).abs().max() / ref.abs().max()) for name, v in vals.items() if name != 'torch'}
        del vals, ref
        peaks = {}
        for name, fn in variants.items():                     # the warm-up, then the peak memory of one forward + backward
            for backward in (False, True):
                for _ in range(WARMUP):
                    step(fn, g, backward)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(fn, g, True)
            torch.cuda.synchronize()
            peaks[name] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)
        times = {(v, k): [] for v in variants for k in ('fwd', 'fwd_bwd')}
        for _ in range(ROUNDS):
            for kind, backward in (('fwd', False), ('fwd_bwd', True)):
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(STEPS):
                        step(fn, g, backward)
                    e1.record()
                    torch.cuda.synchronize()
                    times[(name, kind)].append(e0.elapsed_time(e1) / STEPS)
        for name in variants:
            res[name] = {'peak_above_inputs_gb': peaks[name]}
            for kind in ('fwd', 'fwd_bwd'):
                ms = times[(name, kind)]
                res[name][kind] = {'ms_median': round(statistics.median(ms), 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3)}
        out['groups'][title] = res
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def report(r):
    lines = [f"Per-cloud BatchNorm2d + ReLU (+ member mean) on a use_2d map, y {r['shape']} float32 ({r['tensor_gb']} GB), {r['device']}; "
             'tools/inv_slot_head_wide_time.py.',
             f"Per-cloud statistics over the member points, statistics pass included; every form of a group alternates in one process, {r['rounds']} rounds "
             f"of {r['steps']} steps after a warm-up,",
             'device events around the round; ms per step as median (min - max) over the rounds; peak = the most device memory in use above the inputs during',
             'one forward + backward.  A route stays on the kernels where their slowest round lies below the comparator\'s fastest round.', '']
    for title, res in r['groups'].items():
        lines.append(title)
        ours = 'fused' if 'fused' in res else 'kernels'
        for name, v in res.items():
            if name == 'max_rel_to_torch':
                continue
            f, fb = v['fwd'], v['fwd_bwd']
            lines.append(f"   {name:9s} forward {f['ms_median']:8.2f} ms ({f['ms_min']:.2f} - {f['ms_max']:.2f})   forward + backward {fb['ms_median']:8.2f} ms "
                         f"({fb['ms_min']:.2f} - {fb['ms_max']:.2f})   peak {v['peak_above_inputs_gb']:6.2f} GB")
        for other in res:
            if other in ('max_rel_to_torch', ours):
                continue
            for kind, label in (('fwd', 'forward'), ('fwd_bwd', 'forward + backward')):
                a, b = res[ours][kind], res[other][kind]
                keeps = a['ms_max'] < b['ms_min']
                lines.append(f"   {label}: {other} / {ours} = {b['ms_median'] / a['ms_median']:.2f}; slowest {ours} round {a['ms_max']:.2f} ms, fastest {other} round "
                             f"{b['ms_min']:.2f} ms: " + ('the kernels keep the route' if keeps else 'NOT separated: the route goes back to ' + other))
        lines.append('   largest difference to the torch form, relative to its largest element: ' +
                     ', '.join(f'{k} {v:.1e}' for k, v in res['max_rel_to_torch'].items()))
        lines.append('')
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', action='store_true')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'inv_slot_head_wide.txt'))
    a = ap.parse_args()
    if a.case:
        return case()
    r = subprocess.run(['timeout', '-k', '10', '420', sys.executable, os.path.abspath(__file__), '--case'], stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print(f'exit status {r.returncode}; nothing was recorded')
        return 1
    text = report(json.loads(r.stdout.strip().splitlines()[-1]))
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
