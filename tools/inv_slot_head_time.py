"""tools/inv_slot_head_time.py -- the last unary layer of InvOutBlockOursWithMask behind its contraction: BatchNorm2d (per-cloud statistics over
the member points) + ReLU + the mean over the members, fused (vgtk/so3conv/heads.py _NormActPointMean over csrc/heads.hip eap_bn_act_cloud_mean_*)
against the composition of the kernels the package had (_subset_batchnorm_act over csrc/bn_act.hip eap_bn_act_cloud_*, then slot_masked_mean over
csrc/heads.hip eap_slot_masked_mean_*), on y [B, c, P, A] = [16, 256, P, 60], P = 2048 and 4096.

  python tools/inv_slot_head_time.py [--out profiles/inv_slot_head.txt]     one fresh process per P, each under its own `timeout`; stops at the
                                                                            first that fails
  python tools/inv_slot_head_time.py --case P                               one P in this process -> one JSON line

Per case: both variants in the same process, ALTERNATING over ROUNDS rounds of STEPS steps after WARMUP steps each, timed with device events:
forward alone (statistics pass included) and forward + backward (gradient to y, gamma, beta, bias); median and range over the rounds.  Bytes are
counted from the passes over the [B,c,P,A] tensor of T bytes: forward 2 T fused (statistics, fused pass) against 4 T (statistics, apply read +
write, mean read); backward 3 T fused (reduce, apply read + write) against 6 T (mean backward write, reduce two reads, apply two reads + write).
Peak memory: torch.cuda.max_memory_allocated above what is allocated before the step (y and the small operands)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, A = 16, 256, 60
ROUNDS, STEPS, WARMUP = 5, 10, 3
PASSES = {'fused': {'fwd': 2, 'bwd': 3}, 'unfused': {'fwd': 4, 'bwd': 6}}


def case(p):
    sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, 'equi-articulated-pose_amd'))
    import torch
    import vgtk.so3conv.heads as H
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(2406)
    y = (torch.randn(B, C, p, A, generator=gen, device=dev) * 1.7 + 0.4).requires_grad_(True)
    bias = torch.randn(C, generator=gen, device=dev).requires_grad_(True)
    mask = (torch.rand(B, p, generator=gen, device=dev) > 0.1).float()
    inv_den = 1.0 / mask.sum(1)
    g = torch.randn(B, C, A, generator=gen, device=dev)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()

    def fused():
        return H._norm_act_point_mean(y, bias, mask, inv_den, mask, bn, 0.0)

    def unfused():
        return H.slot_masked_mean(H._subset_batchnorm_act(y, bias, mask, bn, 0.0), mask.view(B, 1, p))[:, 0]

    variants = {'unfused': unfused, 'fused': fused}

    def step(fn, backward):
        if not backward:
            with torch.no_grad():
                return fn()
        return torch.autograd.grad(fn(), [y, bias, bn.weight, bn.bias], g)

    with torch.no_grad():
        a_, b_ = fused(), unfused()
    agree = float((a_ - b_).abs().max() / b_.abs().max())
    tensor_bytes = B * C * p * A * 4
    out = {'shape': [B, C, p, A], 'tensor_gb': round(tensor_bytes / 1e9, 3), 'fused_vs_unfused_max_rel': agree, 'rounds': ROUNDS, 'steps': STEPS}
    times = {(v, k): [] for v in variants for k in ('fwd', 'fwd_bwd')}
    for name, fn in variants.items():                     # peak memory of one forward + backward, and the warm-up
        for backward in (False, True):
            for _ in range(WARMUP):
                step(fn, backward)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fn, True)
        torch.cuda.synchronize()
        out[name + '_peak_above_inputs_gb'] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)
    for _ in range(ROUNDS):
        for kind, backward in (('fwd', False), ('fwd_bwd', True)):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(STEPS):
                    step(fn, backward)
                e1.record()
                torch.cuda.synchronize()
                times[(name, kind)].append(e0.elapsed_time(e1) / STEPS)
    for name in variants:
        fwd, both = times[(name, 'fwd')], times[(name, 'fwd_bwd')]
        bwd = [t2 - t1 for t1, t2 in zip(fwd, both)]
        for kind, ms in (('fwd', fwd), ('bwd', bwd)):
            med = statistics.median(ms)
            nbytes = PASSES[name][kind] * tensor_bytes
            out[f'{name}_{kind}'] = {'ms_median': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'passes': PASSES[name][kind],
                                     'gb': round(nbytes / 1e9, 2), 'tb_per_s': round(nbytes / med / 1e9, 2)}
    for kind in ('fwd', 'bwd'):
        out[f'speedup_{kind}'] = round(out[f'unfused_{kind}']['ms_median'] / out[f'fused_{kind}']['ms_median'], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', type=int)
    ap.add_argument('--points', type=int, nargs='+', default=[2048, 4096])
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'inv_slot_head.txt'))
    a = ap.parse_args()
    if a.case:
        return case(a.case)
    lines = ['tools/inv_slot_head_time.py: BatchNorm2d (per-cloud statistics) + ReLU + member mean on y [16, 256, P, 60], fused against the unfused '
             'composition; ms per step from device events, bwd = (fwd + bwd) - fwd per round; bytes from pass counts']
    for p in a.points:
        cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--case', str(p)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            lines.append(f'P = {p}: exit status {r.returncode}; nothing further was started')
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
