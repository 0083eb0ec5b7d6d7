"""tools/slot_attention_time.py -- SlotAttention (SPConvNets/utils/slot_attention_spec_v2.py:L132-193), forward + backward: the package's
module (vgtk/so3conv/slots.py over csrc/slot_attention.hip) against the batched torch restatement of the same algebra on the device
(tests/slot_attention_common.py restated_forward: what a caller without the kernels has), at B = 16, N in {512, 4096}, d in {256, 316},
S = 2, iters = 3.

  python tools/slot_attention_time.py [--out FILE]          one JSON line per shape, in this process

Per shape: both variants ALTERNATE over ROUNDS rounds of STEPS steps after WARMUP steps each, timed with device events (median and range
over the rounds); the peak allocation of one step above what is allocated before it; the device kernels of one step counted with
torch.profiler ('not measured' where the profiler gives none).  The module's scores and pool passes alone, against a streaming copy of x:
bytes counted from the shapes, x read once per pass (the copy reads and writes x once each)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, ITERS = 16, 2, 3
SHAPES = [(512, 256), (512, 316), (4096, 256), (4096, 316)]
ROUNDS, STEPS, WARMUP = 5, 10, 3


def timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def kernel_count(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or 'not measured'
    except Exception as e:                                 # a count is a side figure: the timings stand without it
        return f'not measured ({type(e).__name__})'


def case(n, d):
    import torch
    import slot_attention_common as C
    import vgtk.so3conv as sptk
    from vgtk import _hip
    dev = torch.device('cuda:0')
    torch.manual_seed(2407)
    model = sptk.SlotAttention(S, d, iters=ITERS).to(dev)
    with torch.no_grad():
        for m in model.norm_input:
            m.weight.normal_(1.0, 0.3); m.bias.normal_(0.0, 0.3)
    leaf = (torch.relu(torch.randn(B, d, n, device=dev)) * 1.5 + 0.2).requires_grad_(True)          # channel-major storage, as the model has it
    noise = torch.randn(B, S, d, device=dev)
    w = (torch.randn(B, S, d, device=dev), torch.randn(B, S, d, device=dev) * 0.5, torch.randn(B, S, n, device=dev), torch.randn(B, S, n, device=dev) * 0.5)
    params = list(model.parameters())
    P = dict(model.named_parameters())

    def module():
        slots, attn = model(leaf.transpose(1, 2), noise=noise)
        return torch.autograd.grad(C.functional(slots, attn, w), [leaf] + params), slots, attn

    def restated():
        slots, attn = C.restated_forward(P, leaf.transpose(1, 2), noise, S, iters=ITERS)
        return torch.autograd.grad(C.functional(slots, attn, w), [leaf] + params), slots, attn

    variants = {'restated': restated, 'module': module}
    (ga, sa, aa), (gb, sb, ab) = module(), restated()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    x_bytes = B * d * n * 4
    out = {'shape': {'B': B, 'N': n, 'd': d, 'S': S, 'iters': ITERS}, 'x_mb': round(x_bytes / 1e6, 2),
           'module_vs_restated_max_rel': {'slots': rel(sa, sb), 'attn': rel(aa, ab), 'dx': rel(ga[0], gb[0])}, 'rounds': ROUNDS, 'steps': STEPS}
    del ga, sa, aa, gb, sb, ab
    for name, fn in variants.items():
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        out[name + '_peak_above_inputs_in_x'] = round((torch.cuda.max_memory_allocated() - base) / x_bytes, 2)
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(timed(fn, STEPS))
    for name, ms in times.items():
        out[name + '_fwd_bwd_ms'] = {'median': round(statistics.median(ms), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3)}
    out['restated_over_module'] = round(out['restated_fwd_bwd_ms']['median'] / out['module_fwd_bwd_ms']['median'], 2)
    # the two forward passes alone against a streaming copy
    x = leaf.detach()
    mean, rstd = _hip.slot_attn_stats(x, 1e-5)
    u, c0 = torch.randn(B, S, d, device=dev) / d ** 0.5, torch.randn(B, S, device=dev)
    attn = _hip.slot_attn_scores_fwd(x, mean, rstd, u, c0, 1e-8)
    dst = torch.empty_like(x)
    passes = {'stats (2 reads)': (lambda: _hip.slot_attn_stats(x, 1e-5), 2), 'scores': (lambda: _hip.slot_attn_scores_fwd(x, mean, rstd, u, c0, 1e-8), 1),
              'pool': (lambda: _hip.slot_attn_pool(x, mean, rstd, attn), 1), 'copy (read + write)': (lambda: dst.copy_(x), 2)}
    out['passes_gb_per_s'] = {}
    for name, (fn, reads) in passes.items():
        for _ in range(WARMUP):
            fn()
        ms = statistics.median(timed(fn, 50) for _ in range(ROUNDS))
        out['passes_gb_per_s'][name] = {'ms': round(ms, 4), 'gb_per_s': round(reads * x_bytes / ms / 1e6, 1)}
    for name, fn in variants.items():
        out[name + '_kernels_per_step'] = kernel_count(fn)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    a = ap.parse_args()
    for p in (HERE, os.path.join(HERE, 'equi-articulated-pose_amd'), os.path.join(HERE, 'tests')):
        sys.path.insert(0, p)
    lines = ['tools/slot_attention_time.py: SlotAttention forward + backward, the module against the torch restatement on the device; ms per step from '
             'device events; measured on one MI355X']
    for n, d in SHAPES:
        lines.append(json.dumps(case(n, d)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
