"""tools/head_pooling_wide_time.py -- the three head poolings on a `use_2d` feature map, x [4, 256, 2048, 240] (2.01 GB): the wide kernels
(csrc/heads.hip at Q = 64, through vgtk.so3conv.anchor_attention_pool / masked_max / slot_masked_mean) against the torch expressions the wrappers
ran at 240 anchors before the kernels existed (the fallback functions of vgtk/so3conv/heads.py themselves).  Forward and forward + backward,
3 repeats after a warm-up, device events; the peak memory above the inputs; the achieved GB/s of every kernel on its algorithmic bytes.
    python tools/head_pooling_wide_time.py [--out profiles/head_pooling_wide.txt] [--shape 4 256 2048 240] [--slots 8 1]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'equi-articulated-pose_amd'))
import torch

import vgtk.so3conv as sptk
from vgtk import _hip
from vgtk.so3conv import heads

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'head_pooling_wide.txt'))
ap.add_argument('--shape', type=int, nargs=4, default=[4, 256, 2048, 240])
ap.add_argument('--slots', type=int, nargs='+', default=[8, 1])
args = ap.parse_args()
dev = torch.device('cuda:0')
b, c, n, na = args.shape
T, REPEATS = 3.0, 3
gen = torch.Generator(device=dev).manual_seed(5)
x = torch.randn(b, c, n, na, device=dev, generator=gen).requires_grad_(True)
logits = torch.randn(b, n, na, device=dev, generator=gen).requires_grad_(True)
member = (torch.rand(b, n, device=dev, generator=gen) > 0.4).float()
slots = {ns: torch.rand(b, ns, n, device=dev, generator=gen) for ns in args.slots}
GB = x.numel() * 4 / 1e9
small = lambda *shape: 4 * int(torch.Size(shape).numel()) / 1e9

# operation -> (kernel side, torch side, gradient inputs, algorithmic GB forward, algorithmic GB backward)
OPS = {
    'anchor_attention_pool': (lambda: sptk.anchor_attention_pool(x, logits, T)[0], lambda: heads._anchor_attention_pool_torch(x, logits, T)[0],
                              [x, logits], GB + 2 * small(b, n, na) + small(b, c, n), 2 * GB + 2 * small(b, n, na) + small(b, c, n)),
    'masked_max': (lambda: sptk.masked_max(x, member), lambda: heads._masked_max_torch(x, member), [x],
                   GB + 2 * small(b, c, na), GB + 2 * small(b, c, na)),
}
for ns, w in slots.items():                     # (8: every slot of the pose head at once; 1: pose_head_over_subsets' masked mean)
    OPS[f'slot_masked_mean, {ns} slot(s)'] = (lambda w=w: sptk.slot_masked_mean(x, w), lambda w=w: heads._slot_masked_mean_torch(x, w), [x],
                                             GB + small(b, ns, c, na), GB + small(b, ns, c, na))


def measure(run, inputs):
    """-> forward ms, forward + backward ms (each: the REPEATS values), peak bytes above what was allocated before the call"""
    fwd, both, peak = [], [], 0
    for it in range(1 + REPEATS):                             # the first is the warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        out = run()
        e1.record()
        grads = torch.autograd.grad(out, inputs, torch.ones_like(out))
        e2.record()
        torch.cuda.synchronize()
        if it:
            fwd.append(e0.elapsed_time(e1)); both.append(e0.elapsed_time(e2))
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del out, grads
    return fwd, both, peak


def kernel_times(run, inputs):
    """device time of every entry the kernel side calls: {entry: [ms per repeat]}"""
    seen = {}
    real = _hip.call

    def timed(name, ref, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); r = real(name, ref, *a, **k); e1.record()
        seen.setdefault(name, []).append((e0, e1))
        return r
    _hip.call = timed
    try:
        for it in range(1 + REPEATS):
            out = run()
            torch.autograd.grad(out, inputs, torch.ones_like(out))
            torch.cuda.synchronize()
    finally:
        _hip.call = real
    return {k: [a.elapsed_time(z) for a, z in v[len(v) // (1 + REPEATS):]] for k, v in seen.items()}


fmt = lambda v: f'{sorted(v)[len(v) // 2]:8.2f} ms ({min(v):.2f} - {max(v):.2f})'
lines = [f'Head poolings on a use_2d map, x [{b}, {c}, {n}, {na}] float32 ({GB:.2f} GB), {torch.cuda.get_device_name(0)}; tools/head_pooling_wide_time.py.',
         f'kernel: csrc/heads.hip at Q = 64 through the wrappers of vgtk.so3conv; torch: the expressions the wrappers ran at {na} anchors without the',
         f'kernels (vgtk/so3conv/heads.py: _anchor_attention_pool_torch, _masked_max_torch, _slot_masked_mean_torch).  Median (min - max) of {REPEATS} repeats after',
         'a warm-up, device events around the whole call; peak = the most device memory in use above the inputs during forward + backward.', '']
for name, (kern, ref, inputs, gb_f, gb_b) in OPS.items():
    lines.append(name)
    res = {}
    for side, run in (('kernel', kern), ('torch', ref)):
        fwd, both, peak = measure(run, inputs)
        res[side] = (fwd, both)
        lines.append(f'   {side:<7} forward {fmt(fwd)}   forward + backward {fmt(both)}   peak {peak / 1e9:6.2f} GB')
    for tag, i in (('forward', 0), ('forward + backward', 1)):
        k, t = res['kernel'][i], res['torch'][i]
        lines.append(f'   {tag}: torch / kernel = {sorted(t)[1] / sorted(k)[1]:.2f}; the kernel is ' +
                     ('faster beyond' if max(k) < min(t) - (max(t) - min(t)) else 'NOT faster beyond') + " the torch side's repeat spread")
    for entry, ms in kernel_times(kern, inputs).items():
        gb = gb_b if '_bwd_' in entry else gb_f
        lines.append(f'   {entry:<38} {fmt(ms)}   {gb:.2f} GB algorithmic: {gb / (sorted(ms)[len(ms) // 2] * 1e-3):.0f} GB/s')
    lines.append('')
text = '\n'.join(lines)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, 'w').write(text)
print(text)
