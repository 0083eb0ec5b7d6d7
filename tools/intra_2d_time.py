"""tools/intra_2d_time.py -- IntraSO3Conv2D (the (60, 4) anchor axis of `use_2d`), forward and forward + backward (gradients to the features
and the weights), from device events, with the peak of allocated memory above the inputs.

  python tools/intra_2d_time.py --compare PARENT_ROOT     (b, c, o, p) = (2, 64, 64, 512), a shape the tensor form of the parent commit still
                                                          holds: GROUPS groups per tree, the two trees ALTERNATING (one fresh process per
                                                          group, parent first), median and range per tree; then, in this tree only, one
                                                          shape the tensor form cannot hold (--large)
  python tools/intra_2d_time.py --group [--root ROOT] [--shape b c o p] [--steps n]
                                                          one group in the tree at ROOT (default: this one) -> one JSON line

PARENT_ROOT is a checkout of the parent commit with its library built.  Record: profiles/intra_2d.txt."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS, WARMUP = 5, 2
SHAPE = (2, 64, 64, 512)
LARGE = (8, 512, 512, 4096)           # the 12-tap tensor alone: 193 GB


def group(root, shape, steps):
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'equi-articulated-pose_amd'))
    import torch
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    from vgtk import _hip
    assert os.path.abspath(_hip.LIB_PATH).startswith(os.path.abspath(root) + os.sep), _hip.LIB_PATH
    dev = torch.device('cuda:0')
    b, c, o, p = shape
    gen = torch.Generator(device=dev).manual_seed(2406)
    torch.manual_seed(2913)
    conv = sptk.IntraSO3Conv2D(c, o).to(dev)
    feats = torch.randn(b, c, p, 240, generator=gen, device=dev).requires_grad_(True)
    gy = torch.randn(b, o, p, 240, generator=gen, device=dev)

    def forward():
        return conv(zptk.SphericalPointCloud(None, feats, None)).feats

    def both():
        return torch.autograd.grad(forward(), [feats, conv.basic_conv.W], gy)

    out = {'root': root, 'shape': list(shape), 'steps': steps}
    for name, fn in (('fwd', forward), ('fwd_bwd', both)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.set_grad_enabled(name != 'fwd'):
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            out[name + '_peak_mb'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
        out[name + '_ms'] = round(e0.elapsed_time(e1) / steps, 3)
    print(json.dumps(out), flush=True)


def child(root, shape, steps):
    cmd = [sys.executable, os.path.abspath(__file__), '--group', '--root', root, '--steps', str(steps), '--shape', *map(str, shape)]
    line = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout.strip().splitlines()[-1]
    return json.loads(line)


def summary(tag, rows):
    rec = {'tree': tag, 'shape': rows[0]['shape'], 'groups': len(rows), 'steps_per_group': rows[0]['steps']}
    for k in ('fwd', 'fwd_bwd'):
        ms = [r[k + '_ms'] for r in rows]
        rec.update({k + '_ms_median': round(statistics.median(ms), 3), k + '_ms_min': min(ms), k + '_ms_max': max(ms),
                    k + '_peak_mb': max(r[k + '_peak_mb'] for r in rows)})
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--compare', metavar='PARENT_ROOT')
    ap.add_argument('--group', action='store_true')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--shape', type=int, nargs=4, default=SHAPE)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--large', type=int, nargs=4, default=LARGE)
    a = ap.parse_args()
    if a.group:
        return group(os.path.abspath(a.root), tuple(a.shape), a.steps)
    if not a.compare:
        ap.error('--compare PARENT_ROOT or --group')
    rows = {'parent': [], 'this': []}
    for _ in range(GROUPS):
        for tag, root in (('parent', os.path.abspath(a.compare)), ('this', HERE)):
            rows[tag].append(child(root, tuple(a.shape), a.steps))
    for tag in ('parent', 'this'):
        summary(tag, rows[tag])
    summary('this (the parent cannot hold the 12-tap tensor of this shape)', [child(HERE, tuple(a.large), 2) for _ in range(2)])


if __name__ == '__main__':
    main()
