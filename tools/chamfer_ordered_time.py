"""tools/chamfer_ordered_time.py -- chamfer forward, scatter backward (float32, atomicAdd) and ordered backward (csrc/chamfer.hip) at
config 3's pair [16,4096,3] x [16,4096,3] and the stage-0 shape [960,512,3] x [960,4096,3], float32 and float64.

HIP events around groups of CALLS calls; one warm-up group, then the median of five groups (min and max beside it: the spread a
difference has to exceed).  Before anything is timed the ordered float32 result is compared with the scatter's at the timed size.
    python tools/chamfer_ordered_time.py [--out profiles/chamfer_ordered.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'equi-articulated-pose_amd'))
import torch

import chamfer

SHAPES = [('config 3 pair', 16, 4096, 4096), ('stage 0', 960, 512, 4096)]
CALLS, GROUPS = 20, 5


def timed(fn):
    """-> (median, min, max) ms per call over GROUPS groups of CALLS calls, after one warm-up group"""
    per_call = []
    for group in range(GROUPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if group:
            per_call.append(e0.elapsed_time(e1) / CALLS)
    per_call.sort()
    return per_call[GROUPS // 2], per_call[0], per_call[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('chamfer_ordered_time: needs the GPU (a timing taken elsewhere says nothing)')
    dev = torch.device('cuda:0')
    lines = [f'chamfer on {torch.cuda.get_device_name(0)}: ms per call of chamfer.forward / chamfer.backward (output allocation + two launches), median of {GROUPS} groups of {CALLS} calls [min .. max], HIP events, one warm-up group',
             f'{"shape":<42}{"width":<9}{"forward":<27}{"scatter backward":<27}{"ordered backward":<29}ordered / forward']
    for label, b, n, m in SHAPES:
        gen = torch.Generator().manual_seed(2913)
        c1, c2 = torch.randn(b, n, 3, dtype=torch.float64, generator=gen), torch.randn(b, m, 3, dtype=torch.float64, generator=gen)
        w1, w2 = torch.randn(b, n, dtype=torch.float64, generator=gen), torch.randn(b, m, dtype=torch.float64, generator=gen)
        for dtype in (torch.float32, torch.float64):
            x1, x2, g1, g2 = (t.to(dtype).to(dev) for t in (c1, c2, w1, w2))
            _, _, i1, i2 = chamfer.forward(x1, x2)
            ordered = chamfer.backward(x1, x2, i1, i2, g1, g2, ordered=True)
            note = ''
            if dtype == torch.float32:
                scatter = chamfer.backward(x1, x2, i1, i2, g1, g2, ordered=False)
                err = max(((o - s).abs().max() / s.abs().max()).item() for o, s in zip(ordered, scatter))
                assert err < 1e-5, err
                note = f'   (ordered against scatter: {err:.1e} of the largest gradient)'
            fmt = lambda t: f'{t[0]:8.4f} [{t[1]:.4f} .. {t[2]:.4f}]'
            fwd = timed(lambda: chamfer.forward(x1, x2))
            sc = timed(lambda: chamfer.backward(x1, x2, i1, i2, g1, g2, ordered=False)) if dtype == torch.float32 else None
            od = timed(lambda: chamfer.backward(x1, x2, i1, i2, g1, g2, ordered=True))
            lines.append(f'{label + f" [{b},{n},3] x [{b},{m},3]":<42}{str(dtype).replace("torch.", ""):<9}{fmt(fwd):<27}'
                         f'{(fmt(sc) if sc else "-"):<27}{fmt(od):<29}{od[0] / fwd[0]:.2f}{note}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
