"""tools/orbit_chamfer_time.py -- time and memory of the reconstruction distances over the orbit, on this tree and on another built checkout
(the parent commit) in ONE run, the two alternating.

    python tools/orbit_chamfer_time.py [--parent OTHER_TREE] [--repeats 5] [--out profiles/orbit_chamfer.txt]

Legs, float32:
    slot     orbit_reconstruction_distances at (B,S,A,M,N) = (8,2,60,256,4096) and (16,2,60,256,4096)
    stage 0  (16,1,60,512,4096): global_orbit_distances where the tree has it, else the reference's expression
             (...pn_38_multi_stage.py:L432-440) through ChamferFunction
Per leg: forward ms, forward + backward ms with a gradient on every output (device events around groups of CALLS calls after a warm-up group,
median of GROUPS groups), and the peak of allocated memory above the inputs over one forward + backward.

Every measurement is a fresh process (`--measure TREE`) that imports only names both trees have (orbit_reconstruction_distances,
ChamferFunction); the driver starts them one after the other, this tree and the other in turn, `--repeats` times each, and reports the median
of the processes' figures with [min .. max].  It stops at the first process that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_SHAPES = [(8, 2, 60, 256, 4096), (16, 2, 60, 256, 4096)]
STAGE0_SHAPE = (16, 1, 60, 512, 4096)
CALLS, GROUPS = 10, 3
CHILD_SECONDS = 300


def measure(tree):
    """one process: -> a JSON line {leg: {'fwd_ms', 'fwd_bwd_ms', 'peak_bytes', 'path'}}"""
    sys.path.insert(0, tree); sys.path.insert(0, os.path.join(tree, 'equi-articulated-pose_amd'))
    import torch
    import extensions.chamfer_dist as cd
    from extensions.chamfer_dist import ChamferFunction, orbit_reconstruction_distances
    if not torch.cuda.is_available():
        sys.exit('orbit_chamfer_time: needs the GPU (a timing taken elsewhere says nothing)')
    dev = torch.device('cuda:0')
    stage0 = getattr(cd, 'global_orbit_distances', None)

    def stage0_reference(recon, ori):
        bz, ka, m, _ = recon.shape
        expanded = ori.transpose(-1, -2).contiguous().unsqueeze(1).contiguous().repeat(1, ka, 1, 1)
        r2o, o2r = ChamferFunction.apply(recon.contiguous().view(bz * ka, m, 3), expanded.contiguous().view(bz * ka, ori.shape[2], 3))
        return r2o.contiguous().view(bz, ka, -1).mean(dim=-1), o2r.contiguous().view(bz, ka, -1).mean(dim=-1)

    def timed(fn):
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
        return statistics.median(per_call)

    result = {}
    for shape in SLOT_SHAPES + [STAGE0_SHAPE]:
        b, s, a, m, n = shape
        gen = torch.Generator().manual_seed(2913)
        recon = (torch.randn(b, s, a, m, 3, generator=gen) * 0.3).to(dev).requires_grad_(True)
        ori = (torch.randn(b, 3, n, generator=gen) * 0.3).to(dev)
        labels = torch.nn.functional.one_hot(torch.randint(0, s, (b, n), generator=gen), s).float().to(dev)
        if shape == STAGE0_SHAPE:
            fn = stage0 or stage0_reference
            forward = lambda: fn(recon[:, 0], ori)
            path = 'global_orbit_distances' if stage0 else 'ChamferFunction on [B*A] copies'
        else:
            forward = lambda: orbit_reconstruction_distances(recon, ori, labels)
            path = 'orbit_reconstruction_distances'
        weights = [torch.randn(v.shape, generator=gen).to(dev) for v in forward()]

        def forward_backward():
            recon.grad = None
            torch.autograd.backward(list(forward()), weights)

        def forward_only():
            with torch.no_grad():
                forward()

        forward_backward()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        forward_backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        result['x'.join(map(str, shape))] = {'fwd_ms': timed(forward_only), 'fwd_bwd_ms': timed(forward_backward), 'peak_bytes': peak,
                                             'path': path}
    print('RESULT ' + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--measure', default=None, help='(internal) measure the built tree at this path and print one JSON line')
    ap.add_argument('--parent', default=None, help='another built checkout to alternate with (the parent commit)')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.measure:
        return measure(os.path.abspath(args.measure))
    if args.repeats < 5 and args.parent:
        sys.exit('orbit_chamfer_time: at least five repeats per version for a comparison')
    trees = [('this tree', ROOT)] + ([('parent', os.path.abspath(args.parent))] if args.parent else [])
    runs = {label: [] for label, _ in trees}
    for _ in range(args.repeats):
        for label, tree in trees:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), '--measure', tree], capture_output=True, text=True, timeout=CHILD_SECONDS)
            line = next((ln for ln in done.stdout.splitlines() if ln.startswith('RESULT ')), None)
            if done.returncode != 0 or line is None:
                sys.exit(f'orbit_chamfer_time: measuring {label} failed (exit {done.returncode}); nothing further is started\n{done.stdout}\n{done.stderr}')
            runs[label].append(json.loads(line[len('RESULT '):]))
            print(f'measured {label} ({len(runs[label])} of {args.repeats})', file=sys.stderr, flush=True)
    fmt = lambda v, unit: f'{statistics.median(v):9.3f} [{min(v):.3f} .. {max(v):.3f}] {unit}'
    lines = [f'orbit chamfer, float32: median over {args.repeats} processes per version, the versions alternating [min .. max]; per process the median of '
             f'{GROUPS} groups of {CALLS} calls after a warm-up group, device events; peak = allocated memory above the inputs over one forward + backward']
    for leg in runs['this tree'][0]:
        lines.append(f'(B,S,A,M,N) = ({leg.replace("x", ",")})')
        for label, _ in trees:
            rs = [r[leg] for r in runs[label]]
            lines.append(f'  {label:<10}{rs[0]["path"]:<34}forward {fmt([r["fwd_ms"] for r in rs], "ms")}   forward + backward '
                         f'{fmt([r["fwd_bwd_ms"] for r in rs], "ms")}   peak {fmt([r["peak_bytes"] / 2**20 for r in rs], "MiB")}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
