"""tools/native_ordered_time.py -- the ordered backwards of csrc/native_ordered.hip against the atomicAdd scatter kernels they stand
beside (csrc/gathering.hip, csrc/zpconv.hip), through the Python operators of vgtk.cuda with ordered=True / ordered=False:

    gather   grad [8, 64, 262144] onto 4097 points, float32 and float64
    intra    8 x 64 x 4096 points, table (na_in, na_out, ann, ks) = (60, 60, 12, 24), float32 and float64
    inter    one 1024-point cloud, 60 anchors, 24 kernel points, 64 neighbours (one list per point), 16 channels, float64

Every (case, kernel) pair is timed in a PROCESS OF ITS OWN, scatter and ordered alternating, ROUNDS rounds: a child builds its
operands from a seed, runs one warm-up group, then GROUPS groups of calls between two HIP events (as many calls as fill ~0.2 s, at
most 20); the parent reports the median of all groups of all rounds with their range.  The ordered child first compares its result
with the scatter's at the timed size, and times the list building apart: the two list-builder entries (eap_inv_lists_rows,
eap_inv_lists_entries_ws) on the very index the operator hands them -- for the inter op the anchor-major copy [b*na, np, ks*ann], made
here with torch -- so the "lists" column is part of the "ordered" column, not on top of it.
    python tools/native_ordered_time.py [--out profiles/native_ordered_backward.txt]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'equi-articulated-pose_amd'))

CASES = [('gather', 'f32'), ('gather', 'f64'), ('intra', 'f32'), ('intra', 'f64'), ('inter', 'f64')]
LABELS = {'gather': 'gather [8,64,262144] -> [8,64,4097]', 'intra': 'intra 8 x 64 x 4096 points, (60,60,12,24)',
          'inter': 'inter 1 x 1024 points, 60 x 24 x 64, c = 16'}
ROUNDS, GROUPS, MAX_CALLS, GROUP_SECONDS = 2, 3, 20, 0.2
CHILD_SECONDS = 240


def timed(torch, fn):
    """-> ms per call of every group: one call to size the groups, one warm-up group, GROUPS timed groups"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    calls = max(1, min(MAX_CALLS, int(GROUP_SECONDS * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    per_call = []
    for group in range(GROUPS + 1):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if group:
            per_call.append(e0.elapsed_time(e1) / calls)
    return per_call


def child(op, width, kernel):
    import torch
    import vgtk.cuda.gathering as G
    import vgtk.cuda.zpconv as Z
    from vgtk import _hip
    if not torch.cuda.is_available():
        sys.exit('native_ordered_time: needs the GPU (a timing taken elsewhere says nothing)')
    dev, dt = torch.device('cuda:0'), torch.float32 if width == 'f32' else torch.float64
    gen = torch.Generator(device=dev).manual_seed(2913)
    randn = lambda *shape: torch.randn(*shape, dtype=dt, device=dev, generator=gen)
    randint = lambda hi, *shape: torch.randint(0, hi, shape, dtype=torch.int32, device=dev, generator=gen)
    if op == 'gather':
        b, c, n, m = 8, 64, 4097, 262144
        idx, g = randint(n, b, m), randn(b, c, m)
        run = lambda ordered: G.gather_points_backward(g, idx, n, ordered=ordered)
        lists = lambda: _hip.inv_lists(idx.view(b, m, 1), n)
    elif op == 'intra':
        b, c, np_, na, ann, ks = 8, 64, 4096, 60, 12, 24
        idx, w, g = randint(na, na, ann), randn(na, ks, ann), randn(b, c, ks, np_, na)
        run = lambda ordered: Z.intra_zpconv_backward(idx, w, g, na, ordered=ordered)
        lists = None                                                           # (the table is inverted inside the kernel)
    else:
        b, c, np_, nq, na, ks, ann = 1, 16, 1024, 1024, 60, 24, 64
        idx = randint(nq, b, np_, 1, 1, ann).expand(b, np_, na, ks, ann).contiguous()
        w, g = randn(b, np_, na, ks, ann), randn(b, c, ks, np_, na)
        run = lambda ordered: Z.inter_zpconv_backward(idx, w, g, nq, ordered=ordered)
        idxT = idx.permute(0, 2, 1, 3, 4).reshape(b * na, np_, ks * ann).contiguous()
        lists = lambda: _hip.inv_lists(idxT, nq)
    result = {}
    if kernel == 'ordered':
        o, s = run(True), run(False)
        result['against_scatter'] = ((o - s).abs().max() / s.abs().max()).item()
        del o, s
        if lists is not None:
            result['lists_ms'] = timed(torch, lists)
    result['ms'] = timed(torch, lambda: run(kernel == 'ordered'))
    print('RESULT ' + json.dumps(result))


def summary(values):
    values = sorted(values)
    return f'{values[len(values) // 2]:10.3f} [{values[0]:.3f} .. {values[-1]:.3f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', nargs=3, metavar=('OP', 'WIDTH', 'KERNEL'), default=None)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    lines = [f'ms per call of the Python operator (output allocation included), median of {ROUNDS} processes x {GROUPS} groups [min .. max]; scatter and '
             'ordered in alternating processes; "lists" = the two list-builder entries alone, a part of "ordered"',
             f'{"case":<46}{"width":<7}{"scatter":<36}{"ordered":<36}{"lists":<36}ordered / scatter   ordered against scatter']
    for op, width in CASES:
        got = {'scatter': [], 'ordered': [], 'lists': []}
        err = None
        for _ in range(ROUNDS):
            for kernel in ('scatter', 'ordered'):
                # a fresh process per measurement; a child that fails or outlives its limit ends the run (nothing more is started)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', op, width, kernel], capture_output=True, text=True,
                                     timeout=CHILD_SECONDS)
                if out.returncode != 0:
                    sys.exit(f'native_ordered_time: {op} {width} {kernel} exited with {out.returncode}\n{out.stdout}\n{out.stderr}')
                r = json.loads(next(l for l in out.stdout.splitlines() if l.startswith('RESULT '))[7:])
                got[kernel] += r['ms']
                got['lists'] += r.get('lists_ms', [])
                err = r.get('against_scatter', err)
        ratio = sorted(got['ordered'])[len(got['ordered']) // 2] / sorted(got['scatter'])[len(got['scatter']) // 2]
        lines.append(f'{LABELS[op]:<46}{width:<7}{summary(got["scatter"]):<36}{summary(got["ordered"]):<36}'
                     f'{(summary(got["lists"]) if got["lists"] else "-"):<36}{ratio:<20.2f}{err:.1e} of the largest gradient')
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
