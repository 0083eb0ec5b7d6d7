"""tools/head_pooling_wide_bounds.py -- what tests/head_pooling_wide_common.py's measured constants come from, and the worst error / bound of
every wide head kernel (csrc/heads.hip at Q = 64) over the grid of tests/test_gpu_head_pooling_wide.py.  Needs the device.
    python tools/head_pooling_wide_bounds.py [--out profiles/head_pooling_wide_bounds.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'equi-articulated-pose_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np
import torch

import head_pooling_wide_common as W
from vgtk import _hip

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'head_pooling_wide_bounds.txt'))
args = ap.parse_args()
dev = torch.device('cuda:0')
f64 = np.float64
to = lambda a: torch.from_numpy(a).to(dev)
LOGITS = {'randn_T1': 'randn', 'randn_T3': 'randn', 'wide_T3': '40 randn', 'equal_T3': 'equal within a point', 'neginf_T3': 'randn, one -inf a point'}


def rel_normal(got, ref):
    """largest relative error over the elements of at least 2^-126"""
    keep = ref >= W.TINY
    return float((np.abs(got.astype(f64)[keep] - ref[keep]) / ref[keep]).max())


def attn_case(c, n, na, family):
    t = W.attn_inputs(c, n, na, family)
    x, l, g, T = to(t['x']), to(t['logits']), to(t['g']), float(t['T'])
    out, conf = torch.empty(W.B, c, n, device=dev), torch.empty(W.B, n, na, device=dev)
    dx, dl = torch.empty_like(x), torch.empty_like(l)
    _hip.call('eap_anchor_attn_pool_wide_fwd_f32', x, W.B, c, n, na, T, x, l, out, conf)
    _hip.call('eap_anchor_attn_pool_wide_bwd_f32', x, W.B, c, n, na, T, x, l, g, dx, dl)
    soft = torch.softmax(l * T, -1)
    return t, dict(out=out.cpu().numpy(), conf=conf.cpu().numpy(), dx=dx.cpu().numpy(), dlogits=dl.cpu().numpy()), soft.cpu().numpy()


# pass 1: the measured term.  pass 2: the ratios under 4 x torch's figure of the same family
torch_rel = {f: 0.0 for f in W.ATTN_FAMILIES}
kern_rel = dict(torch_rel)
cases = {}
for na in W.NA_GRID:
    for n in W.N_GRID:
        for c in W.C_GRID:
            for family in W.ATTN_FAMILIES:
                t, got, soft = attn_case(c, n, na, family)
                ref = W.attn_reference(t, exp_rel=0.0)['conf'][0]
                torch_rel[family] = max(torch_rel[family], rel_normal(soft, ref))
                kern_rel[family] = max(kern_rel[family], rel_normal(got['conf'], ref))
                cases[(c, n, na, family)] = (t, got)
ratio = {k: 0.0 for k in ('out', 'conf', 'dx', 'dlogits')}
conf_normal = {f: 0.0 for f in W.ATTN_FAMILIES}
derived_excess = 0.0
for (c, n, na, family), (t, got) in cases.items():
    refs = W.attn_reference(t, exp_rel=4.0 * torch_rel[family])
    for k, (ref, bound) in refs.items():
        ratio[k] = max(ratio[k], W.worst_ratio(got[k], ref, bound))
    keep = refs['conf'][0] >= W.TINY
    conf_normal[family] = max(conf_normal[family], W.worst_ratio(got['conf'][keep], refs['conf'][0][keep], refs['conf'][1][keep]))
    ref0, b0 = W.attn_reference(t, exp_rel=0.0)['conf']
    derived_excess = max(derived_excess, W.worst_ratio(got['conf'][keep], ref0[keep], b0[keep]))

slot = {'fwd': 0.0, 'bwd': 0.0}
for na in W.NA_GRID:
    for n in W.N_GRID:
        for c in W.C_GRID:
            for ns in W.NS_GRID:
                for family in W.SLOT_FAMILIES:
                    t = W.slot_inputs(c, n, na, ns, family)
                    x, m, d, g = (to(t[k]) for k in ('x', 'mask', 'inv_den', 'g'))
                    fwd, bwd = torch.empty(W.B, ns, c, na, device=dev), torch.empty(W.B, c, n, na, device=dev)
                    _hip.call('eap_slot_masked_mean_wide_fwd_f32', x, W.B, ns, c, n, na, x, m, d, fwd)
                    _hip.call('eap_slot_masked_mean_wide_bwd_f32', g, W.B, ns, c, n, na, g, m, d, bwd)
                    refs = W.slot_reference(t)
                    slot['fwd'] = max(slot['fwd'], W.worst_ratio(fwd.cpu().numpy(), *refs['fwd']))
                    slot['bwd'] = max(slot['bwd'], W.worst_ratio(bwd.cpu().numpy(), *refs['bwd']))

exact, total = 0, 0
for na in W.NA_GRID:
    for n in W.N_GRID:
        for c in W.C_GRID:
            for family in W.MAX_FAMILIES:
                t = W.max_inputs(c, n, na, family)
                x, m, g = to(t['x']), to(t['mask']), to(t['g'])
                out, arg = torch.empty(W.B, c, na, device=dev), torch.empty(W.B, c, na, dtype=torch.int32, device=dev)
                dx = torch.empty(W.B, c, n, na, device=dev)
                _hip.call('eap_masked_max_wide_fwd_f32', x, W.B, c, n, na, x, m, out, arg)
                _hip.call('eap_masked_max_wide_bwd_f32', g, W.B, c, n, na, g, arg, m, dx)
                ref = W.max_reference(t)
                total += 1
                exact += int(W.same_values(out.cpu().numpy(), ref['out']) and np.array_equal(arg.cpu().numpy(), ref['arg'])
                             and W.same_values(dx.cpu().numpy(), ref['dx']))

lines = [
    'Wide head pooling kernels (csrc/heads.hip at Q = 64: eap_anchor_attn_pool_wide_*, eap_slot_masked_mean_wide_*, eap_masked_max_wide_*) against',
    "float64 on an MI355X: what tests/head_pooling_wide_common.py's constants were measured from, and the worst error / bound per kernel.",
    f'Written by tools/head_pooling_wide_bounds.py.  Grid: b = {W.B}, c in {list(W.C_GRID)}, na in {list(W.NA_GRID)}, n in {list(W.N_GRID)}, slot mean also ns in {list(W.NS_GRID)}.',
    '',
    '1. The exponential term of the confidence bound',
    '   Largest relative error of a softmax confidence against float64 over every attention input of the grid, elements of at least 2^-126:',
    "   float32 torch.softmax(logits * T, -1) on the device (the reference's formulation) and the kernel's conf output.",
    '',
    '   family      logits                    T   torch.softmax   kernel conf',
]
for f in W.ATTN_FAMILIES:
    lines.append(f"   {f:<11} {LOGITS[f]:<25} {1 if f == 'randn_T1' else 3}   {torch_rel[f]:.2e}        {kern_rel[f]:.2e}")
lines += [
    '',
    "   The test allows the kernel's exponential 4 x the torch figure of the same family (SOFTMAX_REL_MEASURED, EXP_REL) on top of the derived",
    '   terms u (|T l| + |z|) for the argument, |z| u for the scaling by log2 e and 11 u for the sum, the reciprocal and the product.',
    f"   With the measured term set to 0 the kernel's largest error / bound over the elements of at least 2^-126 is {derived_excess:.3f}.",
    '',
    '2. Worst error / bound per kernel (every element has its own bound; the maximum over the grid and over all input families),',
    '   the measured term at 4 x the torch figures of this run',
    '',
    '   kernel                           output     worst ratio',
    f"   anchor_attn_pool_wide fwd        out        {ratio['out']:.3f}   k = 1 + 3 + 6",
    f"   anchor_attn_pool_wide fwd        conf       {ratio['conf']:.3f}   (over the elements of at least 2^-126, by family: "
    + ', '.join(f'{f} {v:.3f}' for f, v in conf_normal.items()) + ')',
    f"   anchor_attn_pool_wide bwd        dx         {ratio['dx']:.3f}",
    f"   anchor_attn_pool_wide bwd        dlogits    {ratio['dlogits']:.3f}",
    f"   slot_masked_mean_wide fwd        out        {slot['fwd']:.3f}   k = ceil(n / 4) + 4 + 1",
    f"   slot_masked_mean_wide bwd        dx         {slot['bwd']:.3f}   k = 1 + ns",
    f'   masked_max_wide fwd / bwd        out, arg, dx   exact in {exact} of {total} cases ({len(W.MAX_FAMILIES)} input families), NaN and tie cases included',
    '',
    '   Below 2^-126 the bound of a confidence is the absolute 2^-126 (the device may flush), so ratios close to 1 of conf, dx and dlogits in',
    '   the wide family are ref / 2^-126 < 1 by construction.',
]
text = '\n'.join(lines) + '\n'
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, 'w').write(text)
print(text)
print('SOFTMAX_REL_MEASURED =', {f: float(f'{v:.3g}') for f, v in torch_rel.items()})
print('KERNEL_CONF_REL_MEASURED =', {f: float(f'{v:.3g}') for f, v in kern_rel.items()})
