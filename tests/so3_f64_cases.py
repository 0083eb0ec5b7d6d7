"""Shared by tests/test_so3_f64_host.py and tests/test_gpu_so3_f64.py: the float64 references of the SO(3) conv layers (oracle/so3_ref.py
run in float64 on the CPU, unchanged), the bars, and the two oracle-only controls every comparison is preceded by.

Bars (the project's float64 bars, tests/test_gpu_native_f64.py): max|got - ref| <= 1e-12 max|ref| for layer outputs and gradients,
1e-13 for inter_w (values in [0, 1]).

Semantics under test (so3conv/functional.py:L1061-1078 in float64): the neighbour coordinates pass through float32 (group_nd returns
float32 for any input), g = R_rel (float(x_n) - x_p) with the subtraction and everything after it in float64.  The inputs are random
float64 numbers, so
  * `as_float32`: the same layer in float32 (a kernel computing in float32 behind a float64 signature), and
  * `exact_neighbours`: the same layer on exactly-float64 neighbour coordinates (a kernel that skips the float32 pass)
both land more than 1e4 x the bar away from the reference: `controls` asserts that on the oracle alone."""
import contextlib
import os

import numpy as np
import torch

from oracle import so3_ref

BAR, BAR_W = 1e-12, 1e-13
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'so3_f64.npz')


def rel(got, ref):
    """max|got - ref| / max|ref| of two tensors (on the CPU, float64)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@contextlib.contextmanager
def exact_neighbours():
    """the oracle with neighbour coordinates gathered at the input's width instead of through float32 (control only)"""
    keep = so3_ref.group_nd

    def group_nd(pc, idx):
        b = idx.shape[0]
        flat = idx.reshape(b, 1, -1).long().expand(b, pc.shape[1], -1)
        return torch.gather(pc, 2, flat).view(b, -1, *idx.shape[1:])

    so3_ref.group_nd = group_nd
    try:
        yield
    finally:
        so3_ref.group_nd = keep


def rand_rot(gen, *shape):
    q = torch.randn(*shape, 4, generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return R.view(*shape, 3, 3)


def inter_reference(xyz, pose, feats, W, gy, anchors, kernels, radius, sigma, nn, permute_modes, stride=1):
    """The inter conv layer by the oracle, in the dtype of its inputs -> dict(out, gfeats, gW, inter_w, ball_idx).  pose None: the
    pose-free layer (inter_so3conv_grouping).  stride > 1: the strided branch with lazy sampling -- the centres are the first
    ceil(p / stride) points passed through float32 (group_nd) and widened back, their poses gathered; then the oracle's own slab function
    (its sampled wrapper keeps the float32 centres, which a float64 matmul refuses)."""
    feats = feats.clone().requires_grad_(True)
    W = W.clone().requires_grad_(True)
    if pose is None:
        idx, inter_w, _, grouped, _ = so3_ref.inter_so3conv_grouping(xyz, feats, nn, anchors, kernels, radius, sigma)
    elif stride == 1:
        res = so3_ref.inter_so3poseconv_grouping_strided(xyz, pose, feats, nn, anchors, kernels, radius, sigma, permute_modes)
        idx, inter_w, grouped = res['ball_idx'], res['inter_w'], res['new_feats']
    else:
        p2 = -(-xyz.shape[2] // stride)
        sample_idx = torch.arange(p2).view(1, -1).expand(xyz.shape[0], -1).int().contiguous()
        q_xyz = so3_ref.group_nd(xyz, sample_idx).to(xyz.dtype)
        q_pose = so3_ref.batched_index_select(pose, 1, sample_idx.long())
        idx, inter_w, _, grouped = so3_ref._poseconv_slab(q_xyz, q_pose, xyz, pose, so3_ref.add_shadow_feature(feats), nn, anchors, kernels,
                                                          radius, sigma, permute_modes, False)
    out = so3_ref.basic_so3conv(W, grouped)
    gF, gW = torch.autograd.grad(out, [feats, W], gy)
    return {'out': out.detach(), 'gfeats': gF, 'gW': gW, 'inter_w': inter_w.detach(), 'ball_idx': idx.int()}


def intra_reference(feats, W, gy, intra_idx):
    feats = feats.clone().requires_grad_(True)
    W = W.clone().requires_grad_(True)
    out = so3_ref.intra_so3conv_layer(feats, W, intra_idx)
    gF, gW = torch.autograd.grad(out, [feats, W], gy)
    return {'out': out.detach(), 'gfeats': gF, 'gW': gW}


def controls(ref, run, what, keys=('out', 'gfeats', 'gW'), neighbours=True):
    """On the oracle alone: `run(cast)` recomputes the reference with every floating input passed through `cast`.  The float32 result and
    (neighbours=True: layers that gather coordinates) the result on exactly-float64 neighbours are more than 1e4 x the bar from `ref`."""
    low = run(lambda t: t.float())
    for k in keys:
        d = rel(low[k], ref[k])
        print(f'{what}: control float32 {k} {d:.3e}')
        assert d > 1e4 * BAR, (what, k, d)
    if neighbours:
        with exact_neighbours():
            exact = run(lambda t: t)
        for k in keys:
            d = rel(exact[k], ref[k])
            print(f'{what}: control exact-float64 neighbours {k} {d:.3e}')
            assert d > 1e4 * BAR, (what, k, d)
        d = float((exact['inter_w'] - ref['inter_w']).abs().max())
        print(f'{what}: control exact-float64 neighbours inter_w {d:.3e}')
        assert d > 1e4 * BAR_W, (what, d)
        assert torch.equal(exact['ball_idx'], ref['ball_idx'])       # (the ball query reads the float64 coordinates either way)


def check(got, ref, what, bar=BAR):
    d = rel(got, ref)
    print(f'{what}: {d:.3e} of scale (bar {bar:.0e})')
    assert d <= bar, (what, d)
    return d


def load_fixture():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


FIXTURE_CASES = ('pm1', 'pm0', 'nopose', 'k20', 'intra')
RADIUS, SIGMA, NNB = 0.3, 0.05, 8


def fixture_case(z, key):
    """-> dict(xyz, pose or None, feats, gy, W, anchors, kernels, permute_modes, want = {out, gfeats, gW at z['points']}, inter_w [2,4,...])"""
    sub = slice(None, None, 3) if key == 'k20' else slice(None)
    case = {'xyz': z['xyz'], 'pose': None if key in ('nopose', 'intra') else z['pose'], 'feats': z['feats'][..., sub].contiguous(),
            'gy': z['gy'].double()[..., sub].contiguous(), 'W': z[f'{key}_W'], 'permute_modes': 1 if key == 'pm1' else 0,
            'want': {'out': z[f'{key}_out'], 'gfeats': z[f'{key}_gfeats'], 'gW': z[f'{key}_gW']}, 'points': z['points'].long()}
    if key != 'intra':
        case.update(anchors=z[f'{key}_anchors'], kernels=z['kernels'])
        case['inter_w'] = torch.cat([z['inter_w_nopose0'][None], z['inter_w_posed'][1:]]) if key == 'nopose' else z['inter_w_posed'][:, :, sub]
    return case


def at_points(res, points):
    """a result dict with out and gfeats cut to the fixture's stored points"""
    return {'out': res['out'][:, :, points], 'gfeats': res['gfeats'][:, :, points], 'gW': res['gW']}
