"""Shared by tests/test_inv_slot_head_wide_host.py and tests/test_gpu_inv_slot_head_wide.py: the grid, the float64 references and bounds and
a float32 emulation of the wide fused BatchNorm + leaky_relu + point-mean kernels (csrc/heads.hip at Q = 64, eap_bn_act_cloud_mean_wide_*), and
tests/golden/inv_slot_head_2d.npz (tests/golden/make_golden_inv_slot_2d.py) unpacked for the package's class.

The cases are those of tests/test_gpu_inv_slot_head.py (_kernel_case: the same generators, the same float32 coefficients widened, the same
search for a seed without a pre-activation within rounding of zero); the chain lengths are counted from the NEW kernels' mapping:

  One wavefront owns a point's anchor row; wave w of the block's 4 takes the points w, w + 4, ..., 4 rows per loop trip into 4 accumulators,
  so an accumulator receives every 16th point: ceil(n / 16) terms.
  forward   the chain of fused multiply-adds (ceil(n / 16)), the 4 accumulators folded as a tree (2), the 4 waves folded through LDS from
            zero in wave order (4), the product with inv_den (1):                                   L_fwd = ceil(n / 16) + 2 + 4 + 1
  reduce    per trip a lane adds its four anchors as a tree (2) to the row's accumulator (ceil(n / 16) such additions), the 4 accumulators
            are folded as a tree (2) and the 64 lanes by 6 shuffle steps (6); the 4 partials are added in float64:
                                                                                                    L_red = ceil(n / 16) + 2 + 2 + 6
  The constant 20 of the bounds pays for the roundings inside one term (the pre-activation, the slope, the weight, inv_den, xhat), as in the
  narrow kernels' test.  Bounds: forward (L_fwd + 20) u inv_den sum_p |w act|; reduce (L_red + 20) u sum |terms|;
  apply 8 u (|scale gg| + |k2| + |xhat k3|); u = 2^-24."""
import numpy as np
import torch

from head_pooling_common import _fma, worst_ratio
from head_pooling_wide_common import _butterfly64
from inv_slot_common import state_of  # noqa: F401  (re-exported)

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
WAVES, ROWS = 4, 4

# 1 quad, 15 quads (the narrow kernels' domain too), 17 quads, the `use_2d` count, one idle lane, none
NA_GRID = (4, 60, 68, 240, 252, 256)
# fewer points than waves; fewer than one trip of a wave; a partial last trip; several trips
SHAPES = ((1, 3, 1), (2, 5, 3), (3, 4, 5), (2, 3, 17), (2, 2, 131))
SLOPES = (0.0, 0.2)
GRID = [(na, shape) for na in NA_GRID for shape in SHAPES]


def L_fwd(n):
    return -(-n // (WAVES * ROWS)) + 2 + WAVES + 1


def L_red(n):
    return -(-n // (WAVES * ROWS)) + 2 + 2 + 6


def kernel_case(b, c, n, na, slope, soft):
    """-> (t: float32 numpy operands, ref: float64 numpy), the first seed from 100 that _kernel_case accepts"""
    from test_gpu_inv_slot_head import _kernel_case
    seed = 100
    while True:
        case = _kernel_case((b, c, n, na), slope, soft, seed)
        if case is not None:
            break
        seed += 1
    t, ref = case
    return {k: v.numpy() for k, v in t.items()}, {k: v.numpy() for k, v in ref.items()}


def bounds(ref, n):
    """{output: (float64 reference, bound per element)}"""
    return {'fwd': (ref['fwd'], (L_fwd(n) + 20) * U * ref['fwd_abs']),
            'reduce g': (ref['sg'], (L_red(n) + 20) * U * ref['sg_abs']),
            'reduce g xhat': (ref['sgx'], (L_red(n) + 20) * U * ref['sgx_abs']),
            'apply, stat_mask': (ref['gx_masked'], 8 * U * ref['gx_abs_masked']),
            'apply, null': (ref['gx_null'], 8 * U * ref['gx_abs_null'])}


def ratios(got, ref, n):
    return {k: worst_ratio(got[k], *rb) for k, rb in bounds(ref, n).items()}


def _by_trip(a, n):
    """[b, c, n, ...] -> [b, c, trips, ROWS, WAVES, ...]: point p = wave + WAVES * row + WAVES * ROWS * trip; points past n are zero"""
    trips = -(-n // (WAVES * ROWS))
    out = np.zeros(a.shape[:2] + (trips * ROWS * WAVES,) + a.shape[3:], a.dtype)
    out[:, :, :n] = a
    return out.reshape(a.shape[:2] + (trips, ROWS, WAVES) + a.shape[3:])


def emulate(t, slope, wave_fold=True):
    """the three kernels in float32 in their own order of operations, products and sums rounded one by one where the compiler may fuse them
    (the longest path): the per-lane chains over every 16th point, the accumulator tree, the wave fold through LDS (forward) or the four
    anchors of a lane, the accumulator tree and the shuffle tree (reduce; the 4 partials then added in float64), and the apply formula.
    wave_fold=False leaves wave 3 out of the forward's fold (a mutation)."""
    x, g = t['x'], t['g']
    b, c, n, na = x.shape
    slope = f32(slope)
    bc = lambda k: t[k].reshape(b, c, 1, 1)
    sc, sh, mu, inv = bc('scale'), bc('shift'), bc('mean'), bc('invstd')
    w = np.broadcast_to(t['w'].reshape(b, 1, n, 1), x.shape)
    d = t['inv_den'].reshape(b, 1, 1)
    pre = _fma(x, np.broadcast_to(sc, x.shape), np.broadcast_to(sh, x.shape))
    act = np.where(pre > 0, pre, pre * slope)
    # forward
    xa, wa = _by_trip(act, n), _by_trip(np.ascontiguousarray(w), n)
    acc = np.zeros((b, c, ROWS, WAVES, na), f32)
    for trip in range(xa.shape[2]):
        acc = _fma(wa[:, :, trip], xa[:, :, trip], acc)
    part = (acc[:, :, 0] + acc[:, :, 1]) + (acc[:, :, 2] + acc[:, :, 3])                     # [b, c, WAVES, na]
    tot = np.zeros((b, c, na), f32)
    for j in range(WAVES if wave_fold else WAVES - 1):
        tot = tot + part[:, :, j]
    out = dict(fwd=tot * d)
    # reduce
    gq = g * d                                                                                # [b, c, na]
    gg = np.where(pre > 0, gq[:, :, None], gq[:, :, None] * slope) * w                        # [b, c, n, na]
    xh = (x - mu) * inv
    quads = lambda a: a.reshape(a.shape[:-1] + (na // 4, 4))
    tree4 = lambda a: (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
    for key, term in (('reduce g', gg), ('reduce g xhat', gg * xh)):
        rows = _by_trip(tree4(quads(term)), n)                                                # [b, c, trips, ROWS, WAVES, nq]
        s = np.zeros((b, c, ROWS, WAVES, na // 4), f32)
        for trip in range(rows.shape[2]):
            s = s + rows[:, :, trip]
        lane = (s[:, :, 0] + s[:, :, 1]) + (s[:, :, 2] + s[:, :, 3])                          # [b, c, WAVES, nq]
        lanes = np.zeros((b, c, WAVES, 64), f32)                                              # an idle lane contributes nothing
        lanes[..., :na // 4] = lane
        out[key] = _butterfly64(lanes).astype(f64).sum(2)
    # apply
    for key, m in (('apply, stat_mask', t['stat_mask'].reshape(b, 1, n, 1)), ('apply, null', np.ones((b, 1, n, 1), f32))):
        inner = _fma(xh, np.broadcast_to(bc('k3'), x.shape), np.broadcast_to(bc('k2'), x.shape))
        out[key] = _fma(np.broadcast_to(-m, x.shape), inner, gg * sc)
    return out


# ---- tests/golden/inv_slot_head_2d.npz ------------------------------------------------------------------------------------------------------

PARAMS_2D = {'dim_in': 4, 'mlp': [16], 'fc': [16], 'k': 16, 'kanchor': 60, 'temperature': 3.0}


def make_head_2d(tag):
    import vgtk.so3conv as sptk
    return sptk.InvOutBlockOursWithMask(PARAMS_2D, norm=1, pooling_method='attention', use_pointnet=True, use_abs_pos=(tag == 'abs'),
                                        return_point_pooling_feature=True)


def tot_anchors():
    """the 240 rotations PointnetSO3ConvOurs keeps for a `use_2d` map, float32 [240,3,3]"""
    return make_head_2d('rel').pointnet.tot_anchors.detach().clone()


def as_torch(t):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in t.items()}
