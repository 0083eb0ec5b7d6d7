"""float64 through the native operator modules: gather forward, furthest point sampling, anchor_query and
initial_anchor_query (boundary B2: T in {float32, float64}, as the reference's AT_DISPATCH_FLOATING_TYPES) against the float64
twins of the CPU oracle, and the layers above them on float64 clouds.

Bars: indices, counts and the float32 gather output bit-equal; anchor_query within 1e-12 of the reference's scale (acos near +-1
is conditioned ~32x on these inputs, the project's other float64 bars are 1e-12 / 1e-13); the initial_anchor_query weights within
1e-13 of their scale (sums of at most 66 correctly rounded terms in index order, on both sides: equality is expected).  Every test prints the figure it measured
before it asserts.  The inputs are built so that a kernel computing in float32 behind a float64 signature misses the bars: the
oracle-only asserts at the head of the tests check exactly that."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import native  # noqa: E402  (checker only)

T = torch.from_numpy


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


# ------------------------------------------------------------------------------------------------
# gather forward: float64 in, float32 out, one round-to-nearest-even conversion per element
# ------------------------------------------------------------------------------------------------
PLANTED = np.array([0.0, -0.0, 1 + 2.0 ** -30, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -40, -(1 + 2.0 ** -23 + 2.0 ** -24)], np.float64)
# what float32 holds after the conversion: +0, -0, down to 1, the tie to even (1), up to 1 + 2^-23, the tie to even upwards in magnitude
PLANTED_F32 = np.array([0.0, -0.0, 1.0, 1.0, 1 + 2.0 ** -23, -(1 + 2.0 ** -22)], np.float32)


def gather_inputs():
    rng = np.random.default_rng(40)
    pts = rng.standard_normal((3, 5, 97))
    pts[:, 2, :6] = PLANTED
    mag = np.abs(pts)
    assert ((mag == 0) | ((mag >= 1e-30) & (mag <= 1e30))).all()      # neither overflow nor float32 subnormals
    idx = rng.integers(0, 97, (3, 211)).astype(np.int32)
    idx[:, :6] = np.arange(6)
    idx[:, 6], idx[:, 7] = 96, 0
    return pts, idx


def test_gather_forward_rounds_once_to_nearest_even(dev):
    import vgtk.cuda.gathering as GA
    pts, idx = gather_inputs()
    ref = native.gather_points_forward(pts, idx)
    np.testing.assert_array_equal(bits(ref[:, 2, :6]), np.broadcast_to(bits(PLANTED_F32), (3, 6)))    # the oracle itself
    got = GA.gather_points_forward(T(pts).to(dev), T(idx).to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 5, 211)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(ref))


def test_group_nd_on_a_float64_cloud(dev):
    import vgtk.pc as pctk
    rng = np.random.default_rng(41)
    pc = rng.standard_normal((2, 3, 64))
    idx = rng.integers(0, 64, (2, 8, 4)).astype(np.int32)
    got = pctk.group_nd(T(pc).to(dev), T(idx).to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 8, 4)
    ref = native.gather_points_forward(pc, idx.reshape(2, 32)).reshape(2, 3, 8, 4)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(ref))


def test_gathering_autograd_hands_back_float64(dev):
    """The float32 gradient of the float32 output goes through gather_points_backward and is then widened.  The scatter-add runs on
    float atomics whose order is not defined, so the gradient values are multiples of 2^-8 below 4: every partial sum is exact in
    float32 and every order gives the same bits, which is what lets the comparison be exact."""
    from vgtk.spconv.functional import Gathering
    pts, idx = gather_inputs()
    rng = np.random.default_rng(42)
    g32 = (rng.integers(-1024, 1025, (3, 5, 211)) / 256.0).astype(np.float32)
    leaf = T(pts).to(dev).requires_grad_(True)
    out = Gathering.apply(leaf, T(idx).to(dev))
    assert out.dtype == torch.float32
    out.backward(T(g32).to(dev))
    assert leaf.grad.dtype == torch.float64 and tuple(leaf.grad.shape) == (3, 5, 97)
    ref = native.gather_points_backward(g32, idx, 97)
    assert ref.dtype == np.float32
    np.testing.assert_array_equal(leaf.grad.cpu().numpy(), ref.astype(np.float64))


# ------------------------------------------------------------------------------------------------
# furthest point sampling
# ------------------------------------------------------------------------------------------------
def fps_grid_clouds(n):
    """Two clouds of n points of the 12^3 grid 0.25 + 0.125 (i,j,k) in a seeded random order, the second with the coordinate rows
    reversed, plus a perturbation in [-1e-10, 1e-10]: in float32 it vanishes (the grid is exact there, half an ulp at 0.25 is 1.5e-8) and
    the many equal distances are decided by the tie rules; in float64 the perturbation decides them.  Point 5 sits at the origin
    and must be skipped."""
    rng = np.random.default_rng(59)
    ijk = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing='ij'), -1).reshape(-1, 3)
    grid = 0.25 + 0.125 * ijk[rng.permutation(12 ** 3)[:n]].astype(np.float64)       # [n,3]
    xyz = np.stack([grid.T, grid.T[::-1]])                                           # [2,3,n]
    xyz = xyz + rng.uniform(-1e-10, 1e-10, xyz.shape)
    xyz[:, :, 5] = 0.0
    return np.ascontiguousarray(xyz)


FPS_SHAPES = [(97, 24), (1500, 64)]      # block 64 with a ragged tail; block 1024 with a strided scan


@pytest.fixture(scope='module')
def fps_refs():
    out = {}
    for n, m in FPS_SHAPES:
        xyz = fps_grid_clouds(n)
        out[(n, m)] = (xyz, native.furthest_point_sampling(xyz, m), native.furthest_point_sampling(xyz.astype(np.float32), m))
    return out


@pytest.mark.parametrize('n,m', FPS_SHAPES)
def test_fps_float64_picks(dev, fps_refs, n, m):
    import vgtk.cuda.grouping as G
    xyz, ref64, ref32 = fps_refs[(n, m)]
    differ = int((ref64 != ref32).sum())
    print(f'fps n={n} m={m}: float64 and float32 oracles differ in {differ} of {ref64.size} picks')
    assert differ * 4 >= ref64.size                           # double arithmetic is observable on these inputs
    assert all(len(set(row)) == m and 5 not in row for row in ref64.tolist())
    got = G.furthest_point_sampling(T(xyz).to(dev), m)
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), ref64)


def test_fps_float64_surface_cloud(dev):
    import synth_clouds
    import vgtk.cuda.grouping as G
    xyz = synth_clouds.laptop_batch(11, 2, 512)[0].astype(np.float64)
    xyz[:, :, 5] = 0.0
    got = G.furthest_point_sampling(T(xyz).to(dev), 128).cpu().numpy()
    np.testing.assert_array_equal(got, native.furthest_point_sampling(xyz, 128))
    one = G.furthest_point_sampling(T(xyz).to(dev), 1)
    assert tuple(one.shape) == (2, 1) and one.dtype == torch.int32 and int(one.abs().sum()) == 0


def test_furthest_sample_on_a_float64_cloud(dev, fps_refs):
    import vgtk.pc as pctk
    xyz, ref64, _ = fps_refs[(97, 24)]
    chosen, pts = pctk.furthest_sample(T(xyz).to(dev), 24, lazy_sample=False)
    np.testing.assert_array_equal(chosen.cpu().numpy(), ref64)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (2, 3, 24)
    np.testing.assert_array_equal(bits(pts.cpu().numpy()), bits(native.gather_points_forward(xyz, ref64)))
    np.testing.assert_array_equal(pctk.furthest_sample_index(T(xyz).to(dev), 24, False).cpu().numpy(), ref64)


# ------------------------------------------------------------------------------------------------
# anchor_query / initial_anchor_query
# ------------------------------------------------------------------------------------------------
def parity_draws():
    """The draws of test_gpu_parity.test_anchor_queries (same generator, same order), kept in float64."""
    rng = np.random.default_rng(6)
    gx = rng.random((2, 3, 9, 8)) - 0.5
    anchors = rng.standard_normal((12, 3))
    anchors /= np.linalg.norm(anchors, axis=1, keepdims=True)
    kp = rng.random((5, 2))
    centers = rng.random((2, 3, 6)) - 0.5
    frag = rng.random((200, 3)) - 0.5
    kpts = (rng.random((4, 7, 3)) - 0.5) * 0.3
    return gx, anchors, kp, centers, frag, kpts


def anchor_query_inputs(case, golden):
    if case == 'small':
        gx, anchors, kp = parity_draws()[:3]
    else:                                                      # 33 * 16 = 528 entries: more than one block of 256, a ragged last one
        rng = np.random.default_rng(7)
        gx = rng.random((1, 3, 33, 16)) - 0.5
        anchors = golden('constants.npz')['anchors'].astype(np.float64)[:, :, 0]      # [60,3], first columns of the rotations
        anchors /= np.linalg.norm(anchors, axis=1, keepdims=True)
        kp = rng.random((24, 2))
    gx[0, :, 1, 3] = 0.0                                       # a zero offset vector: norm = 1e-6, theta = acos(0)
    return np.ascontiguousarray(gx), np.ascontiguousarray(anchors), kp


@pytest.mark.parametrize('case', ['small', 'two_blocks'])
def test_anchor_query_float64(dev, golden, case):
    import vgtk.cuda.grouping as G
    gx, anchors, kp = anchor_query_inputs(case, golden)
    b, _, np_, nn = gx.shape
    ref = native.anchor_query(None, None, gx, anchors, kp, 10)[0]
    ref32 = native.anchor_query(None, None, gx.astype(np.float32), anchors.astype(np.float32), kp.astype(np.float32), 10)[0]
    apart = rel_err(ref32, ref)
    print(f'anchor_query {case}: float32 oracle vs float64 oracle {apart:.3e}')
    assert apart > 1e-9                                        # a kernel that computes in float32 cannot meet the bar below
    z = torch.zeros(b, np_, dtype=torch.int32, device=dev)
    got = G.anchor_query(z, torch.zeros(b, np_, nn, dtype=torch.int32, device=dev), T(gx).to(dev), T(anchors).to(dev), T(kp).to(dev), 10)[0]
    assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape
    err = rel_err(got.cpu().numpy(), ref)
    print(f'anchor_query {case}: max|got - ref| / max|ref| = {err:.3e}')
    assert err <= 1e-12


def initial_anchor_query_inputs():
    return parity_draws()[3:]


def test_initial_anchor_query_float64(dev):
    import vgtk.cuda.grouping as G
    centers, frag, kpts = initial_anchor_query_inputs()
    rw, rc = native.initial_anchor_query(centers, frag, kpts, 0.4, 0.05)
    w, cnt = G.initial_anchor_query(T(centers).to(dev), T(frag).to(dev), T(kpts).to(dev), 0.4, 0.05)
    assert w.dtype == torch.float64 and cnt.dtype == torch.float64 and tuple(w.shape) == rw.shape == tuple(cnt.shape)
    assert rc.max() > 1                                        # (66 on these draws: the sums have up to 66 terms)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rc)
    err = rel_err(w.cpu().numpy(), rw)
    print(f'initial_anchor_query: max count {rc.max():.0f}, max|w - ref| / max|ref| = {err:.3e}, bit-equal: {np.array_equal(w.cpu().numpy(), rw)}')
    assert err <= 1e-13


# ------------------------------------------------------------------------------------------------
# dtype rules; the float32 calls return what they returned
# ------------------------------------------------------------------------------------------------
def test_mixed_and_half_dtypes_raise(dev, golden):
    import vgtk.cuda.grouping as G
    gx, anchors, kp = (T(a).to(dev) for a in anchor_query_inputs('small', golden))
    z, zz = torch.zeros(2, 9, dtype=torch.int32, device=dev), torch.zeros(2, 9, 8, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match='anchor_query'):
        G.anchor_query(z, zz, gx, anchors.float(), kp, 10)
    with pytest.raises(RuntimeError, match='anchor_query'):
        G.anchor_query(z, zz, gx.float(), anchors.float(), kp, 10)
    centers, frag, kpts = (T(a).to(dev) for a in initial_anchor_query_inputs())
    with pytest.raises(RuntimeError, match='initial_anchor_query'):
        G.initial_anchor_query(centers, frag.float(), kpts, 0.4, 0.05)
    with pytest.raises(RuntimeError, match='initial_anchor_query'):
        G.initial_anchor_query(centers.float(), frag.float(), kpts, 0.4, 0.05)
    cloud = torch.rand(1, 3, 32, device=dev)
    for half in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError):
            G.furthest_point_sampling(cloud.to(half), 4)


def test_float32_calls_are_unchanged(dev, golden, fps_refs):
    import vgtk.cuda.gathering as GA
    import vgtk.cuda.grouping as G
    pts, idx = gather_inputs()
    pts = pts.astype(np.float32)
    got = GA.gather_points_forward(T(pts).to(dev), T(idx).to(dev))
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(native.gather_points_forward(pts, idx)))
    xyz, _, ref32 = fps_refs[(97, 24)]                        # (the grid in float32: every pick is a tie-break)
    np.testing.assert_array_equal(G.furthest_point_sampling(T(xyz.astype(np.float32)).to(dev), 24).cpu().numpy(), ref32)
    gx, anchors, kp = (a.astype(np.float32) for a in anchor_query_inputs('small', golden))
    z, zz = torch.zeros(2, 9, dtype=torch.int32, device=dev), torch.zeros(2, 9, 8, dtype=torch.int32, device=dev)
    w = G.anchor_query(z, zz, T(gx).to(dev), T(anchors).to(dev), T(kp).to(dev), 10)[0]
    assert w.dtype == torch.float32
    assert rel_err(w.cpu().numpy(), native.anchor_query(None, None, gx, anchors, kp, 10)[0]) < 1e-5
    centers, frag, kpts = (a.astype(np.float32) for a in initial_anchor_query_inputs())
    w, cnt = G.initial_anchor_query(T(centers).to(dev), T(frag).to(dev), T(kpts).to(dev), 0.4, 0.05)
    rw, rc = native.initial_anchor_query(centers, frag, kpts, 0.4, 0.05)
    assert w.dtype == torch.float32 and cnt.dtype == torch.float32
    np.testing.assert_array_equal(cnt.cpu().numpy(), rc)
    assert rel_err(w.cpu().numpy(), rw) < 1e-5
