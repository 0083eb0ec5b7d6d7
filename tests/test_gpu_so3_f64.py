"""GPU: the float64 regime of the SO(3) conv layers (csrc/so3_f64.hip; vgtk.so3conv.functional _GroupContractF64 around _F64Args /
_IntraGrouping, _ContractF64) against exact integer products, the reference-made fixture, the CPU oracle in float64, finite differences, itself (run to
run, slab size to slab size) and as the checker of the float32 layer.

Bars (tests/so3_f64_cases.py): 1e-12 of the reference's scale for outputs and gradients, 1e-13 for inter_w and for the random GEMMs (sums of
at most 660 products: 660 x 2^-53 = 7e-14 of the sum of magnitudes is the worst case of either side).  Every test prints the figure it
measured before it asserts; every comparison with the oracle is preceded by the two oracle-only controls (float32 computation, exactly-
float64 neighbour coordinates: both more than 1e4 x the bar away), so a kernel that computes in float32 behind a float64 signature, or that
skips the float32 pass of the neighbour coordinates, fails here."""
import pytest
import torch

import so3_f64_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------
# the GEMM on v_mfma_f64_16x16x4_f64: padded, offset and strided operands, NaN in all padding, canaries around the output
# ------------------------------------------------------------------------------------------------
GUARD = 64
CANARY = 0x7FF8BEEFBEEFBEEF                              # a quiet NaN with a recognisable payload
MS, KS, NS = (1, 3, 17, 48), (24, 50, 72), (60, 420, 660)


class Embedded:
    """a [nb, rows, cols] float64 stack inside a larger buffer: row pitch cols + pad, item stride rows * pitch + gap, first element `base`
    doubles past a guard band; everything outside the logical elements is NaN (inputs) or the canary (outputs)"""

    def __init__(self, values, pad, gap, base, device, output=False):
        nb, rows, cols = values.shape
        self.ld, self.stride, self.off = cols + pad, rows * (cols + pad) + gap, GUARD + base
        self.shape = (nb, rows, cols)
        size = self.off + (nb - 1) * self.stride + rows * self.ld + GUARD
        buf = torch.full((size,), CANARY, dtype=torch.int64).view(torch.float64) if output else torch.full((size,), float('nan'), dtype=torch.float64)
        if not output:
            torch.as_strided(buf, self.shape, (self.stride, self.ld, 1), self.off).copy_(values)
        self.buf = buf.to(device)

    def view(self):
        return torch.as_strided(self.buf, self.shape, (self.stride, self.ld, 1), self.off)

    def untouched_outside(self):
        rest = self.buf.view(torch.int64).clone()
        torch.as_strided(rest, self.shape, (self.stride, self.ld, 1), self.off).fill_(CANARY)
        return bool((rest == CANARY).all())


def gemm_operands(M, K, N, integer, seed):
    """W [M,K], X [2,K,N], gY [2,M,N] in float64: small non-zero integers (every product and sum exact) or random numbers"""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * M + 7 * K + N)
    if integer:
        draw = lambda *s: (torch.randint(1, 5, s, generator=gen) * (torch.randint(0, 2, s, generator=gen) * 2 - 1)).double()
    else:
        draw = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    return draw(1, M, K), draw(2, K, N), draw(2, M, N)


def run_forms(W, X, gY, dev, embedded):
    """the three forms through vgtk._hip.matmul / matmul_reduce -> (Y [2,M,N], dX [2,K,N], dW [M,K], dW in two accumulated slabs), and
    whether every output buffer is untouched outside its logical elements"""
    from vgtk import _hip
    (_, M, K), N = W.shape, X.shape[2]
    emb = (lambda v, pad, gap, base, output=False: Embedded(v, pad, gap, base, dev, output)) if embedded else \
        (lambda v, pad, gap, base, output=False: Embedded(v, 0, 0, 0, dev, output))
    w, x, gy = emb(W, 3, 0, 5), emb(X, 2, 9, 1), emb(gY, 5, 7, 3)
    y, dx = emb(torch.zeros(2, M, N), 1, 11, 7, True), emb(torch.zeros(2, K, N), 4, 3, 2, True)
    dw, dw2 = emb(torch.zeros(1, M, K), 6, 0, 9, True), emb(torch.zeros(1, M, K), 6, 0, 9, True)
    _hip.matmul(w.view()[0], x.view(), y.view())                                        # Y_z = W X_z
    _hip.matmul(w.view()[0].t(), gy.view(), dx.view())                                  # dX_z = W^T gY_z
    _hip.matmul_reduce(gy.view(), x.view().transpose(1, 2), dw.view()[0])               # dW = sum_z gY_z X_z^T
    _hip.matmul_reduce(gy.view()[:1], x.view()[:1].transpose(1, 2), dw2.view()[0])
    _hip.matmul_reduce(gy.view()[1:], x.view()[1:].transpose(1, 2), dw2.view()[0], accumulate=True)
    torch.cuda.synchronize()
    clean = all(o.untouched_outside() for o in (y, dx, dw, dw2))
    return y.view().cpu(), dx.view().cpu(), dw.view()[0].cpu(), dw2.view()[0].cpu(), clean


@pytest.mark.parametrize('M', MS)
def test_gemm_integer_exact(dev, M):
    """Small integers in float64: all three forms equal the int64 result bit for bit -- a wrong accumulator map (the f32 row formula on the
    f64 MFMA puts 3 of every 4 results in the wrong row) cannot pass."""
    for K in KS:
        for N in NS:
            W, X, gY = gemm_operands(M, K, N, True, 1)
            Wi, Xi, Gi = W.long(), X.long(), gY.long()
            want = (torch.matmul(Wi, Xi), torch.matmul(Wi.transpose(1, 2), Gi), torch.matmul(Gi, Xi.transpose(1, 2)).sum(0))
            y, dx, dw, dw2, clean = run_forms(W, X, gY, dev, True)
            wrong = [int((g != w.double()).sum()) for g, w in zip((y, dx, dw, dw2), want + (want[2],))]
            print(f'M={M} K={K} N={N}: elements off the int64 result (Y, dX, dW, dW in slabs) {wrong}, outputs clean outside [M,N]: {clean}')
            assert wrong == [0, 0, 0, 0] and clean


@pytest.mark.parametrize('M', MS)
def test_gemm_random_against_torch_float64(dev, M):
    for K in KS:
        for N in NS:
            W, X, gY = gemm_operands(M, K, N, False, 2)
            want = (torch.matmul(W, X), torch.matmul(W.transpose(1, 2), gY), torch.matmul(gY, X.transpose(1, 2)).sum(0))
            y, dx, dw, dw2, clean = run_forms(W, X, gY, dev, False)
            errs = [S.rel(g, w) for g, w in zip((y, dx, dw), want)]
            print(f'M={M} K={K} N={N}: Y {errs[0]:.2e} dX {errs[1]:.2e} dW {errs[2]:.2e} of scale (bar {S.BAR_W:.0e})')
            assert max(errs) <= S.BAR_W and torch.equal(dw, dw2) and clean


# ------------------------------------------------------------------------------------------------
# the layers
# ------------------------------------------------------------------------------------------------
def run_layer(conv, cloud, feats, gy, dev):
    """a module on the device, forward + backward -> dict(out, gfeats, gW, inter_w, ball_idx, logs)"""
    import vgtk.so3conv.functional as L
    feats = feats.to(dev).requires_grad_(True)
    L.FORWARD_LOG, L.BACKWARD_LOG = [], []
    try:
        res = conv(cloud(feats))
        intra = not isinstance(res, tuple)
        y = res.feats if intra else res[3].feats
        gF, gW = torch.autograd.grad(y, [feats, conv.basic_conv.W], gy.to(dev))
        torch.cuda.synchronize()
        logs = (L.FORWARD_LOG, L.BACKWARD_LOG)
    finally:
        L.FORWARD_LOG = L.BACKWARD_LOG = None
    out = {'out': y.detach(), 'gfeats': gF, 'gW': gW, 'logs': logs}
    if not intra:
        out['handle'] = res[1]
        out['inter_idx'] = res[0]
    return out


def place(conv, W, anchors=None, kernels=None, dev=None):
    conv = conv.double().to(dev)
    with torch.no_grad():
        conv.basic_conv.W.copy_(W)
        if anchors is not None:
            assert S.rel(conv.anchors, anchors) < 1e-6          # the package's own tables are the reference's to float32 rounding
            conv.anchors.copy_(anchors)
            conv.kernels.copy_(kernels)
    return conv


@pytest.fixture(scope='module')
def fixture():
    return S.load_fixture()


@pytest.mark.parametrize('key', S.FIXTURE_CASES)
def test_fixture_through_the_public_modules(dev, fixture, key):
    import vgtk.cuda.grouping as G
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    c = S.fixture_case(fixture, key)
    xyz = c['xyz'].to(dev)
    C, O = 3, 5
    if key == 'intra':
        conv = place(sptk.IntraSO3Conv(C, O), c['W'], dev=dev)
        assert torch.equal(conv.intra_idx.cpu(), fixture['intra_idx'])
        cloud = lambda f: zptk.SphericalPointCloud(xyz, f, None)
    elif key == 'nopose':
        conv = place(sptk.InterSO3Conv(C, O, 1, 1, S.RADIUS, S.SIGMA, S.NNB), c['W'], c['anchors'], c['kernels'], dev)
        cloud = lambda f: zptk.SphericalPointCloud(xyz, f, None)
    else:
        conv = place(sptk.InterSO3PoseConv(C, O, 1, 1, S.RADIUS, S.SIGMA, S.NNB, kanchor=20 if key == 'k20' else 60,
                                           permute_modes=c['permute_modes']), c['W'], c['anchors'], c['kernels'], dev)
        pose = c['pose'].to(dev)
        cloud = lambda f: zptk.SphericalPointCloudPose(xyz, f, None, pose)
    got = run_layer(conv, cloud, c['feats'], c['gy'], dev)
    assert got['out'].dtype == torch.float64 and got['gfeats'].dtype == torch.float64 and got['gW'].dtype == torch.float64
    cut = S.at_points(got, c['points'].to(dev))
    for k in ('out', 'gfeats', 'gW'):
        S.check(cut[k], c['want'][k], f'{key} {k}')
    if key != 'intra':
        idx = G.ball_query(xyz, xyz, S.RADIUS, S.NNB)
        assert torch.equal(idx.cpu(), fixture['ball_idx'])
        if got['inter_idx'] is not None:
            assert torch.equal(got['inter_idx'].cpu().int(), fixture['ball_idx'])
        w = got['handle'].materialize()
        assert w.dtype == torch.float64 and tuple(w.shape) == tuple(got['handle'].shape)
        d = float((w[:, :4].cpu() - c['inter_w']).abs().max())
        print(f'{key} inter_w: {d:.3e} (bar {S.BAR_W:.0e})')
        assert d <= S.BAR_W
        fwd, bwd = got['logs']
        assert [e['regime'] for e in fwd] == ['float64'] and [e['regime'] for e in bwd] == ['float64'], (fwd, bwd)


# (P, nn, radius): a radius small enough that some lists are repeat-padded.  P = 130 with nn = 64 is left out: the oracle's 60 x 60 trace
# tensor is 6.5 GB there and its three runs (reference + two controls) take 8 s on the CPU; several blocks per cloud and 64-entry lists are
# each in the cases that stay.
OFF_TILE = [(1, 1, 0.3), (1, 5, 0.3), (1, 64, 0.3), (37, 1, 0.3), (37, 5, 0.3), (37, 64, 0.3), (130, 1, 0.2), (130, 5, 0.2)]


def off_tile_inputs(P, nn, stride=1, seed=5):
    gen = torch.Generator().manual_seed(seed * 1000 + 10 * P + nn)
    B, C, O = 3, 2, 3
    xyz = torch.rand(B, 3, P, generator=gen, dtype=torch.float64)
    pose = torch.eye(4, dtype=torch.float64).repeat(B, P, 1, 1)
    pose[0, :, :3, :3] = S.rand_rot(gen, P)                       # cloud 1 keeps identity poses beside the per-point ones: the per-cloud flag
    pose[2, :, :3, :3] = S.rand_rot(gen, P)
    feats = torch.randn(B, C, P, 60, generator=gen, dtype=torch.float64)
    W = torch.randn(O, C * 24, generator=gen, dtype=torch.float64)
    gy = torch.randn(B, O, -(-P // stride), 60, generator=gen, dtype=torch.float64)
    return xyz, pose, feats, W, gy


def compare_with_oracle(dev, what, conv, xyz, pose, feats, W, gy, radius, nn, permute_modes, stride=1):
    import vgtk.spconv as zptk
    anchors, kernels = conv.anchors.detach().cpu(), conv.kernels.detach().cpu()
    run = lambda cast: S.inter_reference(cast(xyz), None if pose is None else cast(pose), cast(feats), cast(W), cast(gy), cast(anchors),
                                         cast(kernels), radius, S.SIGMA, nn, permute_modes, stride)
    ref = run(lambda t: t)
    S.controls(ref, run, what)
    x, ps = xyz.to(dev), None if pose is None else pose.to(dev)
    cloud = (lambda f: zptk.SphericalPointCloud(x, f, None)) if pose is None else (lambda f: zptk.SphericalPointCloudPose(x, f, None, ps))
    got = run_layer(conv, cloud, feats, gy, dev)
    for k in ('out', 'gfeats', 'gW'):
        S.check(got[k], ref[k], f'{what} {k}')
    d = float((got['handle'].materialize().cpu() - ref['inter_w']).abs().max())
    print(f'{what} inter_w: {d:.3e} (bar {S.BAR_W:.0e})')
    assert d <= S.BAR_W
    return ref, got


@pytest.mark.parametrize('P,nn,radius', OFF_TILE)
def test_inter_conv_against_the_oracle_off_tile(dev, P, nn, radius):
    import vgtk.cuda.grouping as G
    import vgtk.so3conv as sptk
    xyz, pose, feats, W, gy = off_tile_inputs(P, nn)
    conv = place(sptk.InterSO3PoseConv(2, 3, 1, 1, radius, S.SIGMA, nn, kanchor=60, permute_modes=1), W, dev=dev)
    ref, _ = compare_with_oracle(dev, f'P={P} nn={nn}', conv, xyz, pose, feats, W, gy, radius, nn, 1)
    idx = ref['ball_idx']
    assert torch.equal(G.ball_query(xyz.to(dev), xyz.to(dev), radius, nn).cpu(), idx)
    if nn > 1:
        padded = float((idx[:, :, 1:] == idx[:, :, :1]).any(-1).float().mean())
        print(f'P={P} nn={nn}: {padded:.2f} of the lists are repeat-padded')
        assert padded > 0


def test_strided_branch_against_the_oracle(dev):
    """stride 2, lazy_sample: the centres are the first ceil(p / 2) points, passed through float32 as group_nd returns them and widened
    back; the output cloud carries them in float64."""
    import vgtk.so3conv as sptk
    P, nn, radius = 37, 5, 0.3
    xyz, pose, feats, W, gy = off_tile_inputs(P, nn, stride=2)
    conv = place(sptk.InterSO3PoseConv(2, 3, 1, 2, radius, S.SIGMA, nn, lazy_sample=True, kanchor=60, permute_modes=1), W, dev=dev)
    compare_with_oracle(dev, 'stride 2', conv, xyz, pose, feats, W, gy, radius, nn, 1, stride=2)


def test_pose_free_and_20_anchor_layers_against_the_oracle(dev):
    import vgtk.so3conv as sptk
    P, nn, radius = 37, 5, 0.3
    xyz, pose, feats, W, gy = off_tile_inputs(P, nn, seed=6)
    conv = place(sptk.InterSO3Conv(2, 3, 1, 1, radius, S.SIGMA, nn), W, dev=dev)
    compare_with_oracle(dev, 'pose-free', conv, xyz, None, feats, W, gy, radius, nn, 0)
    one = pose.clone()
    one[:] = pose[:, :1]                                          # one rotation per cloud: the 20-anchor set stays unpermuted
    conv = place(sptk.InterSO3PoseConv(2, 3, 1, 1, radius, S.SIGMA, nn, kanchor=20, permute_modes=1), W, dev=dev)
    compare_with_oracle(dev, 'kanchor 20, one rotation per cloud', conv, xyz, one, feats[..., ::3].contiguous(), W, gy[..., ::3].contiguous(),
                        radius, nn, 1)


def test_intra_conv_against_the_oracle(dev):
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    import vgtk.spconv as zptk
    gen = torch.Generator().manual_seed(77)
    B, P, C, O = 3, 37, 5, 7
    feats = torch.randn(B, C, P, 60, generator=gen, dtype=torch.float64)
    W = torch.randn(O, C * 12, generator=gen, dtype=torch.float64)
    gy = torch.randn(B, O, P, 60, generator=gen, dtype=torch.float64)
    conv = place(sptk.IntraSO3Conv(C, O), W, dev=dev)
    idx = conv.intra_idx.cpu()
    run = lambda cast: S.intra_reference(cast(feats), cast(W), cast(gy), idx)
    ref = run(lambda t: t)
    S.controls(ref, run, 'intra', neighbours=False)
    xyz = torch.zeros(B, 3, P, dtype=torch.float64, device=dev)
    got = run_layer(conv, lambda f: zptk.SphericalPointCloud(xyz, f, None), feats, gy, dev)
    for k in ('out', 'gfeats', 'gW'):
        S.check(got[k], ref[k], f'intra {k}')
    # the functional grouping API and BasicSO3Conv: the same layer in two nodes
    f = feats.to(dev).requires_grad_(True)
    y = conv.basic_conv(L.intra_so3conv_grouping(conv.intra_idx, f))
    gF, gW = torch.autograd.grad(y, [f, conv.basic_conv.W], gy.to(dev))
    for k, v in (('out', y), ('gfeats', gF), ('gW', gW)):
        S.check(v, ref[k], f'intra, grouping + contraction {k}')


def test_functional_grouping_api_against_the_oracle(dev):
    """inter_so3poseconv_grouping_strided, inter_so3conv_grouping (fresh and with the cached handle) and inter_so3conv_grouping_anchor"""
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    from oracle import so3_ref
    P, nn, radius = 37, 5, 0.3
    xyz, pose, feats, W, _ = off_tile_inputs(P, nn, seed=8)
    conv = sptk.InterSO3PoseConv(2, 3, 1, 1, radius, S.SIGMA, nn, kanchor=60, permute_modes=1).double().to(dev)
    A, Kp = conv.anchors.cpu(), conv.kernels.cpu()
    ref = so3_ref.inter_so3poseconv_grouping_strided(xyz, pose, feats, nn, A, Kp, radius, S.SIGMA, 1)
    gen = torch.Generator().manual_seed(9)
    gX = torch.randn(ref['new_feats'].shape, generator=gen, dtype=torch.float64)
    f0 = feats.clone().requires_grad_(True)
    want_g, = torch.autograd.grad(so3_ref.inter_so3poseconv_grouping_strided(xyz, pose, f0, nn, A, Kp, radius, S.SIGMA, 1)['new_feats'], f0, gX)
    f = feats.to(dev).requires_grad_(True)
    _, w, _, new_feats, _, _ = L.inter_so3poseconv_grouping_strided(xyz.to(dev), pose.to(dev), f, 1, nn, conv.anchors, conv.kernels, radius,
                                                                    S.SIGMA, permute_modes=1)
    S.check(new_feats, ref['new_feats'], 'pose grouping X')
    S.check(torch.autograd.grad(new_feats, f, gX.to(dev))[0], want_g, 'pose grouping dF')
    d = float((w.materialize().cpu() - ref['inter_w']).abs().max())
    print(f'pose grouping inter_w {d:.3e}')
    assert d <= S.BAR_W
    idx0, w0, _, grouped0, _ = so3_ref.inter_so3conv_grouping(xyz, feats, nn, A, Kp, radius, S.SIGMA)
    idx1, w1, _, grouped1, _ = L.inter_so3conv_grouping(xyz.to(dev), feats.to(dev), 1, nn, conv.anchors, conv.kernels, radius, S.SIGMA)
    assert torch.equal(idx1.cpu(), idx0.int())
    S.check(grouped1, grouped0, 'pose-free grouping X')
    again = L.inter_so3conv_grouping(xyz.to(dev), feats.to(dev), 1, nn, conv.anchors, conv.kernels, radius, S.SIGMA, inter_idx=idx1, inter_w=w1)[3]
    assert torch.equal(again, grouped1)                            # the cached handle: the same kernel on the same numbers
    g = so3_ref.ball_query(xyz, xyz, radius, nn)[1] - xyz.unsqueeze(3)
    wa = L.inter_so3conv_grouping_anchor(g.to(dev), conv.anchors, conv.kernels, S.SIGMA)
    d = float((wa.cpu() - w0).abs().max())
    print(f'inter_so3conv_grouping_anchor {d:.3e}')
    assert d <= S.BAR_W


# ------------------------------------------------------------------------------------------------
# the nodes against finite differences, against themselves
# ------------------------------------------------------------------------------------------------
def small_inter_node(dev):
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    gen = torch.Generator().manual_seed(11)
    P, nn = 6, 4
    conv = sptk.InterSO3PoseConv(2, 3, 1, 1, 0.6, S.SIGMA, nn, kanchor=60, permute_modes=1).double().to(dev)
    xyz = torch.rand(1, 3, P, generator=gen, dtype=torch.float64).to(dev)
    pose = torch.eye(4, dtype=torch.float64).repeat(1, P, 1, 1)
    pose[0, :, :3, :3] = S.rand_rot(gen, P)
    args = L._neighbourhood_f64(xyz, pose.to(dev), nn, conv.anchors, conv.kernels, 0.6, S.SIGMA, True, None, None)
    feats = torch.randn(1, 2, P, 60, generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    W = torch.randn(3, 48, generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    return args, feats, W


def test_gradcheck_inter_node(dev):
    import vgtk.so3conv.functional as L
    args, feats, W = small_inter_node(dev)
    assert args.mult is not None and len(torch.unique(args.r)) > 1        # the poses really permute the anchors
    assert torch.autograd.gradcheck(lambda f, w: L._GroupContractF64.apply(f, w, args), (feats, W))


def test_gradcheck_intra_node(dev):
    import vgtk.so3conv.functional as L
    gen = torch.Generator().manual_seed(12)
    feats = torch.randn(1, 2, 3, 60, generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    W = torch.randn(3, 24, generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    idx = torch.from_numpy(L.get_intra_idx()).to(torch.int32).to(dev).contiguous()
    assert torch.autograd.gradcheck(lambda f, w: L._GroupContractF64.apply(f, w, L._IntraGrouping(idx, 'f64')), (feats, W))


def layer_pair(dev):
    """an inter and an intra layer at B = 3 with their inputs on the device"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    P, nn, radius = 37, 5, 0.3
    xyz, pose, feats, W, gy = off_tile_inputs(P, nn, seed=13)
    inter = place(sptk.InterSO3PoseConv(2, 3, 1, 1, radius, S.SIGMA, nn, kanchor=60, permute_modes=1), W, dev=dev)
    gen = torch.Generator().manual_seed(14)
    intra = place(sptk.IntraSO3Conv(2, 3), torch.randn(3, 24, generator=gen, dtype=torch.float64), dev=dev)
    x, ps = xyz.to(dev), pose.to(dev)
    return ((inter, lambda f: zptk.SphericalPointCloudPose(x, f, None, ps)), (intra, lambda f: zptk.SphericalPointCloud(x, f, None))), feats, gy


def test_backward_is_reproducible(dev):
    layers, feats, gy = layer_pair(dev)
    for conv, cloud in layers:
        a, b = run_layer(conv, cloud, feats, gy, dev), run_layer(conv, cloud, feats, gy, dev)
        same = {k: torch.equal(a[k], b[k]) for k in ('out', 'gfeats', 'gW')}
        print(type(conv).__name__, 'bit-identical run to run:', same)
        assert all(same.values())


def test_results_do_not_depend_on_the_slab_size(dev, monkeypatch):
    import vgtk.so3conv.functional as L
    layers, feats, gy = layer_pair(dev)
    for conv, cloud in layers:
        ks = conv.basic_conv.W.shape[1] // feats.shape[1]
        one_cloud = 8 * feats.shape[1] * ks * feats.shape[2] * 60
        monkeypatch.setattr(L, 'F64_X_BYTES_MAX', 1 << 62)
        assert len(L._f64_slabs(3, one_cloud)) == 1
        whole = run_layer(conv, cloud, feats, gy, dev)
        monkeypatch.setattr(L, 'F64_X_BYTES_MAX', one_cloud)
        assert len(L._f64_slabs(3, one_cloud)) == 3
        slabs = run_layer(conv, cloud, feats, gy, dev)
        same = {k: torch.equal(whole[k], slabs[k]) for k in ('out', 'gfeats', 'gW')}
        print(type(conv).__name__, 'one slab against one cloud per slab, bit-identical:', same)
        assert all(same.values())


def test_float64_layer_checks_the_float32_layer(dev):
    """The checker use: the float32 layer in its default regime against the float64 layer on the same inputs widened (the float32 pass of
    the neighbour coordinates is then a no-op).  Bars of tests/test_gpu_dense_golden.py: out and dF 1e-5, dW 2e-5 of scale."""
    import copy
    import synth_clouds
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    xyz, _, pose = synth_clouds.laptop_batch(0, 2, 256)
    xyz, pose = torch.from_numpy(xyz).to(dev), torch.from_numpy(pose).to(dev)
    torch.manual_seed(2913)
    conv32 = sptk.InterSO3PoseConv(32, 64, 1, 1, 0.16, 0.0128, 32, kanchor=60, permute_modes=1).to(dev)
    conv64 = copy.deepcopy(conv32).double()
    gen = torch.Generator().manual_seed(15)
    feats = torch.randn(2, 32, 256, 60, generator=gen)
    gy = torch.randn(2, 64, 256, 60, generator=gen)
    low = run_layer(conv32, lambda f: zptk.SphericalPointCloudPose(xyz, f, None, pose), feats, gy, dev)
    ref = run_layer(conv64, lambda f: zptk.SphericalPointCloudPose(xyz.double(), f, None, pose.double()), feats.double(), gy.double(), dev)
    assert ref['out'].dtype == torch.float64 and low['out'].dtype == torch.float32
    print('float32 regime', low['logs'][0], low['logs'][1])
    for k, bar in (('out', 1e-5), ('gfeats', 1e-5), ('gW', 2e-5)):
        S.check(low[k], ref[k], f'float32 layer against the float64 layer, {k}', bar)


# ------------------------------------------------------------------------------------------------
# what stays float32 only
# ------------------------------------------------------------------------------------------------
def test_refusals_say_float64_and_launch_no_conv(dev, monkeypatch):
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    import vgtk.spconv as zptk
    from vgtk import _hip
    from vgtk.so3conv.blocks import BatchNormLeakyReLU, InstanceNormLeakyReLU, conv_norm_act
    d = torch.float64
    gen = torch.Generator().manual_seed(16)
    P = 12
    xyz = torch.rand(1, 3, P, generator=gen, dtype=d).to(dev)
    pose = torch.eye(4, dtype=d).repeat(1, P, 1, 1)
    pose[0, :, :3, :3] = S.rand_rot(gen, P)
    pose = pose.to(dev)
    feats = torch.ones(1, 2, P, 60, dtype=d, device=dev)
    launched = []
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda name, *a, **k: (launched.append(name), real(name, *a, **k))[1])
    L.FORWARD_LOG = []
    try:
        with pytest.raises(RuntimeError, match='use_2d.*float64'):
            sptk.InterSO3PoseConv(2, 4, 1, 1, 0.5, 0.05, 4, use_2d=True).double().to(dev)(
                zptk.SphericalPointCloudPose(xyz, torch.ones(1, 2, P, 240, dtype=d, device=dev), None, pose))
        with pytest.raises(RuntimeError, match='use_art_mode.*float64'):
            sptk.InterSO3PoseConv(2, 4, 1, 1, 0.5, 0.05, 4, use_art_mode=True).double().to(dev)(
                zptk.SphericalPointCloudPose(torch.stack([xyz, xyz], 1), feats, None, pose), seg=torch.zeros(1, P, dtype=torch.long, device=dev))
        with pytest.raises(RuntimeError, match='IntraSO3Conv2D.*float64'):
            sptk.IntraSO3Conv2D(2, 4).double().to(dev)(zptk.SphericalPointCloud(xyz, torch.ones(1, 2, P, 240, dtype=d, device=dev), None))
        conv = sptk.InterSO3PoseConv(2, 4, 1, 1, 0.5, 0.05, 4).double().to(dev)
        with pytest.raises(RuntimeError, match='epilogue.*float64'):
            conv_norm_act(conv, BatchNormLeakyReLU(4).to(dev), zptk.SphericalPointCloudPose(xyz, feats, None, pose))
        with pytest.raises(RuntimeError, match='BatchNormLeakyReLU.*float64'):
            BatchNormLeakyReLU(2).to(dev)(feats)
        with pytest.raises(RuntimeError, match='InstanceNormLeakyReLU.*float64'):
            InstanceNormLeakyReLU(2).to(dev)(feats)
        assert launched == [], launched
        # a really permuted 20-anchor cloud: the neighbour lists and the anchor map are looked at (they decide), no conv kernel runs
        k20 = sptk.InterSO3PoseConv(2, 4, 1, 1, 0.5, 0.05, 4, kanchor=20, permute_modes=1).double().to(dev)
        with pytest.raises(NotImplementedError, match='float64'):
            k20(zptk.SphericalPointCloudPose(xyz, feats[..., ::3].contiguous(), None, pose))
        print('launched before the 20-anchor refusal:', launched)
        assert launched and all(n in ('eap_ball_query_f64', 'eap_so3_anchor_map_f32') for n in launched)
        assert L.FORWARD_LOG == []
    finally:
        L.FORWARD_LOG = None
