"""GPU: the 'residual map' regime of the `use_2d` inter conv (csrc/so3_inter_res.hip; so3conv/functional.py:L1934-1957, L2124) -- poses that
really permute the residual index of the 60 x 4 anchor axis: the per-entry index as one byte, the grouping through it for all 240 anchors
and its transpose without float atomics, one autograd node.

Inputs (every test asserts the precondition itself: the smallest gap between the best and the second-best of an entry's four traces,
evaluated in float64 on the host, is > 1e-4 -- two orders above the fp32 evaluation error, so the kernel's index must equal the tensor
form's on EVERY entry):
  T-fix  tests/golden/inter_pose_2d.npz `random_pm1`: 40 points, 8 neighbours, r = 0.2, one rotation per point (made by the reference)
  T-A    synth_clouds.laptop_batch(93, 2, 300), r = 0.12, 32 neighbours, seed 78: one rotation per rigid part + 7 points of their own
  T-B    laptop_batch(95, 1, 520), r = 0.16, 64 neighbours, seed 79, the same way
Bars: grouped features 5e-6 of the largest magnitude (the project's bar for them), their transpose 2e-5, the module 2e-5 / 2e-5 / 5e-5 for
y / dF / dW (the bars of the reference-made fixture's test)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = torch.from_numpy
OWN_POSE_POINTS = (3, 5, 64, 65, 127, 255, -1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def quat_to_R(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w_, x_, y_, z_ = q.unbind(-1)
    return torch.stack([1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - z_ * w_), 2 * (x_ * z_ + y_ * w_), 2 * (x_ * y_ + z_ * w_), 1 - 2 * (x_ * x_ + z_ * z_),
                        2 * (y_ * z_ - x_ * w_), 2 * (x_ * z_ - y_ * w_), 2 * (y_ * z_ + x_ * w_), 1 - 2 * (x_ * x_ + y_ * y_)], -1).view(*q.shape[:-1], 3, 3)


class Case:
    def __init__(self, dev, xyz, pose, radius, nn, sigma):
        import vgtk.cuda.grouping as cuda_nn
        self.xyz, self.pose, self.radius, self.nn, self.sigma = xyz.to(dev).contiguous(), pose.to(dev).contiguous(), radius, nn, sigma
        self.idx = cuda_nn.ball_query(self.xyz, self.xyz, radius, nn)
        self.B, self.P = xyz.shape[0], xyz.shape[2]


def _synth(dev, start, B, P, radius, nn, seed):
    import synth_clouds
    xyz_np, lab, _ = synth_clouds.laptop_batch(start, B, P)
    gen = torch.Generator().manual_seed(seed)
    R = quat_to_R(torch.randn(B, 2, 4, generator=gen))
    pose = torch.eye(4).repeat(B, P, 1, 1)
    for b in range(B):
        pose[b, :, :3, :3] = R[b][T(lab[b]).long()]
    Rp = quat_to_R(torch.randn(7, 4, generator=gen))
    for i, pt in enumerate(OWN_POSE_POINTS):
        pose[0, pt, :3, :3] = Rp[i]
    return Case(dev, T(xyz_np), pose, radius, nn, radius * radius / 2)


@pytest.fixture(scope='module')
def cases(dev, golden):
    g = golden('inter_pose_2d.npz')
    return {'T-fix': Case(dev, T(g['xyz']), T(g['random_pm1_pose']), 0.2, 8, 0.02),
            'T-A': _synth(dev, 93, 2, 300, 0.12, 32, 78),
            'T-B': _synth(dev, 95, 1, 520, 0.16, 64, 79)}


def _trace_gap(case):
    """smallest gap between the largest and the second largest of tr(R_rel^T RES_z RES_j^T), j = 0..3, over every entry and z: float64, host"""
    import vgtk.so3conv.functional as L
    res = L.RES_ROT_2D.double()
    rot = case.pose.cpu().double()[:, :, :3, :3]
    idx = case.idx.cpu().long()
    grouped = rot[torch.arange(case.B)[:, None, None], idx]                                  # [b,p,nn,3,3]
    r_rel = rot[:, :, None] @ grouped.transpose(-1, -2)
    ra = r_rel.transpose(-1, -2)[:, :, :, None] @ res                                        # [b,p,nn,4,3,3]
    tr = torch.einsum('bpnzik,jik->bpnzj', ra, res)
    top = tr.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


# ---- 1. the index kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['T-fix', 'T-A', 'T-B'])
def test_index_kernel_equals_the_tensor_form_on_every_entry(dev, cases, name):
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    case = cases[name]
    gap = _trace_gap(case)
    print(f'{name}: smallest trace gap {gap:.3g}')
    assert gap > 1e-4
    packed, nontrivial = _hip.so3_residual_index(case.idx, case.pose, case.pose, L._res_rot_2d(dev))
    want = L.residual_rotation_index(case.pose, case.idx)
    got = _hip.residual_index_unpack(packed)
    assert packed.dtype == torch.uint8 and packed.shape == case.idx.shape
    assert torch.equal(got, want)
    assert set(want.unique().tolist()) == {0, 1, 2, 3} and bool((packed != _hip.RESIDUAL_IDENTITY_BYTE).any())
    # the per-cloud flag is exactly the tensor form's "some entry is not (0, 1, 2, 3)": 1 for every cloud but T-A's second one, whose single
    # part-to-part rotation stays nearest to the identity among the four residual rotations (the oracle's index is unpermuted there too)
    assert nontrivial.tolist() == (want != torch.arange(4, device=dev)).flatten(1).any(1).int().tolist()
    assert nontrivial.tolist() == {'T-fix': [1], 'T-A': [1, 0], 'T-B': [1]}[name]
    # unpermuted: identity poses, one rotation per cloud
    eye = torch.eye(4, device=dev).repeat(case.B, case.P, 1, 1)
    one = eye.clone()
    one[:, :, :3, :3] = quat_to_R(torch.randn(case.B, 1, 4, generator=torch.Generator().manual_seed(3))).to(dev)
    for pose in (eye, one):
        packed, nontrivial = _hip.so3_residual_index(case.idx, pose, pose, L._res_rot_2d(dev))
        assert nontrivial.tolist() == [0] * case.B and bool((packed == _hip.RESIDUAL_IDENTITY_BYTE).all())


# ---- 2., 3. the grouping kernels at the ABI, any byte ----------------------------------------------------------------------------------

def _group_f64(feats, idx, gx, rk, fields, sigma, chunk=100):
    """The gather + einsum expression of _conv_2d in float64: feats [b,c,n,240] (a shadow row of zeros appended: idx == n), idx long [b,p,nn],
    gx [b,p,nn,3], rk [240,ks,3], fields long [b,p,nn,4] -> [b,c,ks,p,240]"""
    b, c, n, na4 = feats.shape
    na, ks, p = na4 // 4, rk.shape[1], idx.shape[1]
    fs = torch.cat([feats.view(b, c, n, na, 4), torch.zeros(b, c, 1, na, 4, dtype=feats.dtype, device=feats.device)], dim=2)
    trans = fs.permute(0, 2, 3, 4, 1)                                                        # [b,n+1,na,4,c]
    bi = torch.arange(b, device=feats.device)[:, None, None]
    outs = []
    for s0 in range(0, p, chunk):
        s1 = min(p, s0 + chunk)
        d = gx[:, s0:s1, :, None, None, :] - rk                                              # [b,pc,nn,240,ks,3]
        w = torch.relu(1 - (d * d).sum(-1) / sigma).view(b, s1 - s0, -1, na, 4, ks)
        g = trans[bi, idx[:, s0:s1]]                                                         # [b,pc,nn,na,4,c]
        g = torch.gather(g, 4, fields[:, s0:s1, :, None, :, None].expand(-1, -1, -1, na, -1, c))
        outs.append(torch.einsum('bpnazc,bpnazk->bckpaz', g, w).reshape(b, c, ks, s1 - s0, na4))
    return torch.cat(outs, dim=3)


class Grouping:
    """T-A's geometry, 16 channels, RANDOM index bytes (non-cyclic and many-to-one maps), with and without shadow-row entries; the float64
    forward and its autograd, made once.  The 5-channel cases are the first 5 channels: the op is independent per channel."""

    def __init__(self, dev, case):
        import vgtk.so3conv.functional as L
        from vgtk import _hip
        gen = torch.Generator().manual_seed(401)
        B, P, NN, C = case.B, case.P, case.nn, 16
        anchors = T(np.ascontiguousarray(L.get_anchors(60))).to(dev)
        kernels = T(L.get_sphereical_kernel_points_from_ply(0.7 * case.radius, 1)).to(dev)
        tot = torch.matmul(anchors.unsqueeze(1), L._res_rot_2d(dev).unsqueeze(0)).contiguous()
        self.rk = L.rotated_kernels(tot.view(240, 3, 3), kernels)
        self.gx, _ = _hip.so3_prep(case.xyz, case.xyz, case.idx, case.pose, case.pose, anchors, 0)
        self.sigma, self.n = case.sigma, P
        self.shift = torch.randint(0, 256, (B, P, NN), generator=gen).to(torch.uint8).to(dev)
        self.feats = torch.randn(B, C, P, 240, generator=gen).to(dev)
        self.gout = torch.randn(B, C, 24, P, 240, generator=gen).to(dev)
        shadow = case.idx.clone()
        shadow[torch.rand(B, P, NN, generator=gen).to(dev) < 0.07] = P                         # the shadow row
        self.idx = {'plain': case.idx, 'shadow': shadow}
        assert int((shadow == P).sum()) > 100 and int(case.idx.max()) < P
        self.ref = {}
        fields = _hip.residual_index_unpack(self.shift)
        for kind, idx in self.idx.items():
            f64 = self.feats.double().requires_grad_(True)
            out = _group_f64(f64, idx.long(), self.gx[..., :3].double(), self.rk.double(), fields, self.sigma)
            gf, = torch.autograd.grad(out, f64, self.gout.double())
            self.ref[kind] = (out.detach(), gf)


@pytest.fixture(scope='module')
def grouping(dev, cases):
    return Grouping(dev, cases['T-A'])


GROUPING_CASES = [(5, 'plain'), (16, 'plain'), (5, 'shadow')]


@pytest.mark.parametrize('c,kind', GROUPING_CASES)
def test_grouping_forward_at_the_abi_takes_any_byte(grouping, c, kind):
    from vgtk import _hip
    g = grouping
    assert len(g.shift.unique()) == 256
    out = _hip.so3_inter_group_fwd_res(g.feats[:, :c].contiguous(), g.idx[kind], g.gx, g.rk, g.shift, g.sigma)
    want = g.ref[kind][0][:, :c]
    err = rel(out, want)
    print(f'forward c = {c} {kind}: {err:.3g}')
    assert out.shape == want.shape and err < 5e-6
    if kind == 'shadow':                 # ... and the shadow entries did contribute nothing: the plain lists give another result
        assert rel(g.ref['plain'][0][:, :c], want) > 1e-3


@pytest.mark.parametrize('c,kind', GROUPING_CASES)
def test_grouping_backward_at_the_abi_is_the_transpose_and_bit_equal_run_to_run(grouping, c, kind):
    from vgtk import _hip
    g = grouping
    gout = g.gout[:, :c].contiguous()
    first = _hip.so3_inter_group_bwd_res(gout, g.idx[kind], g.gx, g.rk, g.shift, g.sigma, g.n)
    again = _hip.so3_inter_group_bwd_res(gout, g.idx[kind], g.gx, g.rk, g.shift, g.sigma, g.n)
    want = g.ref[kind][1][:, :c]
    err = rel(first, want)
    print(f'backward c = {c} {kind}: {err:.3g}')
    assert first.shape == want.shape and err < 2e-5
    assert torch.equal(first, again)


# ---- 4. the module against the reference-made fixture -----------------------------------------------------------------------------------

class Logs:
    """FORWARD_LOG / BACKWARD_LOG switched on for a block"""

    def __enter__(self):
        import vgtk.so3conv.functional as L
        L.FORWARD_LOG, L.BACKWARD_LOG = [], []
        self.fwd, self.bwd = L.FORWARD_LOG, L.BACKWARD_LOG
        return self

    def __exit__(self, *exc):
        import vgtk.so3conv.functional as L
        L.FORWARD_LOG = L.BACKWARD_LOG = None

    def regimes(self):
        return [e.get('regime') for e in self.fwd], [e.get('regime') for e in self.bwd]


def test_module_against_the_reference_fixture_on_the_kernels(dev, golden, monkeypatch):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    g = golden('inter_pose_2d.npz')
    tag = 'random_pm1'
    monkeypatch.setattr(L, 'KERNEL_2D_MIN_POINTS', 0)
    slow = []
    orig = L._hip.so3_inter_weights
    monkeypatch.setattr(L._hip, 'so3_inter_weights', lambda *a, **k: (slow.append(1), orig(*a, **k))[1])
    conv = sptk.InterSO3PoseConv(4, 4, 1, 1, 0.2, 0.02, 8, kanchor=60, permute_modes=1, use_2d=True).to(dev)
    with torch.no_grad():
        conv.basic_conv.W.copy_(T(g[f'{tag}_W']))
    feats = T(g[f'{tag}_feats']).to(dev).requires_grad_(True)
    with Logs() as logs:
        _, w, _, out = conv(zptk.SphericalPointCloudPose(T(g['xyz']).to(dev), feats, None, T(g[f'{tag}_pose']).to(dev)))
        assert not slow                                                      # the materialised weights were not asked for
        gF, gW = torch.autograd.grad(out.feats, [feats, conv.basic_conv.W], T(g[f'{tag}_gy']).to(dev))
    assert logs.regimes() == (['residual map'], ['residual map'])
    errs = (rel(out.feats.detach().cpu(), T(g[f'{tag}_out'])), rel(gF.cpu(), T(g[f'{tag}_gfeats'])), rel(gW.cpu(), T(g[f'{tag}_gW'])))
    print('fixture: y %.3g dF %.3g dW %.3g' % errs)
    assert out.feats.shape == (1, 4, 40, 240)
    assert errs[0] < 2e-5 and errs[1] < 2e-5 and errs[2] < 5e-5
    wm = w.materialize().view(1, 40, 240, 24, 8)[:, ::8, ::7, ::5].cpu().numpy()
    assert np.abs(wm - g[f'{tag}_inter_w_sample']).max() < 2e-6


# ---- 5. the module against the tensor form at width ------------------------------------------------------------------------------------

def _run_module(case, c, o, pm, feats0, gy, pose=None, seed=2913):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    torch.manual_seed(seed)
    conv = sptk.InterSO3PoseConv(c, o, 1, 1, case.radius, case.sigma, case.nn, kanchor=60, permute_modes=pm, use_2d=True).to(feats0.device)
    feats = feats0.clone().requires_grad_(True)
    with Logs() as logs:
        y = conv(zptk.SphericalPointCloudPose(case.xyz, feats, None, case.pose if pose is None else pose))[3].feats
        gF, gW = torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)
    return (y.detach(), gF, gW), logs.regimes()


@pytest.mark.parametrize('name,c,o', [('T-B', 16, 128), ('T-A', 5, 7)])
def test_module_against_the_tensor_form(dev, cases, monkeypatch, name, c, o):
    import vgtk.so3conv.functional as L
    case = cases[name]
    gen = torch.Generator(device=dev).manual_seed(5)
    feats0 = torch.randn(case.B, c, case.P, 240, device=dev, generator=gen)
    gy = torch.randn(case.B, o, case.P, 240, device=dev, generator=gen)
    got, regimes = _run_module(case, c, o, 1, feats0, gy)
    assert regimes == (['residual map'], ['residual map'])
    monkeypatch.setattr(L, 'FORCE_GENERAL_2D', True)
    want, regimes = _run_module(case, c, o, 1, feats0, gy)
    assert regimes == ([], [])
    errs = tuple(rel(a_, b_) for a_, b_ in zip(got, want))
    print(f'{name} {c} -> {o}: y %.3g dF %.3g dW %.3g' % errs)
    assert errs[0] < 2e-5 and errs[1] < 2e-5 and errs[2] < 5e-5


# ---- 6. routing -------------------------------------------------------------------------------------------------------------------------

def test_an_unpermuted_index_still_takes_the_four_fused_convolutions(dev, cases):
    case = cases['T-A']
    c, o = 5, 7
    gen = torch.Generator(device=dev).manual_seed(6)
    feats0 = torch.randn(case.B, c, case.P, 240, device=dev, generator=gen)
    gy = torch.randn(case.B, o, case.P, 240, device=dev, generator=gen)
    eye = torch.eye(4, device=dev).repeat(case.B, case.P, 1, 1)
    one = eye.clone()
    one[:, :, :3, :3] = quat_to_R(torch.randn(case.B, 1, 4, generator=torch.Generator().manual_seed(3))).to(dev)
    for pose in (eye, one):
        outs = {}
        for pm in (1, 0):
            outs[pm], (fwd, bwd) = _run_module(case, c, o, pm, feats0, gy, pose=pose)
            assert len(fwd) == 4 and len(bwd) == 4 and 'residual map' not in fwd + bwd
        assert torch.equal(outs[1][0], outs[0][0])                            # the output, bit for bit
        # (the gradients: the same four nodes, whose backward regime may follow the layer's previous step -- the module's bars)
        assert rel(outs[1][1], outs[0][1]) < 2e-5 and rel(outs[1][2], outs[0][2]) < 5e-5


def test_a_cloud_of_one_slab_keeps_the_tensor_form(dev, cases, monkeypatch):
    import vgtk.so3conv.functional as L
    case = cases['T-fix']
    assert case.P == 40 < L.KERNEL_2D_MIN_POINTS == L.SLOW_2D_CHUNK + 1
    slow = []
    orig = L._hip.so3_inter_weights
    monkeypatch.setattr(L._hip, 'so3_inter_weights', lambda *a, **k: (slow.append(1), orig(*a, **k))[1])
    gen = torch.Generator(device=dev).manual_seed(7)
    feats0 = torch.randn(1, 4, 40, 240, device=dev, generator=gen)
    gy = torch.randn(1, 4, 40, 240, device=dev, generator=gen)
    _, regimes = _run_module(case, 4, 4, 1, feats0, gy)
    assert regimes == ([], []) and len(slow) == 1


# ---- 7. memory: what the regime is for ---------------------------------------------------------------------------------------------------

def test_the_kernels_need_less_memory_than_the_tensor_form(dev, cases, monkeypatch):
    """T-B at 64 -> 128 channels, forward + backward: the tensor form keeps, per slab of 64 points, the gathered features [b,64,nn,60,4,c], the
    materialised weights [b,64,60,4,24,nn] and the grouped tensor for autograd; the kernels keep X [b,c,ks,p,240] once."""
    import gc
    import vgtk.so3conv.functional as L
    case = cases['T-B']
    c, o = 64, 128
    gen = torch.Generator(device=dev).manual_seed(8)
    feats0 = torch.randn(case.B, c, case.P, 240, device=dev, generator=gen)
    gy = torch.randn(case.B, o, case.P, 240, device=dev, generator=gen)
    peak = {}
    for form in ('kernels', 'tensor form'):
        monkeypatch.setattr(L, 'FORCE_GENERAL_2D', form == 'tensor form')
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        outs, regimes = _run_module(case, c, o, 1, feats0, gy)
        torch.cuda.synchronize()
        peak[form] = torch.cuda.max_memory_allocated() - base
        assert regimes == ((['residual map'],) * 2 if form == 'kernels' else ([], []))
        del outs
    print('peak memory above the inputs: kernels %.0f MB, tensor form %.0f MB' % (peak['kernels'] / 2 ** 20, peak['tensor form'] / 2 ** 20))
    assert peak['kernels'] < peak['tensor form']
