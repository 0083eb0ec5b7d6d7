"""GPU: the pose-aware inter conv on the 20- and 40-anchor sets (the reference's `--kanchor` default is 20, SPConvNets/options.py:L38)
with per-point poses -- the 'anchor map' regime.  The two sets are subsets of the 60 icosahedral rotations (select_anchor,
so3conv/functional.py:L2641-2649), not groups: the anchor index argmax_j tr(R_rel^T A_a A_j^T) (L1199-1204) is searched per entry
(csrc/so3_anchor_map.hip) and is in general many-to-one; forward and backward go through it (csrc/so3_inter_map.hip).

Against the fixture the reference's own layer produced (tests/golden/make_golden_subsets.py) and against the oracle on larger clouds.

Ties: the arg-max runs in fp32 in an order nobody can mirror, so every test that compares indices (or values that depend on them)
first recomputes the traces in float64 from the oracle's expression and asserts, as a precondition on its own inputs, that the best
and the second-best trace are at least TIE_GAP apart -- ~20 x the fp32 rounding of a 9-term trace of magnitude <= 3.  No entry is left
out of a comparison."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import so3_ref  # noqa: E402  (checker only)

T = torch.from_numpy
TIE_GAP = 2e-5
BARS = (2e-5, 2e-5, 5e-5)           # out, dF, dW relative to the max norm: the bars of tests/test_gpu_2d.py for reference-made fixtures


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def rotations(gen, *shape):
    """unit-quaternion rotations [*shape,3,3]"""
    q = torch.randn(*shape, 4, generator=gen)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return R.view(*shape, 3, 3)


def oracle_index(ball_idx, q_pose, pose, anchors):
    """The oracle's expression (so3_ref.rotated_anchor_index) in float64 for R_rel = R_q R_idx^T
    -> (index int64 [b,p,nn,na], the smallest gap between the best and the second-best trace over ALL entries and anchors)"""
    rot, q_rot = pose[:, :, :3, :3].double(), q_pose[:, :, :3, :3].double()
    grouped = so3_ref.batched_index_select_other(rot, ball_idx.long(), dim=1)
    relr = torch.matmul(q_rot.unsqueeze(2), grouped.transpose(3, 4).contiguous())
    A = anchors.double()
    top = torch.einsum('bpnji,ajk,cik->bpnac', relr, A, A).topk(2, dim=-1).values
    return so3_ref.rotated_anchor_index(relr, A), float((top[..., 0] - top[..., 1]).min())


def anchors_of(na):
    import vgtk.so3conv.functional as L
    return T(np.ascontiguousarray(L.get_anchors(na)))


def count_calls(monkeypatch, record=None):
    """counters on the three entries of the anchor-map regime (record: a list that receives every map made)"""
    import vgtk.so3conv.functional as L
    calls = {'so3_anchor_map': 0, 'so3_inter_group_fwd_map': 0, 'so3_inter_group_bwd_map': 0}
    for name in calls:
        orig = getattr(L._hip, name)

        def wrapped(*a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            out = _orig(*a, **k)
            if record is not None and _name == 'so3_anchor_map':
                record.append(out[0])
            return out
        monkeypatch.setattr(L._hip, name, wrapped)
    return calls


# ---- 1. the module against the reference-made fixture ---------------------------------------------------------------------------------

@pytest.mark.parametrize('na', [20, 40])
@pytest.mark.parametrize('tag', ['random', 'parts', 'art_random'])
def test_module_against_the_reference_fixture(dev, golden, monkeypatch, na, tag):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    g = golden('inter_pose_subsets.npz')
    key, art = f'k{na}_{tag}', tag.startswith('art')
    B, P, NNB = 2, 40, 8
    pose, anchors = T(g[f'{key}_pose']), T(g[f'k{na}_anchors'])
    xyz = T(g['xyz_states'] if art else g['xyz'])
    seg = T(g['seg'])
    # precondition: no near-tie among this case's traces, and the stored index is the oracle's
    if art:
        per_state = torch.stack([so3_ref.ball_query(xyz[:, s].contiguous(), xyz[:, s].contiguous(), 0.2, NNB)[0].long() for s in range(xyz.shape[1])], 1)
        ball_idx = per_state.gather(1, seg.view(B, 1, P, 1).expand(B, 1, P, NNB)).squeeze(1)
    else:
        ball_idx = so3_ref.ball_query(xyz, xyz, 0.2, NNB)[0].long()
    want, gap = oracle_index(ball_idx, pose, pose, anchors)
    print(f'{key}: smallest trace gap {gap:.3e}')
    assert gap >= TIE_GAP
    assert np.array_equal(want.numpy(), g[f'{key}_rotated_anchor_idx'])

    maps = []
    calls = count_calls(monkeypatch, maps)
    conv = sptk.InterSO3PoseConv(4, 4, 1, 1, 0.2, 0.02, NNB, kanchor=na, permute_modes=1, use_art_mode=art).to(dev)
    assert np.allclose(conv.anchors.cpu().numpy(), g[f'k{na}_anchors'], atol=1e-6) and np.allclose(conv.kernels.cpu().numpy(), g['kernels'], atol=1e-7)
    with torch.no_grad():
        conv.basic_conv.W.copy_(T(g[f'{key}_W']))
    feats = T(g[f'{key}_feats']).to(dev).requires_grad_(True)
    L.BACKWARD_LOG, L.FORWARD_LOG = [], []
    try:
        x = zptk.SphericalPointCloudPose(xyz.to(dev), feats, None, pose.to(dev))
        inter_idx, w, sample_idx, out = conv(x, seg=seg.to(dev)) if art else conv(x)
        gF, gW = torch.autograd.grad(out.feats, [feats, conv.basic_conv.W], T(g[f'{key}_gy']).to(dev))
    finally:
        blog, flog, L.BACKWARD_LOG, L.FORWARD_LOG = L.BACKWARD_LOG, L.FORWARD_LOG, None, None
    assert out.feats.shape == (B, 4, P, na) and inter_idx is None and sample_idx is None
    assert [e['regime'] for e in blog] == ['anchor map'] and [e.get('regime') for e in flog] == ['anchor map']
    assert calls == {'so3_anchor_map': 1, 'so3_inter_group_fwd_map': 1, 'so3_inter_group_bwd_map': 1}
    # the map the conv used equals the reference's index, every entry
    assert len(maps) == 1 and maps[0].dtype == torch.uint8
    assert torch.equal(maps[0].cpu().long(), want)
    errs = (rel(out.feats.detach().cpu().numpy(), g[f'{key}_out']), rel(gF.cpu().numpy(), g[f'{key}_gfeats']), rel(gW.cpu().numpy(), g[f'{key}_gW']))
    print(f'{key}: out / dF / dW rel. error {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}')
    assert errs[0] < BARS[0] and errs[1] < BARS[1] and errs[2] < BARS[2]
    wm = w.materialize()[:, ::8, ::7, ::5].cpu().numpy()
    assert np.abs(wm - g[f'{key}_inter_w_sample']).max() < 2e-6


# ---- 2. map and layer against the oracle ----------------------------------------------------------------------------------------------

ORACLE_SEED = 2         # chosen on the CPU: the smallest trace gap of these inputs is >= TIE_GAP for both anchor sets (asserted below)


def oracle_case(seed=ORACLE_SEED):
    """B = 2, P = 128: cloud 0 with one rotation per rigid part + two points with their own rotation, cloud 1 with a rotation per point"""
    import synth_clouds
    gen = torch.Generator().manual_seed(seed)
    B, P = 2, 128
    xyz_np, lab, _ = synth_clouds.laptop_batch(81, B, P)
    pose = torch.eye(4).repeat(B, P, 1, 1)
    pose[0, :, :3, :3] = rotations(gen, 2)[T(lab[0])]
    pose[0, 5, :3, :3] = rotations(gen, 1)[0]
    pose[0, 77, :3, :3] = rotations(gen, 1)[0]
    pose[1, :, :3, :3] = rotations(gen, P)
    return T(xyz_np), pose, gen


@pytest.fixture(scope='module')
def oracle_inputs():
    xyz, pose, gen = oracle_case()
    feats = {na: torch.randn(2, 5, 128, na, generator=gen) for na in (20, 40)}
    W = torch.randn(8, 5 * 24, generator=gen) * 0.2
    gy = {na: torch.randn(2, 8, 128, na, generator=gen) for na in (20, 40)}
    return xyz, pose, feats, W, gy


@pytest.mark.parametrize('na', [20, 40])
def test_map_and_layer_against_the_oracle(dev, oracle_inputs, na):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    xyz, pose, feats_all, W0, gy_all = oracle_inputs
    B, P, NNB, C, O, radius, sigma = 2, 128, 16, 5, 8, 0.25, 0.03
    anchors = anchors_of(na)
    kernels = T(L.get_sphereical_kernel_points_from_ply(0.7 * radius, 1))
    ball_idx = so3_ref.ball_query(xyz, xyz, radius, NNB)[0].long()
    want, gap = oracle_index(ball_idx, pose, pose, anchors)
    print(f'{na} anchors: smallest trace gap {gap:.3e}')
    assert gap >= TIE_GAP
    got = L.anchor_permutation_index(xyz.to(dev), pose.to(dev), NNB, anchors.to(dev), radius)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    # many-to-one: some entry's map is no permutation of the anchors
    distinct = (torch.nn.functional.one_hot(want, na).sum(-2) > 0).sum(-1)
    assert int(distinct.min()) < na

    feats = feats_all[na].clone().requires_grad_(True)
    W = W0.clone().requires_grad_(True)
    ref = so3_ref.inter_so3poseconv_layer(xyz, pose, feats, W, anchors, kernels, radius, sigma, NNB, permute_modes=1)
    rF, rW = torch.autograd.grad(ref, [feats, W], gy_all[na])
    conv = sptk.InterSO3PoseConv(C, O, 1, 1, radius, sigma, NNB, kanchor=na, permute_modes=1).to(dev)
    with torch.no_grad():
        conv.basic_conv.W.copy_(W0)
    f = feats_all[na].to(dev).requires_grad_(True)
    L.BACKWARD_LOG = []
    try:
        y = conv(zptk.SphericalPointCloudPose(xyz.to(dev), f, None, pose.to(dev)))[3].feats
        gF, gW = torch.autograd.grad(y, [f, conv.basic_conv.W], gy_all[na].to(dev))
    finally:
        log, L.BACKWARD_LOG = L.BACKWARD_LOG, None
    assert [e['regime'] for e in log] == ['anchor map']
    errs = (rel(y.detach().cpu().numpy(), ref.detach().numpy()), rel(gF.cpu().numpy(), rF.numpy()), rel(gW.cpu().numpy(), rW.numpy()))
    print(f'{na} anchors: out / dF / dW rel. error {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}')
    assert errs[0] < BARS[0] and errs[1] < BARS[1] and errs[2] < BARS[2]


# ---- 3. repeat-padded lists, a width of more than one channel chunk ---------------------------------------------------------------------

DUP_SEED = 2            # chosen on the CPU like ORACLE_SEED


def dup_case(seed=DUP_SEED):
    import synth_clouds
    gen = torch.Generator().manual_seed(seed)
    P = 256
    xyz = T(synth_clouds.laptop_batch(57, 1, P)[0])
    pose = torch.eye(4).repeat(1, P, 1, 1)
    pose[0, :, :3, :3] = rotations(gen, P)
    return xyz, pose, gen


def test_repeat_padded_lists_and_width(dev):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    import vgtk.cuda.grouping as cuda_nn
    B, P, NNB, C, O, na, radius, sigma = 1, 256, 32, 32, 64, 20, 0.12, 0.01
    xyz, pose, gen = dup_case()
    anchors = anchors_of(na)
    kernels = T(L.get_sphereical_kernel_points_from_ply(0.7 * radius, 1))
    ball_idx = cuda_nn.ball_query(xyz.to(dev), xyz.to(dev), radius, NNB).cpu().long()
    assert torch.equal(ball_idx, so3_ref.ball_query(xyz, xyz, radius, NNB)[0].long())
    srt = ball_idx.sort(dim=-1).values
    padded = (srt[..., 1:] == srt[..., :-1]).any(-1)
    assert bool(padded.any()) and not bool(padded.all())           # some lists name a row twice, some are full
    _, gap = oracle_index(ball_idx, pose, pose, anchors)
    print(f'smallest trace gap {gap:.3e}; padded lists {int(padded.sum())} of {P}')
    assert gap >= TIE_GAP
    feats0 = torch.randn(B, C, P, na, generator=gen)
    W0 = torch.randn(O, C * 24, generator=gen) * 0.1
    gy = torch.randn(B, O, P, na, generator=gen)
    feats, W = feats0.clone().requires_grad_(True), W0.clone().requires_grad_(True)
    ref = so3_ref.inter_so3poseconv_layer(xyz, pose, feats, W, anchors, kernels, radius, sigma, NNB, permute_modes=1, chunk=64)
    rF, rW = torch.autograd.grad(ref, [feats, W], gy)
    conv = sptk.InterSO3PoseConv(C, O, 1, 1, radius, sigma, NNB, kanchor=na, permute_modes=1).to(dev)
    with torch.no_grad():
        conv.basic_conv.W.copy_(W0)
    f = feats0.to(dev).requires_grad_(True)
    L.BACKWARD_LOG = []
    try:
        y = conv(zptk.SphericalPointCloudPose(xyz.to(dev), f, None, pose.to(dev)))[3].feats
        gF, gW = torch.autograd.grad(y, [f, conv.basic_conv.W], gy.to(dev), retain_graph=True)
        gF2, gW2 = torch.autograd.grad(y, [f, conv.basic_conv.W], gy.to(dev))
    finally:
        log, L.BACKWARD_LOG = L.BACKWARD_LOG, None
    assert [e['regime'] for e in log] == ['anchor map', 'anchor map']
    assert torch.equal(gF, gF2) and torch.equal(gW, gW2)           # no float atomics: bit-identical run to run
    errs = (rel(y.detach().cpu().numpy(), ref.detach().numpy()), rel(gF.cpu().numpy(), rF.numpy()), rel(gW.cpu().numpy(), rW.numpy()))
    print(f'out / dF / dW rel. error {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}')
    assert errs[0] < BARS[0] and errs[1] < BARS[1] and errs[2] < BARS[2]


# ---- 4. the strided grouping of the functional API --------------------------------------------------------------------------------------

def test_strided_grouping_against_the_oracle(dev, oracle_inputs):
    import vgtk.so3conv.functional as L
    xyz, pose, feats_all, _, _ = oracle_inputs
    na, NNB, radius, sigma, stride = 20, 16, 0.25, 0.03, 2
    anchors = anchors_of(na)
    kernels = T(L.get_sphereical_kernel_points_from_ply(0.7 * radius, 1))
    feats = feats_all[na]
    ref = so3_ref.inter_so3poseconv_grouping_strided_sampled(xyz, pose, feats, stride, NNB, anchors, kernels, radius, sigma, permute_modes=1)
    # precondition on the centres' entries (query poses = the sampled ones)
    ball_idx = so3_ref.ball_query(ref[2], xyz, radius, NNB)[0].long()
    _, gap = oracle_index(ball_idx, ref[5], pose, anchors)
    print(f'strided: smallest trace gap {gap:.3e}')
    assert gap >= TIE_GAP
    out = L.inter_so3poseconv_grouping_strided(xyz.to(dev), pose.to(dev), feats.to(dev), stride, NNB, anchors.to(dev), kernels.to(dev), radius, sigma,
                                               permute_modes=1)
    assert out[0] is None and out[3].shape == (2, 5, 24, 64, na)
    assert torch.equal(out[4].cpu(), ref[4].long())                                  # sample_idx
    assert torch.equal(out[2].cpu(), ref[2]) and torch.equal(out[5].cpu(), ref[5])
    err = rel(out[3].cpu().numpy(), ref[3].numpy())
    print(f'strided: new_feats rel. error {err:.2e}')
    assert err < 5e-6
    # really through the map: the same call without permutation differs
    plain = L.inter_so3poseconv_grouping_strided(xyz.to(dev), pose.to(dev), feats.to(dev), stride, NNB, anchors.to(dev), kernels.to(dev), radius, sigma,
                                                 permute_modes=0)
    assert not torch.equal(plain[3], out[3])


# ---- 5. identity poses: exactly the call without permutation ---------------------------------------------------------------------------

def test_identity_poses_continue_as_without_permutation(dev, monkeypatch):
    import synth_clouds
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    B, P, c, o, na = 1, 512, 16, 128, 20
    _, _, radius, sigma = synth_clouds.backbone_layers(4096)[2]
    xyz = T(synth_clouds.laptop_batch(91, B, P)[0]).to(dev)
    pose = torch.eye(4, device=dev).repeat(B, P, 1, 1)
    gen = torch.Generator(device=dev).manual_seed(5)
    feats0 = torch.randn(B, c, P, na, device=dev, generator=gen)
    gy = torch.randn(B, o, P, na, device=dev, generator=gen)
    calls = count_calls(monkeypatch)
    outs = []
    for pm in (1, 0):
        torch.manual_seed(2913)
        conv = sptk.InterSO3PoseConv(c, o, 1, 1, radius, sigma, 64, kanchor=na, permute_modes=pm).to(dev)
        feats = feats0.clone().requires_grad_(True)
        L.BACKWARD_LOG, L.FORWARD_LOG = [], []
        try:
            y = conv(zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
            gF, gW = torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)
        finally:
            blog, flog, L.BACKWARD_LOG, L.FORWARD_LOG = L.BACKWARD_LOG, L.FORWARD_LOG, None, None
        outs.append((y.detach(), gF, gW, blog, flog))
    # the map was made once (permute_modes = 1), found trivial, and nothing went through it
    assert calls == {'so3_anchor_map': 1, 'so3_inter_group_fwd_map': 0, 'so3_inter_group_bwd_map': 0}
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert outs[0][3] == outs[1][3] and outs[0][4] == outs[1][4] and len(outs[0][3]) == 1
    assert outs[0][3][0]['regime'] != 'anchor map'


# ---- 6. closed anchor sets stay where they were ------------------------------------------------------------------------------------------

def test_closed_sets_never_reach_the_map_entries(dev, monkeypatch, oracle_inputs):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    xyz, pose, _, _, _ = oracle_inputs
    gen = torch.Generator().manual_seed(3)
    feats = torch.randn(2, 5, 128, 60, generator=gen).to(dev).requires_grad_(True)
    gy = torch.randn(2, 8, 128, 60, generator=gen).to(dev)
    calls = count_calls(monkeypatch)
    torch.manual_seed(2913)
    conv = sptk.InterSO3PoseConv(5, 8, 1, 1, 0.25, 0.03, 16, kanchor=60, permute_modes=1).to(dev)
    L.BACKWARD_LOG, L.FORWARD_LOG = [], []
    try:
        y = conv(zptk.SphericalPointCloudPose(xyz.to(dev), feats, None, pose.to(dev)))[3].feats
        torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)
        idx = L.anchor_permutation_index(xyz.to(dev), pose.to(dev), 16, conv.anchors, 0.25)
    finally:
        blog, flog, L.BACKWARD_LOG, L.FORWARD_LOG = L.BACKWARD_LOG, L.FORWARD_LOG, None, None
    assert calls == {'so3_anchor_map': 0, 'so3_inter_group_fwd_map': 0, 'so3_inter_group_bwd_map': 0}
    assert len(blog) == 1 and blog[0]['regime'] in ('inverse lists', 'textbook dX', 'dense rows') and 'regime' not in flog[0]
    # a group's index is a permutation of the anchors in every entry
    assert idx.shape == (2, 128, 16, 60) and bool((idx.sort(dim=-1).values == torch.arange(60, device=dev)).all())
