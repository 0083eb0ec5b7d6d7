"""GPU: PointnetSO3Conv / PointnetSO3PoseConv on csrc/pointnet_max.hip (vgtk.so3conv.pointnet_max: the 1x1 embed fused with the max over the
points, vgtk/vgtk/so3conv/modules.py:L393-413): the modules against the fixture the reference classes produced
(tests/golden/pointnet_max.npz), the entries through the C ABI against float64 under the bounds of tests/pointnet_max_common.py, every
point index as an arg, ties, masks, NaN, offset storage, the memory the fused form may take, kernel attribution, and
pose_head_over_subsets with 'pointnet' pooling against the per-cloud loop.  Outputs are carved between sentinels and every run is made
twice: guard bands intact, every element written, the two runs bit-identical."""
import copy

import numpy as np
import pytest
import torch

import pointnet_max_common as P

pytestmark = pytest.mark.gpu

GUARD = 64                               # elements of the sentinel on either side of an output
SENTINEL = 0x7FC5A5A5                    # as float32 a NaN: a kernel that reads its output before writing it shows, too


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


class Carved:
    """an output tensor inside a larger buffer: 16-byte aligned, GUARD elements of SENTINEL in front of and behind it"""

    def __init__(self, shape, dtype, dev, fill=SENTINEL):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.t = self.buf[GUARD:GUARD + self.numel].view(dtype).view(shape)
        if fill != SENTINEL:
            self.t.view(torch.int32).fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.numel:] == SENTINEL).all())

    def bits(self):
        return self.buf[GUARD:GUARD + self.numel]


def _twice(run, sparse=()):
    """run() -> {name: Carved}, two times into fresh buffers: guard bands intact, results bit-identical, every element written (the names
    in `sparse` are zero-filled by the caller and written only where a gradient lands) -> {name: device tensor}"""
    first, second = run(), run()
    torch.cuda.synchronize()
    for k in first:
        assert first[k].intact() and second[k].intact(), f'{k}: written outside the tensor'
        assert torch.equal(first[k].bits(), second[k].bits()), f'{k}: two runs differ'
        if k not in sparse:
            assert not bool((first[k].bits() == SENTINEL).any()), f'{k}: an element was not written'
    return {k: v.t for k, v in first.items()}


def _device(d, dev):
    return {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in d.items()}


def _forward(D, centre, v, member=None, feats=None):
    """eap_pointnet_max_fwd_f32 twice -> out, arg (device tensors)"""
    from vgtk import _hip
    feats = D['feats'] if feats is None else feats
    B, C, N, na = feats.shape
    O = D['w'].shape[0]
    parts = int(_hip.abi.eap_pointnet_max_parts(N))
    wt = D['w'][:, :C].t().contiguous()                    # [C, O]: the feature half of the weights, transposed

    def run():
        o = dict(out=Carved((B, O, na), torch.float32, dev=feats.device), arg=Carved((B, O, na), torch.int32, dev=feats.device),
                 pval=Carved((B, parts, O, na), torch.float32, dev=feats.device), parg=Carved((B, parts, O, na), torch.int32, dev=feats.device))
        _hip.call('eap_pointnet_max_fwd_f32', feats, B, C, O, N, na, feats, D['xyz'], centre, member, wt, v, D['bias'],
                  o['pval'].t, o['parg'].t, o['out'].t, o['arg'].t)
        return o

    got = _twice(run)
    return got['out'], got['arg']


def _backward(D, centre, arg, member=None):
    """the two backward entries twice -> dict(dfeats, dxyz, dw, dbias); the small tensor ops behind them as the operator has them"""
    from vgtk import _hip
    B, C, N, na = D['feats'].shape
    O = D['w'].shape[0]

    def run():
        o = dict(dfeats=Carved((B, C, N, na), torch.float32, dev=arg.device, fill=0), dcoords=Carved((B, 3, N, na), torch.float32, dev=arg.device, fill=0),
                 dwp=Carved((B, O, C + 4), torch.float32, dev=arg.device))
        _hip.call('eap_pointnet_max_bwd_data_f32', D['g'], B, C, O, N, na, D['g'], arg, D['w'], C + 3, o['dfeats'].t, o['dcoords'].t)
        _hip.call('eap_pointnet_max_bwd_weight_f32', D['g'], B, C, O, N, na, D['g'], arg, D['feats'], D['xyz'], centre, D['anchors'], o['dwp'].t)
        return o

    got = _twice(run, sparse=('dfeats', 'dcoords'))
    dxc = torch.einsum('aji,bina->bjn', D['anchors'], got['dcoords'])
    total = dxc.sum(2, keepdim=True)
    dxyz = dxc - total / N if member is None else dxc - member.unsqueeze(1) * (total / member.sum(1).clamp(min=1.0).view(B, 1, 1))
    dwp = got['dwp'].sum(0, dtype=torch.float64)
    return dict(dfeats=got['dfeats'], dxyz=dxyz, dw=dwp[:, :C + 3].float(), dbias=dwp[:, C + 3].float())


# ---- the modules against the reference's fixture ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('cls', ['conv', 'pose'])
@pytest.mark.parametrize('ka', [60, 20])
def test_module_matches_reference_golden(dev, golden, ka, cls):
    """out under the value bound; the reference's arg-max at every (b,o,a), so its gradients under the gradient bounds"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    G = golden('pointnet_max.npz')
    d = {k: np.asarray(G[f'{ka}_{k}']) for k in ('xyz', 'feats', 'g')}
    c, o = d['feats'].shape[1], d['g'].shape[1]
    net = sptk.PointnetSO3Conv(c, o, kanchor=ka) if cls == 'conv' else sptk.PointnetSO3PoseConv(c, o, kanchor=ka)
    net.load_state_dict({k[len(f'{ka}_{cls}_state_'):]: torch.from_numpy(v) for k, v in G.items() if k.startswith(f'{ka}_{cls}_state_')})
    net = net.to(dev)
    d.update(w=net.embed.weight.detach().cpu().numpy().reshape(o, c + 3), bias=net.embed.bias.detach().cpu().numpy(), anchors=net.anchors.cpu().numpy())
    D = _device(d, dev)
    x, f = D['xyz'].clone().requires_grad_(True), D['feats'].clone().requires_grad_(True)
    res = net(zptk.SphericalPointCloud(x, f, None))
    from vgtk import _hip
    assert _hip.abi.eap_last_kernel().decode() == f'pointnet_max_kernel<{ka}>', 'the module did not run the fused kernel'
    grads = torch.autograd.grad((res * D['g']).sum(), [f, x, net.embed.weight, net.embed.bias])
    centre = P.centre_of(D['xyz'])
    y, bound, out64, bound_out = P.value_reference(d, centre, P.table_of(D['anchors'], D['w'], c))
    ref_out = torch.from_numpy(np.asarray(G[f'{ka}_{cls}_out'])).double()
    assert bool(((res.detach().double().cpu() - ref_out).abs() <= bound_out).all()), 'against the reference-made output'
    assert bool(((res.detach().double().cpu() - out64).abs() <= bound_out).all())
    arg = y.argmax(2)                                       # (no near-tie in the fixture: the float32 runs agree with float64 on every arg)
    got = dict(dfeats=grads[0], dxyz=grads[1], dw=grads[2].view(o, c + 3), dbias=grads[3])
    print('fixture', ka, cls, P.check_gradients(got, d, arg, dev))
    for k, name in (('dfeats', 'grad_feats'), ('dxyz', 'grad_xyz'), ('dw', 'grad_weight'), ('dbias', 'grad_bias')):
        ref = np.asarray(G[f'{ka}_{cls}_{name}']).reshape(got[k].shape)
        assert np.abs(got[k].detach().cpu().numpy() - ref).max() <= 2e-5 * np.abs(ref).max(), (k, 'against the reference-made gradient')


def test_return_raw_is_the_concatenation_free_form(dev):
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    d = P.inputs(2, 16, 24, 37, 60, seed=9)
    net = sptk.PointnetSO3Conv(16, 24, kanchor=60, return_raw=True).to(dev)
    D = _device(d, dev)
    with torch.no_grad():
        res = net(zptk.SphericalPointCloud(D['xyz'], D['feats'], None))
    xc = D['xyz'] - D['xyz'].mean(2, keepdim=True)
    cat = torch.cat([D['feats'], torch.einsum('aji,bjn->bina', net.anchors, xc)], 1).double()
    ref = torch.nn.functional.conv2d(cat, net.embed.weight.detach().double(), net.embed.bias.detach().double())
    assert res.shape == ref.shape and float((res.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())


# ---- the entries through the C ABI against float64 -------------------------------------------------------------------------------------

# channels below a k-step and a prime N; just past a 128-point group and four 32-channel blocks + 2, 17 chunks; one point (arg 0, centred
# coordinates 0); the 20- and 12-anchor sets with a last chunk that holds a single point
ENTRY_SHAPES = [(2, 5, 3, 37, 60), (1, 64, 130, 130, 60), (3, 20, 24, 1, 60), (2, 16, 32, 257, 20), (2, 16, 32, 257, 12)]


@pytest.mark.parametrize('shape', ENTRY_SHAPES)
def test_entries_against_float64(dev, shape):
    B, C, O, N, na = shape
    d = P.inputs(B, C, O, N, na, seed=sum(shape))
    D = _device(d, dev)
    centre, v = P.centre_of(D['xyz']).contiguous(), P.table_of(D['anchors'], D['w'], C)
    out, arg = _forward(D, centre, v)
    y, bound, out64, bound_out = P.value_reference(d, centre, v)
    figures = dict(zip(('value', 'arg'), P.check_values(out.cpu(), arg.cpu(), y, out64, bound_out)))
    if N == 1:
        assert bool((arg == 0).all())
    figures.update(P.check_gradients(_backward(D, centre, arg), d, arg, dev))
    print('error / bound', shape, {k: round(x, 3) for k, x in figures.items()})


def test_every_point_is_some_channels_arg_and_ties_take_the_lowest(dev):
    """(1,64,130,130,60) with the maximum of channel o planted at point o: every point index, chunk and group boundaries included, is reported
    exactly; then point 5 copied onto point 70 (coordinates and features): the channel planted at 5 still reports 5"""
    d = P.planted()
    for tie in (False, True):
        if tie:
            d['feats'][:, :, 70] = d['feats'][:, :, 5]
            d['xyz'][:, :, 70] = d['xyz'][:, :, 5]
        D = _device(d, dev)
        centre, v = P.centre_of(D['xyz']).contiguous(), P.table_of(D['anchors'], D['w'], 64)
        out, arg = _forward(D, centre, v)
        y, bound, out64, bound_out = P.value_reference(d, centre, v)
        P.check_values(out.cpu(), arg.cpu(), y, out64, bound_out)
        want = torch.arange(130, device=dev).view(1, 130, 1).expand(1, 130, 60)
        if tie:
            assert bool((arg[0, 5] == 5).all()), 'equal values: the lowest point'
            keep = torch.ones(130, dtype=torch.bool, device=dev)
            keep[70] = False
            assert torch.equal(arg[0, keep].long(), want[0, keep])
        else:
            assert torch.equal(arg.long(), want)


def test_mask_non_members_never_win(dev):
    """a random half are members; the others carry features 100 x larger.  arg is always a member and the result equals, bit for bit, the
    entry on the gathered subset with the same centre; values and gradients under the bounds"""
    B, C, O, N, na = 2, 16, 32, 257, 60
    d = P.inputs(B, C, O, N, na, seed=21)
    rng = np.random.RandomState(5)
    member = rng.rand(B, N) < 0.5
    member[:, 0] = False
    member[:, 256] = True                      # the single point of the last chunk
    d['feats'] = np.where(member[:, None, :, None], d['feats'], 100.0 * d['feats']).astype(np.float32)
    D = _device(d, dev)
    m = torch.from_numpy(member.astype(np.float32)).to(dev)
    centre, v = P.centre_of(D['xyz'], m).contiguous(), P.table_of(D['anchors'], D['w'], C)
    out, arg = _forward(D, centre, v, member=m)
    y, bound, out64, bound_out = P.value_reference(d, centre, v, member=m)
    P.check_values(out.cpu(), arg.cpu(), y, out64, bound_out, member=m)
    for b in range(B):
        sel = torch.from_numpy(np.nonzero(member[b])[0]).to(dev)
        Ds = dict(D, xyz=D['xyz'][b:b + 1][:, :, sel].contiguous())
        sub_out, sub_arg = _forward(Ds, centre[b:b + 1].contiguous(), v, feats=D['feats'][b:b + 1][:, :, sel].contiguous())
        assert torch.equal(sub_out.view(torch.int32), out[b:b + 1].view(torch.int32)), 'the gathered subset, bit for bit'
        assert torch.equal(sel[sub_arg.long()], arg[b:b + 1].long())
    got = _backward(D, centre, arg, member=m)
    print('mask: error / bound', P.check_gradients(got, d, arg, dev, member=m))
    assert bool((got['dfeats'].permute(0, 2, 1, 3)[~torch.from_numpy(member).to(dev)] == 0).all()), 'non-members receive no gradient'
    assert bool((got['dxyz'].permute(0, 2, 1)[~torch.from_numpy(member).to(dev)] == 0).all())


def test_nan_wins_where_it_is_and_nowhere_else(dev):
    B, C, O, N, na = 2, 5, 35, 140, 60
    d = P.inputs(B, C, O, N, na, seed=33)
    D = _device(d, dev)
    centre, v = P.centre_of(D['xyz']).contiguous(), P.table_of(D['anchors'], D['w'], C)
    clean_out, clean_arg = _forward(D, centre, v)
    for (b, c, n, a) in ((1, 3, 131, 59), (0, 0, 0, 0), (0, 4, 77, 30)):
        feats = D['feats'].clone()
        feats[b, c, n, a] = float('nan')
        out, arg = _forward(D, centre, v, feats=feats)
        assert bool(torch.isnan(out[b, :, a]).all()) and bool((arg[b, :, a] == n).all())
        other = torch.ones(B, na, dtype=torch.bool, device=dev)
        other[b, a] = False
        sel = other.view(B, 1, na).expand(B, O, na)
        assert torch.equal(out.view(torch.int32)[sel], clean_out.view(torch.int32)[sel]) and torch.equal(arg[sel], clean_arg[sel])
    feats = D['feats'].clone()
    feats[0, 1, 100, 7] = feats[0, 2, 20, 7] = float('nan')                  # two NaN points of one anchor: the lowest
    out, arg = _forward(D, centre, v, feats=feats)
    assert bool(torch.isnan(out[0, :, 7]).all()) and bool((arg[0, :, 7] == 20).all())


def test_features_at_an_offset_of_4_bytes(dev):
    """include/eap_hip.h: every operand is moved by 4-byte words, any element-aligned address is taken -- the same bits"""
    B, C, O, N, na = 2, 5, 3, 37, 60
    d = P.inputs(B, C, O, N, na, seed=41)
    D = _device(d, dev)
    centre, v = P.centre_of(D['xyz']).contiguous(), P.table_of(D['anchors'], D['w'], C)
    out, arg = _forward(D, centre, v)
    big = torch.zeros(D['feats'].numel() + 8, device=dev)
    shifted = big[1:1 + D['feats'].numel()].view(B, C, N, na)
    shifted.copy_(D['feats'])
    assert shifted.data_ptr() % 16 == 4
    out2, arg2 = _forward(D, centre, v, feats=shifted)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(arg, arg2)
    import vgtk.so3conv as sptk
    res = sptk.pointnet_max(shifted, D['xyz'], D['w'], D['bias'], D['anchors'])
    assert torch.equal(res.view(torch.int32), out.view(torch.int32))


def test_nothing_of_the_size_of_the_map_is_allocated(dev):
    import vgtk.so3conv as sptk
    B, C, O, N, na = 2, 64, 64, 2048, 60
    gen = torch.Generator(device=dev).manual_seed(2)
    feats = torch.randn(B, C, N, na, device=dev, generator=gen).requires_grad_(True)
    xyz = torch.randn(B, 3, N, device=dev, generator=gen).requires_grad_(True)
    w = (torch.randn(O, C + 3, device=dev, generator=gen) / 8).requires_grad_(True)
    bias = torch.randn(O, device=dev, generator=gen).requires_grad_(True)
    anchors = torch.from_numpy(P.anchors_of(na)).to(dev)
    g = torch.randn(B, O, na, device=dev, generator=gen)
    map_bytes = 4 * B * O * N * na
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = sptk.pointnet_max(feats, xyz, w, bias, anchors)
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated() - base
    (out * g).sum().backward()
    torch.cuda.synchronize()
    both = torch.cuda.max_memory_allocated() - base
    print(f'peak above the inputs: forward {fwd / 2**20:.1f} MiB, forward + backward {both / 2**20:.1f} MiB; the map {map_bytes / 2**20:.1f} MiB')
    assert fwd <= map_bytes // 4
    assert both <= 4 * feats.numel() + map_bytes // 4
    assert feats.grad is not None and xyz.grad is not None and w.grad is not None and bias.grad is not None


def test_the_forward_names_its_kernel(dev):
    import vgtk.so3conv as sptk
    from vgtk import _hip
    for na, name in ((60, 'pointnet_max_kernel<60>'), (40, 'pointnet_max_kernel<40>'), (20, 'pointnet_max_kernel<20>'), (12, 'pointnet_max_kernel<12>'),
                     (8, 'pointnet_max_kernel<0>'), (64, 'pointnet_max_kernel<0>')):
        D = _device(P.inputs(1, 4, 6, 9, na, seed=na), dev)
        _hip.abi.eap_last_kernel()
        res = sptk.pointnet_max(D['feats'], D['xyz'], D['w'], D['bias'], D['anchors'])
        assert _hip.abi.eap_last_kernel().decode() == name
        xc = D['xyz'] - D['xyz'].mean(2, keepdim=True)
        ref = P.dense(D['feats'].double(), xc.double(), D['w'].double(), P.table_of(D['anchors'], D['w'], 4).double(), D['bias'].double()).max(2)[0]
        assert float((res.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ---- pose_head_over_subsets with the pointnet pooling ------------------------------------------------------------------------------------

def _rel(a, b):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def test_pose_head_over_subsets_with_pointnet_pooling(dev, A=60):
    """against the model's inner loop -- the head called once per cloud, batch 1, on the gathered subset with mask=None: every dictionary
    entry, the running statistics, the feature gradient and every parameter gradient, at the bars tests/test_gpu_lists_and_modules.py holds
    the mean / max modes to"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    torch.manual_seed(3)
    B, C, N = 3, 16, 40
    head = sptk.SO3OutBlockRTWithMaskSep({'dim_in': C, 'mlp': [32, 32], 'kanchor': A, 'temperature': 3.0}, norm=1, pooling_method='pointnet',
                                         pred_axis=True, pred_pv_points=True, pred_central_points=True).to(dev)
    feats = torch.randn(B, C, N, A, device=dev)
    xyz = torch.randn(B, 3, N, device=dev) * 0.3
    member = torch.rand(B, N, device=dev) > 0.5
    member[:, 0] = True
    member[1, 4:] = False; member[1, :4] = True                    # a 4-point subset
    anchors = torch.from_numpy(np.ascontiguousarray(L.get_anchors(A))).to(dev)
    keys = ('R', 'T', 'axis', 'pv_points', 'central_points')

    def loop(h, f):
        outs = []
        for b in range(B):
            sel = member[b].nonzero().squeeze(1)
            fx, px = f[b:b + 1, :, sel].contiguous(), xyz[b:b + 1, :, sel].contiguous()
            outs.append(h(zptk.SphericalPointCloud(px, fx, None), None, fx, trans_xyz=px, anchors=anchors.unsqueeze(0)))
        return {k: torch.cat([o[k] for o in outs], 0) for k in keys}

    for training in (True, False):
        ref_head, fast_head = copy.deepcopy(head).train(training), copy.deepcopy(head).train(training)
        with torch.no_grad():
            ref = loop(ref_head, feats)
            got = sptk.pose_head_over_subsets(fast_head, feats, xyz, member, anchors)
        for k in keys:
            assert got[k].shape == ref[k].shape, k
            assert _rel(got[k], ref[k]) < 2e-5, (training, k, _rel(got[k], ref[k]))
        for (k, v), (_, w) in zip(ref_head.state_dict().items(), fast_head.state_dict().items()):
            if 'running' in k:
                assert _rel(w, v) < 1e-5, k
        ref_head, fast_head = copy.deepcopy(head).train(training), copy.deepcopy(head).train(training)
        gen = torch.Generator().manual_seed(11)
        f_ref = feats.clone().requires_grad_(True)
        ref = loop(ref_head, f_ref)
        probes = {k: torch.randn(ref[k].shape, generator=gen).to(dev) for k in keys}
        sum((ref[k] * probes[k]).sum() for k in keys).backward()
        f_fast = feats.clone().requires_grad_(True)
        got = sptk.pose_head_over_subsets(fast_head, f_fast, xyz, member, anchors)
        sum((got[k] * probes[k]).sum() for k in keys).backward()
        assert _rel(f_fast.grad, f_ref.grad) < 5e-5, training
        assert (f_fast.grad.permute(0, 2, 1, 3)[~member] == 0).all(), 'points outside the subset must receive no gradient'
        seen = 0
        for (k, v), (_, w) in zip(ref_head.named_parameters(), fast_head.named_parameters()):
            if v.grad is None:
                assert w.grad is None or w.grad.abs().max().item() == 0.0, k
                continue
            pre_bn_bias = training and k.endswith('.bias') and (k.startswith('linear.') or k.startswith('trans_linear.') or k.startswith('regressor_dense_layer.0.'))
            if pre_bn_bias:        # a bias in front of a training-mode BatchNorm is absorbed by the batch mean: exactly zero in the fused backward
                top = max(float(p_.grad.abs().max()) for p_ in ref_head.parameters() if p_.grad is not None)
                assert float(v.grad.abs().max()) < 1e-4 * top and (w.grad is None or float(w.grad.abs().max()) == 0.0), k
            else:
                assert _rel(w.grad, v.grad) < 1e-4, (training, k, _rel(w.grad, v.grad))
            seen += k.startswith('pointnet.embed')
        assert seen == 2, 'the gradients of pointnet.embed.weight and .bias were compared'
