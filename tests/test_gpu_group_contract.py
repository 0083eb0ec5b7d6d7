"""GPU: the regimes that group and contract (vgtk.so3conv.functional: a grouping pair inside _group_contract / _backward_textbook) -- the
list kernels with a 'textbook dX' backward, the 'anchor map', the 'residual map', the float64 inter and intra convs.  Every case has b = 3
clouds, so that X_CHUNK_CLOUDS = 2 leaves an uneven last slab, fixed seeds, and otherwise the smallest inputs that reach its kernels.

Per case:
  1. the node IS the composition group -> W X, dW = sum_b dY_b X_b^T, dF = group^T(W^T dY), written here from the vgtk._hip wrappers over
     the whole batch: torch.equal, no tolerance (float32: W^T written out; float64: the view) -- wherever X is in the reference layout.
     The list regime at c = 16 keeps X transposed, its scratch form with store-order columns: no independent composition; there two runs
     agree bit for bit and the node agrees with the float64 node on the same inputs widened at the bars of
     test_gpu_so3_f64.py::test_float64_layer_checks_the_float32_layer (out and dF 1e-5, dW 2e-5 of scale);
  2. a kept X and a regrouped X give the same dW and dF, bit for bit, where the regime has both: the list regime under BACKWARD_MODE
     'auto' (its first backward finds 'textbook dX' with X not kept and sets the hint, the second forward keeps X).  The map regimes keep X
     whenever dW is wanted and the float64 nodes never do: one form each, held by 1;
  3. the launch list (vgtk._hip.call wrapped): a backward that wants dF alone, X not kept, launches no forward grouping; one that wants
     dW alone launches no transposed grouping."""
import copy

import pytest
import torch

import so3_f64_cases as S
from test_gpu_so3_f64 import layer_pair, small_inter_node

pytestmark = pytest.mark.gpu

B, P, NN, RADIUS, SIGMA = 3, 24, 4, 0.4, 0.05          # (a radius at which a fifth of the lists are repeat-padded)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def grouped_fwd(names):
    return [n for n in names if '_group_fwd' in n or '_group2d_fwd' in n]


def grouped_bwd(names):
    return [n for n in names if '_group_bwd' in n or '_group2d_bwd' in n]


def run(conv, cloud, feats, gy, monkeypatch, need_f=True, need_w=True, grad=True):
    """forward (+ backward) of a module with _hip.call and _group_contract wrapped -> dict(out, dF, dW, fwd / bwd: the entries launched,
    grouping: the pair the forward was built around, logs)"""
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    names, seen = [], []
    real_call, real_loop = _hip.call, L._group_contract
    W = conv.basic_conv.W
    f = feats.detach().clone().requires_grad_(need_f)
    res = {}
    with monkeypatch.context() as m:
        m.setattr(_hip, 'call', lambda name, *a, **k: (names.append(name), real_call(name, *a, **k))[1])
        m.setattr(L, '_group_contract', lambda grouping, *a: (seen.append(grouping), real_loop(grouping, *a))[1])
        m.setattr(L, 'FORWARD_LOG', [])
        m.setattr(L, 'BACKWARD_LOG', [])
        W.requires_grad_(need_w)
        try:
            with torch.enable_grad() if grad else torch.no_grad():
                out = conv(cloud(f))
            y = out.feats if not isinstance(out, tuple) else out[3].feats
            res['fwd'], mark = list(names), len(names)
            if grad:
                wanted = [t for t, need in ((f, need_f), (W, need_w)) if need]
                grads = dict(zip([k for k, need in (('dF', need_f), ('dW', need_w)) if need], torch.autograd.grad(y, wanted, gy)))
                res.update(grads)
            torch.cuda.synchronize()
            res['bwd'] = names[mark:]
            res['logs'] = (list(L.FORWARD_LOG), list(L.BACKWARD_LOG))
        finally:
            W.requires_grad_(True)
    assert len(seen) == 1, 'one group-and-contract forward per layer'
    res['out'], res['grouping'] = y.detach(), seen[0]
    assert all(float(res[k].abs().max()) > 0 for k in ('out', 'dF', 'dW') if k in res), 'a result that is all zeros checks nothing'
    return res


def compose(group, group_t, feats, W, gy, mid):
    """the reference composition over the whole batch, from the vgtk._hip wrappers"""
    from vgtk import _hip
    b, c, n, a = feats.shape
    o, p = W.shape[0], gy.shape[2]
    x = group(feats)
    assert tuple(x.shape) == (b, c, mid, p, a)
    y = torch.empty(b, o, p * a, dtype=feats.dtype, device=feats.device)
    _hip.matmul(W, x.view(b, c * mid, p * a), y)
    dW = torch.empty_like(W)
    _hip.matmul_reduce(gy.view(b, o, p * a), x.view(b, c * mid, p * a).transpose(1, 2), dW)
    gx = torch.empty(b, c * mid, p * a, dtype=feats.dtype, device=feats.device)
    _hip.matmul(W.t() if feats.dtype == torch.float64 else W.t().contiguous(), gy.view(b, o, p * a), gx)
    dF = group_t(gx.view(b, c, mid, p, a), n)
    torch.cuda.synchronize()
    return {'out': y.view(b, o, p, a), 'dW': dW, 'dF': dF}


def composition_of(g):
    """(group, group_t) of a pair's regime from the wrappers and the pair's data tensors"""
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    if isinstance(g, L._F64Args):
        return (lambda f: _hip.so3_inter_group_fwd_f64(f, g.idx, g.g, g.r, g.rk, g.mult, g.sigma),
                lambda gx, n: _hip.so3_inter_group_bwd_f64(gx, g.inverse_lists(n), g.g, g.r, g.rk, g.multinv, g.sigma, n, g.idx.shape[2]))
    if isinstance(g, L._IntraGrouping):
        return (lambda f: _hip.so3_intra_group_fwd_f64(f, g.idx32), lambda gx, n: _hip.so3_intra_group_bwd_f64(gx, g.idx32))
    a = g.a
    if a.shift is not None:
        return (lambda f: _hip.so3_inter_group_fwd_res(f, a.idx, a.gx, a.rk, a.shift, a.sigma),
                lambda gx, n: _hip.so3_inter_group_bwd_res(gx, a.idx, a.gx, a.rk, a.shift, a.sigma, n))
    if a.amap is not None:
        return (lambda f: _hip.so3_inter_group_fwd_map(f, a.idx, a.gx, a.rk, a.amap, a.sigma),
                lambda gx, n: _hip.so3_inter_group_bwd_map(gx, a.idx, a.gx, a.rk, a.amap, a.sigma, n))
    return (lambda f: _hip.so3_inter_group_fwd(f, a.idx, a.gx, a.rk, a.mult, a.sigma, a.nonident),
            lambda gx, n: _hip.so3_inter_group_bwd(gx, a.idx, a.gx, a.rk, a.mult, a.sigma, n, a.ident))


def equal_to_the_composition(what, got, g, feats, W, gy):
    want = compose(*composition_of(g), feats, W.detach(), gy, g.mid)
    same = {k: torch.equal(got[k], want[k]) for k in ('out', 'dF', 'dW') if k in got}
    print(f'{what}: bit-equal to group -> W X / dY X^T / group^T(W^T dY):', same)
    assert same and all(same.values()), (what, same)


def posed_inputs(c, o, p, a, seed, dev, dtype=torch.float32):
    """b = 3 clouds of p points with one random rotation per point"""
    gen = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, 3, p, generator=gen, dtype=torch.float64)
    pose = torch.eye(4, dtype=torch.float64).repeat(B, p, 1, 1)
    pose[:, :, :3, :3] = S.rand_rot(gen, B, p)
    feats = torch.randn(B, c, p, a, generator=gen, dtype=torch.float64)
    gy = torch.randn(B, o, p, a, generator=gen, dtype=torch.float64)
    return tuple(t.to(dtype).to(dev) for t in (xyz, pose, feats, gy))


def posed_cloud(xyz, pose):
    import vgtk.spconv as zptk
    return lambda f: zptk.SphericalPointCloudPose(xyz, f, None, pose)


def launch_list_holds(what, conv, cloud, feats, gy, monkeypatch):
    """3. of the header; the forwards here do not keep X: nobody wants dW, or the regime never keeps it"""
    only_f = run(conv, cloud, feats, gy, monkeypatch, need_w=False)
    only_w = run(conv, cloud, feats, gy, monkeypatch, need_f=False)
    print(f'{what}: dF alone launches {only_f["bwd"]}\n{what}: dW alone launches {only_w["bwd"]}')
    assert grouped_bwd(only_f['bwd']) and not grouped_fwd(only_f['bwd'])
    assert not grouped_bwd(only_w['bwd']) and only_w['dW'] is not None
    return only_f, only_w


# ---- 'textbook dX' on the list kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', [2, 16])
def test_list_kernels_with_a_textbook_backward(dev, monkeypatch, c):
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    o = 8
    xyz, pose, feats, gy = posed_inputs(c, o, P, 60, 100 + c, dev)
    torch.manual_seed(200 + c)
    conv = sptk.InterSO3PoseConv(c, o, 1, 1, RADIUS, SIGMA, NN, kanchor=60, permute_modes=1).to(dev)
    assert conv.kernels.shape[0] == 24
    cloud = posed_cloud(xyz, pose)
    monkeypatch.setattr(L, 'BACKWARD_MODE', 'dx')
    monkeypatch.setattr(L, 'X_CHUNK_CLOUDS', 2)
    got = run(conv, cloud, feats, gy, monkeypatch)
    g = got['grouping']
    print(f'c = {c}: layout {g.layout}, forward {got["fwd"]}, backward {got["bwd"]}, regimes {[e["regime"] for e in got["logs"][1]]}')
    assert isinstance(g, L._ListGrouping) and g.a.mult is not None and int(g.a.nonident.min()) == 1        # the poses permute every cloud
    assert [e['regime'] for e in got['logs'][1]] == ['textbook dX']
    assert g.layout == (0 if c == 2 else 2)
    assert len(grouped_fwd(got['fwd'])) == 1 and not grouped_fwd(got['bwd'])                               # 'dx': X kept, one slab
    scratch = run(conv, cloud, feats, gy, monkeypatch, grad=False)                                         # X scratch: slabs of 2 + 1 clouds
    assert len(grouped_fwd(scratch['fwd'])) == 2
    if c == 2:
        equal_to_the_composition('list kernels, c = 2', got, g, feats, conv.basic_conv.W, gy)
        assert torch.equal(scratch['out'], got['out'])
    else:
        again = run(conv, cloud, feats, gy, monkeypatch)
        assert all(torch.equal(got[k], again[k]) for k in ('out', 'dF', 'dW'))
        conv64 = copy.deepcopy(conv).double()
        ref = run(conv64, posed_cloud(xyz.double(), pose.double()), feats.double(), gy.double(), monkeypatch)
        assert [e['regime'] for e in ref['logs'][1]] == ['float64']
        for k, bar in (('out', 1e-5), ('dF', 1e-5), ('dW', 2e-5)):
            S.check(got[k], ref[k], f'list kernels, c = 16, against the float64 node, {k}', bar)
            if k == 'out':
                S.check(scratch['out'], ref['out'], 'list kernels, c = 16, X as scratch with store-order columns, out', bar)
    # 2. kept and regrouped X: under 'auto' the first backward finds X not kept and regroups it, the second forward keeps it
    monkeypatch.setattr(L, 'BACKWARD_MODE', 'auto')
    monkeypatch.setattr(L, 'DENSE_MODE', 'off')
    monkeypatch.setattr(L, '_KEEP_X_HINT', {})
    first = run(conv, cloud, feats, gy, monkeypatch)
    second = run(conv, cloud, feats, gy, monkeypatch)
    print(f'c = {c}, auto: first backward {first["bwd"]}, second {second["bwd"]}')
    assert [e['regime'] for e in first['logs'][1] + second['logs'][1]] == ['textbook dX', 'textbook dX']
    assert len(grouped_fwd(first['fwd'])) == 2 and len(grouped_fwd(first['bwd'])) == 1                     # regrouped, whole batch
    assert len(grouped_fwd(second['fwd'])) == 1 and not grouped_fwd(second['bwd'])                         # kept
    assert torch.equal(first['dW'], second['dW']) and torch.equal(first['dF'], second['dF'])
    assert torch.equal(first['dW'], got['dW']) and torch.equal(first['dF'], got['dF'])
    # 3. the launch list; dF alone with X not kept (no hint yet) is the grouping launch the shared backward no longer makes
    monkeypatch.setattr(L, '_KEEP_X_HINT', {})
    only_f, only_w = launch_list_holds(f'list kernels, c = {c}', conv, cloud, feats, gy, monkeypatch)
    assert [e['regime'] for e in only_f['logs'][1]] == ['textbook dX'] and len(grouped_fwd(only_f['fwd'])) == 2
    assert torch.equal(only_f['dF'], got['dF']) and torch.equal(only_w['dW'], got['dW'])


# ---- the per-entry maps ---------------------------------------------------------------------------------------------------------------

def test_anchor_map(dev, monkeypatch):
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    c, o, na = 4, 4, 20
    xyz, pose, feats, gy = posed_inputs(c, o, P, na, 300, dev)
    torch.manual_seed(301)
    conv = sptk.InterSO3PoseConv(c, o, 1, 1, RADIUS, SIGMA, NN, kanchor=na, permute_modes=1).to(dev)
    cloud = posed_cloud(xyz, pose)
    monkeypatch.setattr(L, 'X_CHUNK_CLOUDS', 2)
    got = run(conv, cloud, feats, gy, monkeypatch)
    g = got['grouping']
    assert isinstance(g, L._MapGrouping) and ([e['regime'] for e in got['logs'][0]], [e['regime'] for e in got['logs'][1]]) == (['anchor map'],) * 2
    # the map is non-trivial, and many-to-one: some entry's map is no permutation of the anchors
    amap = g.a.amap.long()
    distinct = (torch.nn.functional.one_hot(amap, na).sum(-2) > 0).sum(-1)
    assert bool((amap != torch.arange(na, device=dev)).any()) and int(distinct.min()) < na
    equal_to_the_composition('anchor map', got, g, feats, conv.basic_conv.W, gy)
    scratch = run(conv, cloud, feats, gy, monkeypatch, grad=False)
    assert len(grouped_fwd(scratch['fwd'])) == 2 and len(grouped_fwd(got['fwd'])) == 1 and torch.equal(scratch['out'], got['out'])
    only_f, only_w = launch_list_holds('anchor map', conv, cloud, feats, gy, monkeypatch)
    assert len(grouped_fwd(only_f['fwd'])) == 2                                                            # dF alone: X was scratch
    assert torch.equal(only_f['dF'], got['dF']) and torch.equal(only_w['dW'], got['dW'])


def test_residual_map(dev, monkeypatch):
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    c, o = 2, 4
    p = L.KERNEL_2D_MIN_POINTS                                                                             # the smallest cloud the kernels take
    xyz, pose, feats, gy = posed_inputs(c, o, p, 240, 400, dev)
    torch.manual_seed(401)
    conv = sptk.InterSO3PoseConv(c, o, 1, 1, 0.3, SIGMA, NN, kanchor=60, permute_modes=1, use_2d=True).to(dev)
    cloud = posed_cloud(xyz, pose)
    monkeypatch.setattr(L, 'X_CHUNK_CLOUDS', 2)
    got = run(conv, cloud, feats, gy, monkeypatch)
    g = got['grouping']
    assert [e['regime'] for e in got['logs'][0]] == ['residual map'] and [e['regime'] for e in got['logs'][1]] == ['residual map']
    assert isinstance(g, L._MapGrouping) and g.a.shift is not None
    equal_to_the_composition('residual map', got, g, feats, conv.basic_conv.W, gy)
    scratch = run(conv, cloud, feats, gy, monkeypatch, grad=False)
    assert len(grouped_fwd(scratch['fwd'])) == 2 and len(grouped_fwd(got['fwd'])) == 1 and torch.equal(scratch['out'], got['out'])
    only_f, only_w = launch_list_holds('residual map', conv, cloud, feats, gy, monkeypatch)
    assert torch.equal(only_f['dF'], got['dF']) and torch.equal(only_w['dW'], got['dW'])


# ---- the float64 nodes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['inter', 'intra'])
def test_float64_nodes(dev, monkeypatch, which):
    import vgtk.so3conv.functional as L
    layers, feats, gy = layer_pair(dev)
    conv, cloud = layers[0 if which == 'inter' else 1]
    feats, gy = feats.to(dev), gy.to(dev)
    one_cloud = 8 * conv.basic_conv.W.shape[1] * feats.shape[2] * 60
    monkeypatch.setattr(L, 'F64_X_BYTES_MAX', 2 * one_cloud)                                               # slabs of 2 + 1 clouds
    assert L._f64_slabs(B, one_cloud) == [(0, 2), (2, 3)] and feats.shape[0] == B
    got = run(conv, cloud, feats, gy, monkeypatch)
    g = got['grouping']
    assert isinstance(g, L._F64Args if which == 'inter' else L._IntraGrouping) and got['out'].dtype == torch.float64
    print(f'float64 {which}: forward {got["fwd"]}, backward {got["bwd"]}')
    assert len(grouped_fwd(got['fwd'])) == 2 and len(grouped_fwd(got['bwd'])) == 2 and len(grouped_bwd(got['bwd'])) == 2      # X never kept
    equal_to_the_composition(f'float64 {which}', got, g, feats, conv.basic_conv.W, gy)
    only_f, only_w = launch_list_holds(f'float64 {which}', conv, cloud, feats, gy, monkeypatch)
    assert torch.equal(only_f['dF'], got['dF']) and torch.equal(only_w['dW'], got['dW'])


def test_float64_node_applied_directly(dev, monkeypatch):
    """the node of test_gpu_so3_f64.py::test_gradcheck_inter_node (one cloud) against the composition over its own pair"""
    import vgtk.so3conv.functional as L
    args, feats, W = small_inter_node(dev)
    gen = torch.Generator().manual_seed(17)
    y = L._GroupContractF64.apply(feats, W, args)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64).to(dev)
    dF, dW = torch.autograd.grad(y, [feats, W], gy)
    equal_to_the_composition('float64 inter node, one cloud', {'out': y.detach(), 'dF': dF, 'dW': dW}, args, feats.detach(), W, gy)
