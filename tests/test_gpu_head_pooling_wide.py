"""GPU: the wide twins of the three oldest head kernels (csrc/heads.hip at Q = 64: eap_anchor_attn_pool_wide_*, eap_slot_masked_mean_wide_*,
eap_masked_max_wide_*) at every anchor and point edge of their mapping (one wavefront per point: 15 quads where the narrow kernels also run,
17 quads just past them, 60 at the use_2d count, one idle lane at 252 and none at 256; blocks of 4 points, chains of 1 to 5 wave iterations;
1 to 8 slots), every output element against float64 under its own bound (tests/head_pooling_wide_common.py; tests/test_head_pooling_wide_host.py
shows the bounds pass the kernels' own order of operations and fail a single wrong element); the autograd wrappers at 240 anchors; and
InvPPOutBlock2DOurs against the reference class's own outputs and gradients (tests/golden/inv_head_2d.npz)."""
import numpy as np
import pytest
import torch

import head_pooling_wide_common as W
from test_gpu_head_pooling import Carved, _to, _twice, dev  # noqa: F401  (the guard-banded buffers and the two-run check of the narrow kernels' test)

pytestmark = pytest.mark.gpu

T = torch.from_numpy


# ---- (a) the entries against float64 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('na', W.NA_GRID)
def test_attention_pool_wide_entries_against_float64(dev, na):
    """out, conf, dx, dlogits; randn logits at T = 1 and 3, logits in the hundreds, equal logits, a masked (-inf) anchor"""
    from vgtk import _hip
    figures = {}
    for n in W.N_GRID:
        for c in W.C_GRID:
            for family in W.ATTN_FAMILIES:
                t = W.attn_inputs(c, n, na, family)
                d, temp = _to(dev, t), float(t['T'])

                def run():
                    o = dict(out=Carved((W.B, c, n), torch.float32, dev), conf=Carved((W.B, n, na), torch.float32, dev),
                             dx=Carved((W.B, c, n, na), torch.float32, dev), dlogits=Carved((W.B, n, na), torch.float32, dev))
                    _hip.call('eap_anchor_attn_pool_wide_fwd_f32', d['x'], W.B, c, n, na, temp, d['x'], d['logits'], o['out'].t, o['conf'].t)
                    _hip.call('eap_anchor_attn_pool_wide_bwd_f32', d['x'], W.B, c, n, na, temp, d['x'], d['logits'], d['g'], o['dx'].t, o['dlogits'].t)
                    return o

                got = _twice(run)
                for k, (ref, bound) in W.attn_reference(t).items():
                    figures[(n, c, family, k)] = W.worst_ratio(got[k], ref, bound)
    print('error / bound, wide attention pool:', {k: round(max(v for kk, v in figures.items() if kk[3] == k), 3) for k in ('out', 'conf', 'dx', 'dlogits')})
    for k, v in figures.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize('na', W.NA_GRID)
def test_slot_masked_mean_wide_entries_against_float64(dev, na):
    """1, 3 and 8 slots; hard masks with an empty slot and a slot that is the single point n - 1, soft masks; inv_den a float32 tensor made by
    the test and widened by the reference"""
    from vgtk import _hip
    figures = {}
    for n in W.N_GRID:
        for c in W.C_GRID:
            for ns in W.NS_GRID:
                for family in W.SLOT_FAMILIES:
                    t = W.slot_inputs(c, n, na, ns, family)
                    d = _to(dev, t)

                    def run():
                        o = dict(fwd=Carved((W.B, ns, c, na), torch.float32, dev), bwd=Carved((W.B, c, n, na), torch.float32, dev))
                        _hip.call('eap_slot_masked_mean_wide_fwd_f32', d['x'], W.B, ns, c, n, na, d['x'], d['mask'], d['inv_den'], o['fwd'].t)
                        _hip.call('eap_slot_masked_mean_wide_bwd_f32', d['g'], W.B, ns, c, n, na, d['g'], d['mask'], d['inv_den'], o['bwd'].t)
                        return o

                    got = _twice(run)
                    for k, (ref, bound) in W.slot_reference(t).items():
                        figures[(n, c, ns, family, k)] = W.worst_ratio(got[k], ref, bound)
    print('error / bound, wide slot mean:', {k: round(max(v for kk, v in figures.items() if kk[4] == k), 3) for k in ('fwd', 'bwd')})
    for k, v in figures.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize('na', W.NA_GRID)
def test_masked_max_wide_entries_are_exact(dev, na):
    """value, arg and dx, exactly, against the rule `NaN first, else the maximum, at the lowest point`: every family of the narrow kernels' test"""
    from vgtk import _hip
    for n in W.N_GRID:
        for c in W.C_GRID:
            for family in W.MAX_FAMILIES:
                t = W.max_inputs(c, n, na, family)
                d = _to(dev, t)

                def run():
                    o = dict(out=Carved((W.B, c, na), torch.float32, dev), arg=Carved((W.B, c, na), torch.int32, dev),
                             dx=Carved((W.B, c, n, na), torch.float32, dev))
                    _hip.call('eap_masked_max_wide_fwd_f32', d['x'], W.B, c, n, na, d['x'], d['mask'], o['out'].t, o['arg'].t)
                    _hip.call('eap_masked_max_wide_bwd_f32', d['g'], W.B, c, n, na, d['g'], o['arg'].t, d['mask'], o['dx'].t)
                    return o

                got = _twice(run)
                ref = W.max_reference(t)
                assert W.same_values(got['out'], ref['out']), (n, c, family, 'value')
                assert np.array_equal(got['arg'], ref['arg']), (n, c, family, 'arg')
                assert W.same_values(got['dx'], ref['dx']), (n, c, family, 'dx')


def test_at_60_anchors_the_wide_entries_repeat_the_narrow_ones(dev):
    """the overlap of the two domains (the parametrised tests above hold the wide entries at 60 anchors to float64): where the two kernels
    perform the same operations per element -- the masked max and its scatter, the slot mean's backward chain -- their results are bit-equal"""
    import head_pooling_common as H
    from vgtk import _hip
    c, n, na = 5, 17, 60
    t = H.max_inputs(c, n, na, 'ties')
    d = _to(dev, t)
    res = []
    for infix in ('', '_wide'):
        out, arg = torch.empty(H.B, c, na, device=dev), torch.empty(H.B, c, na, dtype=torch.int32, device=dev)
        dx = torch.empty(H.B, c, n, na, device=dev)
        _hip.call(f'eap_masked_max{infix}_fwd_f32', d['x'], H.B, c, n, na, d['x'], d['mask'], out, arg)
        _hip.call(f'eap_masked_max{infix}_bwd_f32', d['g'], H.B, c, n, na, d['g'], arg, d['mask'], dx)
        res.append((out, arg, dx))
    assert all(torch.equal(a, w) for a, w in zip(res[1], res[0]))
    t = H.slot_inputs(c, n, na, 3, 'soft')
    d = _to(dev, t)
    bwd = [torch.empty(H.B, c, n, na, device=dev) for _ in range(2)]
    for infix, o in zip(('', '_wide'), bwd):
        _hip.call(f'eap_slot_masked_mean{infix}_bwd_f32', d['g'], H.B, 3, c, n, na, d['g'], d['mask'], d['inv_den'], o)
    assert torch.equal(bwd[0], bwd[1])                      # the same chain of ns fused multiply-adds per element


# ---- (b) the wrappers at 240 anchors -------------------------------------------------------------------------------------------------------------

WIDE_ENTRIES = {f'eap_{op}_wide_{d}_f32' for op in ('anchor_attn_pool', 'slot_masked_mean', 'masked_max') for d in ('fwd', 'bwd')}


@pytest.fixture
def calls(monkeypatch):
    """the names vgtk.so3conv.heads hands to _hip.call while a test runs"""
    from vgtk import _hip
    real, seen = _hip.call, []

    def recording(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(_hip, 'call', recording)
    return seen


def test_wrappers_at_240_anchors_run_the_wide_entries(dev, calls):
    """anchor_attention_pool, masked_max and slot_masked_mean with autograd at 240 anchors against the torch expressions in float64, every
    element under the bound of the kernel that computes it (head_pooling_wide_common); the slot mean's denominator, made by the wrapper in
    float32 (a sum of n terms, a clamp, a reciprocal: n + 1 roundings), adds (n + 1) u of the value.  All six _wide entries must have been
    called: a wrapper that fell back to the torch expressions would pass the numbers and fail here."""
    import vgtk.so3conv as sptk
    c, n, na, ns = 5, 17, 240, 3
    ta, tm, ts = W.attn_inputs(c, n, na, 'randn_T3'), W.max_inputs(c, n, na, 'hard'), W.slot_inputs(c, n, na, ns, 'soft')
    temp = float(ta['T'])
    ok = lambda got, ref, bound: W.worst_ratio(got.detach().cpu().numpy(), ref.detach().cpu().numpy(), bound) <= 1.0

    # attention pooling, logits with a gradient
    x, logits, g = (T(ta[k]).to(dev) for k in ('x', 'logits', 'g'))
    x.requires_grad_(True), logits.requires_grad_(True)
    xr, lr = x.detach().double().requires_grad_(True), logits.detach().double().requires_grad_(True)
    cref = torch.softmax(lr * temp, -1)
    pref = (xr * cref.unsqueeze(1)).sum(-1)
    wx, wl = torch.autograd.grad(pref, [xr, lr], g.double(), retain_graph=True)
    bounds = {k: v[1] for k, v in W.attn_reference(ta).items()}
    pooled, conf = sptk.anchor_attention_pool(x, logits.unsqueeze(1), temp)
    assert pooled.shape == (W.B, c, n) and conf.shape == (W.B, n, na)
    assert ok(pooled, pref, bounds['out']) and ok(conf, cref, bounds['conf'])
    gx, gl = torch.autograd.grad(pooled, [x, logits], g, retain_graph=True)
    assert ok(gx, wx, bounds['dx']) and ok(gl, wl, bounds['dlogits'])
    assert conf.requires_grad, 'the confidence of logits that require a gradient must carry one'
    probe = torch.randn(conf.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    gc, = torch.autograd.grad(conf, [logits], probe)
    wc, = torch.autograd.grad(cref, [lr], probe.double())
    # (torch's own float32 softmax and its backward, not the kernels': sums of na terms, held to (na + 6) u of the largest element)
    assert float((gc.double() - wc).abs().max()) <= (na + 6) * W.U * float(wc.abs().max())
    # ... and without: the kernel's confidence, as data
    pooled2, conf2 = sptk.anchor_attention_pool(x, logits.detach(), temp)
    assert not conf2.requires_grad and torch.equal(pooled2, pooled) and ok(conf2, cref, bounds['conf'])

    # masked max: exact, the gradient at the member point that attains it
    x = T(tm['x']).to(dev).requires_grad_(True)
    member, g = T(tm['mask']).to(dev) > 0.5, T(tm['g']).to(dev)
    xr = x.detach().double().requires_grad_(True)
    want = (xr * member.double().view(W.B, 1, n, 1)).max(2)[0]
    got = sptk.masked_max(x, member)
    assert torch.equal(got.double(), want)
    assert torch.equal(torch.autograd.grad(got, [x], g)[0].double(), torch.autograd.grad(want, [xr], g.double())[0])

    # slot mean
    x = T(ts['x']).to(dev).requires_grad_(True)
    mask, g = T(ts['mask']).to(dev), T(ts['g']).to(dev)
    xr, mr = x.detach().double().requires_grad_(True), mask.double()
    want = torch.einsum('bcna,bsn->bsca', xr, mr) / mr.sum(-1).clamp(min=1e-8)[:, :, None, None]
    wx, = torch.autograd.grad(want, [xr], g.double(), retain_graph=True)
    refs = W.slot_reference(ts)
    got = sptk.slot_masked_mean(x, mask)
    gx, = torch.autograd.grad(got, [x], g)
    den = (n + 1) * W.U
    assert ok(got, want, refs['fwd'][1] + den * np.abs(refs['fwd'][0]))
    terms = refs['bwd'][1] / ((1 + ns) * W.U)              # sum_s |m g inv_den|: every term carries its own denominator
    assert ok(gx, wx, refs['bwd'][1] + den * terms)
    with pytest.raises(RuntimeError, match='treated as data'):
        sptk.slot_masked_mean(x, mask.clone().requires_grad_(True))

    assert WIDE_ENTRIES <= set(calls), sorted(WIDE_ENTRIES - set(calls))


# ---- (c) InvPPOutBlock2DOurs ---------------------------------------------------------------------------------------------------------------------

PARAMS = {'dim_in': 8, 'mlp': [6], 'fc': [6], 'k': 6, 'kanchor': 60, 'temperature': 3.0}
MODES = {'attention': ('attention', None), 'max': ('max', None), 'mean': ('mean', None), 'sel_mode': ('max', 17)}


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize('tag', list(MODES))
def test_invariant_head_2d_matches_reference_golden(dev, golden, calls, tag):
    """InvPPOutBlock2DOurs against the reference class (base_so3conv.py:L921-1008) run on CPU, at the bars of
    test_invariant_head_matches_reference_golden for the 60-anchor head: outputs in training and eval mode, anchor confidences,
    running-statistic updates, and for the attention and sel_mode variants every gradient."""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    g = golden('inv_head_2d.npz')
    pooling, sel = MODES[tag]
    assert sel is None or sel == int(g['sel_mode'])
    head = sptk.InvPPOutBlock2DOurs(PARAMS, norm=1, pooling_method=pooling, sel_mode=sel)
    pre = f'{tag}_state_'
    state = {k[len(pre):]: T(v) for k, v in g.items() if k.startswith(pre)}
    assert set(state) == set(head.state_dict()), 'state_dict names differ from the reference class'
    head = head.to(dev)
    for phase in ('train', 'eval'):
        head.load_state_dict(state)
        head.train(phase == 'train')
        x = T(g['x']).to(dev).requires_grad_(True)
        res = head(zptk.SphericalPointCloud(None, x, None))
        assert isinstance(res, tuple) == (tag == 'attention')
        y = res[0] if tag == 'attention' else res
        assert rel_err(y.detach().cpu().numpy(), g[f'{tag}_{phase}_out']) < 5e-6
        if tag == 'attention':
            assert rel_err(res[1].detach().cpu().numpy(), g[f'{tag}_{phase}_conf']) < 5e-6
        if tag in ('attention', 'sel_mode'):
            names = [n for n, _ in head.named_parameters()]
            grads = torch.autograd.grad(y, [x] + list(head.parameters()), T(g[f'{tag}_{phase}_grad_out']).to(dev))
            top = max(float(np.abs(g[f'{tag}_{phase}_grad_{n}']).max()) for n in names)
            for n, got in zip(['x'] + names, grads):
                want = g[f'{tag}_{phase}_grad_{n}']
                # (the floor: a conv bias in front of a training-mode BatchNorm has an exactly-zero gradient, rounding noise on both sides)
                scale = max(float(np.abs(want).max()), 5e-2 * top)
                assert float(np.abs(got.cpu().numpy() - want).max()) < 5e-5 * scale, (phase, n)
        if phase == 'train':
            for k, v in head.state_dict().items():
                if 'running' in k:
                    assert rel_err(v.cpu().numpy(), g[f'{tag}_after_{k}']) < 1e-5, k
    if tag == 'attention':
        assert {'eap_anchor_attn_pool_wide_fwd_f32', 'eap_anchor_attn_pool_wide_bwd_f32'} <= set(calls)
    if tag == 'sel_mode':                                   # the gathered [B,C,N,4] tensor: the narrow kernel at na = 4
        assert {'eap_anchor_attn_pool_fwd_f32', 'eap_anchor_attn_pool_bwd_f32'} <= set(calls)


def test_the_1d_head_on_a_240_anchor_map_is_the_2d_head(dev, golden):
    """InvPPOutBlockOurs(pooling_method='attention') on the fixture's [2,8,7,240] map and InvPPOutBlock2DOurs('attention') with the same state
    differ by a view and share every kernel: pooled tensor and confidence bit-equal, training and eval mode"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    g = golden('inv_head_2d.npz')
    pre = 'attention_state_'
    state = {k[len(pre):]: T(v) for k, v in g.items() if k.startswith(pre)}
    heads = [cls(PARAMS, norm=1, pooling_method='attention').to(dev) for cls in (sptk.InvPPOutBlockOurs, sptk.InvPPOutBlock2DOurs)]
    for phase in ('train', 'eval'):
        res = []
        for head in heads:
            head.load_state_dict(state)
            head.train(phase == 'train')
            res.append(head(zptk.SphericalPointCloud(None, T(g['x']).to(dev), None)))
        assert res[0][0].shape == (2, 6, 7) and res[0][1].shape == (2, 7, 240)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), phase
