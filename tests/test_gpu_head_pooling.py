"""GPU: the three oldest kernel pairs of csrc/heads.hip -- anchor attention pooling (eap_anchor_attn_pool_*), the slot-masked point mean
(eap_slot_masked_mean_*), the masked point max (eap_masked_max_*) -- at every anchor and point edge of their mapping (16 lanes per point with
one idle lane at 60 anchors and none at 64, 16-point blocks and strides, clamped rows below 16 points, 1 to 8 slots), every output element
against float64 under its own bound (tests/head_pooling_common.py; tests/test_head_pooling_host.py shows the bounds pass the kernels' own
order of operations and fail a single wrong element), and the autograd wrappers at the anchor counts, slot counts and operand layouts the
entries do not take."""
import numpy as np
import pytest
import torch

import head_pooling_common as H

pytestmark = pytest.mark.gpu

GUARD = 64                               # elements of the sentinel on either side of an output
SENTINEL = 0x7FC5A5A5                    # as float32 a NaN: a kernel that reads its output before writing it shows, too
GRID = [(na, n) for na in H.NA_GRID for n in H.N_GRID]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


class Carved:
    """an output tensor inside a larger buffer: 16-byte aligned, GUARD elements of SENTINEL in front of and behind it"""

    def __init__(self, shape, dtype, dev):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.t = self.buf[GUARD:GUARD + self.numel].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.numel:] == SENTINEL).all())

    def bits(self):
        return self.buf[GUARD:GUARD + self.numel]


def _twice(run):
    """run() -> {name: Carved}, two times into fresh buffers: guard bands intact, results bit-identical -> {name: numpy}"""
    first, second = run(), run()
    torch.cuda.synchronize()
    for k in first:
        assert first[k].intact() and second[k].intact(), f'{k}: written outside the tensor'
        assert torch.equal(first[k].bits(), second[k].bits()), f'{k}: two runs differ'
        assert not bool((first[k].bits() == SENTINEL).any()), f'{k}: an element was not written'
    return {k: v.t.cpu().numpy() for k, v in first.items()}


def _to(dev, t):
    return {k: torch.from_numpy(v).to(dev) for k, v in t.items() if isinstance(v, np.ndarray)}


# ---- (a) the entries against float64 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('na,n', GRID)
def test_attention_pool_entries_against_float64(dev, na, n):
    """out, conf, dx, dlogits; randn logits at T = 1 and 3, logits in the hundreds, equal logits, a masked (-inf) anchor; c = 1 is the narrow
    contraction's own logit shape"""
    from vgtk import _hip
    figures, shown = {}, {}
    for c in H.C_GRID:
        for family in H.ATTN_FAMILIES:
            t = H.attn_inputs(c, n, na, family)
            d, T = _to(dev, t), float(t['T'])

            def run():
                o = dict(out=Carved((H.B, c, n), torch.float32, dev), conf=Carved((H.B, n, na), torch.float32, dev),
                         dx=Carved((H.B, c, n, na), torch.float32, dev), dlogits=Carved((H.B, n, na), torch.float32, dev))
                _hip.call('eap_anchor_attn_pool_fwd_f32', d['x'], H.B, c, n, na, T, d['x'], d['logits'], o['out'].t, o['conf'].t)
                _hip.call('eap_anchor_attn_pool_bwd_f32', d['x'], H.B, c, n, na, T, d['x'], d['logits'], d['g'], o['dx'].t, o['dlogits'].t)
                return o

            got = _twice(run)
            refs = H.attn_reference(t)
            for k, (ref, bound) in refs.items():
                figures[(c, family, k)] = H.worst_ratio(got[k], ref, bound)
            normal = refs['conf'][0] >= H.TINY             # (printed apart: below 2^-126 the figure is ref / 2^-126 wherever the device flushes)
            shown[family] = max(shown.get(family, 0.0), H.worst_ratio(got['conf'][normal], refs['conf'][0][normal], refs['conf'][1][normal]))
    print('error / bound, attention pool:', {k: round(max(v for kk, v in figures.items() if kk[2] == k), 3) for k in ('out', 'conf', 'dx', 'dlogits')},
          'conf >= 2^-126 by family:', {k: round(v, 3) for k, v in shown.items()})
    for k, v in figures.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize('na,n', GRID)
def test_slot_masked_mean_entries_against_float64(dev, na, n):
    """1, 3 and 8 slots; hard masks with an empty slot and a slot that is the single point n - 1, soft masks; inv_den a float32 tensor made by
    the test and widened by the reference"""
    from vgtk import _hip
    figures = {}
    for c in H.C_GRID:
        for ns in H.NS_GRID:
            for family in H.SLOT_FAMILIES:
                t = H.slot_inputs(c, n, na, ns, family)
                d = _to(dev, t)

                def run():
                    o = dict(fwd=Carved((H.B, ns, c, na), torch.float32, dev), bwd=Carved((H.B, c, n, na), torch.float32, dev))
                    _hip.call('eap_slot_masked_mean_fwd_f32', d['x'], H.B, ns, c, n, na, d['x'], d['mask'], d['inv_den'], o['fwd'].t)
                    _hip.call('eap_slot_masked_mean_bwd_f32', d['g'], H.B, ns, c, n, na, d['g'], d['mask'], d['inv_den'], o['bwd'].t)
                    return o

                got = _twice(run)
                for k, (ref, bound) in H.slot_reference(t).items():
                    figures[(c, ns, family, k)] = H.worst_ratio(got[k], ref, bound)
    print('error / bound, slot mean:', {k: round(max(v for kk, v in figures.items() if kk[3] == k), 3) for k in ('fwd', 'bwd')})
    for k, v in figures.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize('na,n', GRID)
def test_masked_max_entries_are_exact(dev, na, n):
    """value, arg and dx, exactly, against the rule `NaN first, else the maximum, at the lowest point`: hard and soft masks, a negative channel
    among non-members, one member, no member, planted ties inside a lane's chain and across lanes and waves, a member's exact 0.0 behind
    non-members, NaN at a member, a non-member, the first and the last point"""
    from vgtk import _hip
    for c in H.C_GRID:
        for family in H.MAX_FAMILIES:
            t = H.max_inputs(c, n, na, family)
            d = _to(dev, t)

            def run():
                o = dict(out=Carved((H.B, c, na), torch.float32, dev), arg=Carved((H.B, c, na), torch.int32, dev),
                         dx=Carved((H.B, c, n, na), torch.float32, dev))
                _hip.call('eap_masked_max_fwd_f32', d['x'], H.B, c, n, na, d['x'], d['mask'], o['out'].t, o['arg'].t)
                _hip.call('eap_masked_max_bwd_f32', d['g'], H.B, c, n, na, d['g'], o['arg'].t, d['mask'], o['dx'].t)
                return o

            got = _twice(run)
            ref = H.max_reference(t)
            assert H.same_values(got['out'], ref['out']), (c, family, 'value')
            assert np.array_equal(got['arg'], ref['arg']), (c, family, 'arg')
            assert H.same_values(got['dx'], ref['dx']), (c, family, 'dx')


# ---- (b) the wrappers ----------------------------------------------------------------------------------------------------------------------------

def _exprs(x, logits, mask_b, mask_s, T):
    """the three operations as torch expressions, on float64 copies the caller made"""
    conf = torch.softmax(logits * T, -1)
    pooled = (x * conf.unsqueeze(1)).sum(-1)
    mx = (x * mask_b.view(x.shape[0], 1, x.shape[2], 1)).max(2)[0]
    mean = torch.einsum('bcna,bsn->bsca', x, mask_s) / mask_s.sum(-1).clamp(min=1e-8)[:, :, None, None]
    return pooled, conf, mx, mean


@pytest.mark.parametrize('na,ns', [(1, 3), (3, 3), (4, 9)], ids=['1-anchor', '3-anchors', '9-slots'])
def test_wrappers_at_counts_the_entries_do_not_take(dev, na, ns):
    """anchor_attention_pool, masked_max and slot_masked_mean with autograd at 1 and 3 anchors, slot_masked_mean at 9 slots: the torch
    expressions, compared with the same expressions in float64: the max exactly; the others, float32 sums of at most n = 17 terms behind a
    softmax or a quotient (n + 6 roundings on n terms of at most the tensor's largest magnitude), to (n + 6) n u of that magnitude"""
    import vgtk.so3conv as sptk
    gen = torch.Generator().manual_seed(40 + na + ns)
    b, c, n, T = 2, 5, 17, 3.0
    x = torch.randn(b, c, n, na, generator=gen).to(dev).requires_grad_(True)
    logits = torch.randn(b, 1, n, na, generator=gen).to(dev).requires_grad_(True)
    member = (torch.rand(b, n, generator=gen) > 0.4).to(dev)
    member[:, 0] = True
    slots = torch.rand(b, ns, n, generator=gen).to(dev)
    probes = [torch.randn(s, generator=gen).to(dev) for s in ((b, c, n), (b, n, na), (b, c, na), (b, ns, c, na))]
    pooled, conf = sptk.anchor_attention_pool(x, logits, T)
    got = (pooled, conf, sptk.masked_max(x, member), sptk.slot_masked_mean(x, slots))
    xr, lr = x.detach().double().requires_grad_(True), logits.detach().double().requires_grad_(True)
    want = _exprs(xr, lr.squeeze(1), member.double(), slots.double(), T)
    assert torch.equal(got[2].double(), want[2])
    close = lambda a, w: float((a.double() - w).abs().max()) <= (n + 6) * n * H.U * float(w.abs().max())
    for a, w in zip(got, want):
        assert a.shape == w.shape and close(a.detach(), w.detach())
    gx, gl = torch.autograd.grad(sum((p * a).sum() for p, a in zip(probes, got)), [x, logits])
    wx, wl = torch.autograd.grad(sum((p.double() * w).sum() for p, w in zip(probes, want)), [xr, lr])
    assert close(gx, wx) and close(gl, wl)


def test_attention_head_with_a_single_anchor(dev):
    """InvPPOutBlockOurs(pooling_method='attention') at kanchor = 1, where the reference class runs: equal to the plain torch formulation of
    its own layers, outputs and gradients (tests/test_gpu_lists_and_modules.py does the same at 60 anchors, with these bars)"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    torch.manual_seed(14)
    params = {'dim_in': 24, 'mlp': [16, 12], 'fc': [12], 'k': 12, 'kanchor': 1, 'temperature': 3.0}
    head = sptk.InvPPOutBlockOurs(params, pooling_method='attention').to(dev)
    x = torch.randn(2, 24, 37, 1, device=dev, requires_grad=True)
    out, conf = head(zptk.SphericalPointCloud(None, x, None))
    xr = x.detach().clone().requires_grad_(True)
    h = xr
    for lid, lin in enumerate(head.linear):
        h = torch.relu(head.norm[lid](lin(h)))
    cref = torch.softmax(head.attention_layer(h) * 3.0, dim=-1)
    oref = (h * cref).sum(-1)
    assert out.shape == (2, 12, 37) and conf.shape == (2, 37, 1)
    rel = lambda a, w: float((a - w).abs().max()) / float(w.abs().max())
    assert rel(out.detach(), oref.detach()) < 2e-6 and torch.equal(conf.detach(), cref.squeeze(1).detach())
    g = torch.randn_like(out)
    names = ['x'] + [k for k, _ in head.named_parameters() if not k.startswith('attention_layer')]
    params_ = [p for k, p in head.named_parameters() if not k.startswith('attention_layer')]
    grads = torch.autograd.grad(out, [x] + params_, g, retain_graph=True)
    grefs = torch.autograd.grad(oref, [xr] + params_, g)
    top = max(float(w.abs().max()) for w in grefs)
    for k, a, w in zip(names, grads, grefs):
        assert float((a - w).abs().max()) < 2e-5 * max(float(w.abs().max()), 1e-2 * top), k
    # (one anchor: the confidence is the constant 1, the attention layer takes no gradient on either side)
    ga = torch.autograd.grad(out, list(head.attention_layer.parameters()), g, allow_unused=True)
    assert all(v is None or float(v.abs().max()) == 0.0 for v in ga)


def _offset_view(t):
    """a contiguous view of the same values that starts 4 bytes into its storage"""
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    store[1:] = t.reshape(-1)
    v = store[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _permuted_view(t):
    """a non-contiguous view of the same values: the storage holds the first two axes swapped"""
    v = t.transpose(0, 1).contiguous().transpose(0, 1)
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


@pytest.mark.parametrize('layout', [_offset_view, _permuted_view], ids=['offset_4_bytes', 'permuted'])
def test_wrappers_take_offset_and_permuted_operands(dev, layout):
    """x, the logits and the gradient handed to backward as a contiguous view 4 bytes into its storage and as a permuted view: torch.equal
    to the results from aligned contiguous copies, for the three operations, forward and backward"""
    import vgtk.so3conv as sptk
    gen = torch.Generator().manual_seed(77)
    b, c, n, na, ns = 2, 5, 17, 60, 3
    x0 = torch.randn(b, c, n, na, generator=gen).to(dev)
    l0 = torch.randn(b, n, na, generator=gen).to(dev)
    member = (torch.rand(b, n, generator=gen) > 0.4).to(dev)
    slots = torch.rand(b, ns, n, generator=gen).to(dev)
    probes = [torch.randn(s, generator=gen).to(dev) for s in ((b, c, n), (b, c, na), (b, ns, c, na))]
    res = []
    for lay in (lambda t: t.clone(), layout):
        x, logits = lay(x0).requires_grad_(True), lay(l0).requires_grad_(True)
        if lay is layout:
            assert x.data_ptr() % 16 == 4 or not x.is_contiguous()
        outs = (sptk.anchor_attention_pool(x, logits, 3.0)[0], sptk.masked_max(x, member), sptk.slot_masked_mean(x, slots))
        grads = []
        for o, p in zip(outs, probes):
            grads += [v for v in torch.autograd.grad(o, [x, logits], lay(p), allow_unused=True) if v is not None]
        res.append([o.detach() for o in outs] + grads)
    assert len(res[0]) == len(res[1]) == 3 + 4
    for a, w in zip(res[1], res[0]):
        assert torch.equal(a, w)
