"""CPU: the wide twins of the three oldest head kernels (csrc/heads.hip at Q = 64: anchor rows of up to 256 floats, one wavefront per point) and
InvPPOutBlock2DOurs as far as they go without a device: the six C-ABI entries on calls that return before they launch (arity, empty batch,
anchor and slot counts, 16-byte alignment), the predicate and the fallbacks of the wrappers past the kernels' domain, the per-element bounds
that tests/test_gpu_head_pooling_wide.py holds the kernels to (tests/head_pooling_wide_common.py): a float32 emulation of each kernel in
the kernel's own summation order must pass them, a result that is wrong by one element must fail them; and the head's names and refusals."""
import numpy as np
import pytest
import torch

import head_pooling_wide_common as W

INVALID_VALUE = 1           # hipErrorInvalidValue

# name -> (integer dimensions in order, takes the temperature, pointer parameters in order, those moved by 16-byte words)
ENTRIES = {
    'eap_anchor_attn_pool_wide_fwd_f32': (('b', 'c', 'n', 'na'), True, ('x', 'logits', 'out', 'conf'), ('x', 'logits', 'conf')),
    'eap_anchor_attn_pool_wide_bwd_f32': (('b', 'c', 'n', 'na'), True, ('x', 'logits', 'g', 'dx', 'dlogits'), ('x', 'logits', 'dx', 'dlogits')),
    'eap_slot_masked_mean_wide_fwd_f32': (('b', 'ns', 'c', 'n', 'na'), False, ('x', 'mask', 'inv_den', 'out'), ('x', 'out')),
    'eap_slot_masked_mean_wide_bwd_f32': (('b', 'ns', 'c', 'n', 'na'), False, ('g', 'mask', 'inv_den', 'dx'), ('g', 'dx')),
    'eap_masked_max_wide_fwd_f32': (('b', 'c', 'n', 'na'), False, ('x', 'mask', 'out', 'arg'), ('x', 'out', 'arg')),
    'eap_masked_max_wide_bwd_f32': (('b', 'c', 'n', 'na'), False, ('g', 'arg', 'mask', 'dx'), ('g', 'arg', 'dx')),
}
ARITY = {'eap_anchor_attn_pool_wide_fwd_f32': 10, 'eap_anchor_attn_pool_wide_bwd_f32': 11, 'eap_slot_masked_mean_wide_fwd_f32': 10,
         'eap_slot_masked_mean_wide_bwd_f32': 10, 'eap_masked_max_wide_fwd_f32': 9, 'eap_masked_max_wide_bwd_f32': 9}


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def _args(name, pointers=None, **dims):
    """the entry's argument tuple: dimensions (b = 3, ns = 2, c = 8, n = 40, na = 240 unless given), temperature, pointers (null unless
    given: {parameter: address}), null stream"""
    ints, temp, ptrs, _ = ENTRIES[name]
    size = dict(b=3, ns=2, c=8, n=40, na=240)
    size.update(dims)
    return tuple(size[k] for k in ints) + ((3.0,) if temp else ()) + tuple((pointers or {}).get(p) for p in ptrs) + (None,)


def _short(name):
    return name[len('eap_'):-len('_f32')]


def test_the_six_entries_have_the_headers_arity_and_their_narrow_twins_parameters(hip):
    for name, count in ARITY.items():
        twin = getattr(hip.abi, name.replace('_wide', ''))
        assert len(getattr(hip.abi, name).argtypes) == count == len(_args(name)), name
        assert list(getattr(hip.abi, name).argtypes) == list(twin.argtypes), name


def test_an_empty_batch_returns_before_a_pointer_is_touched(hip):
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, b=0)) == 0, name
        assert getattr(hip.abi, name)(*_args(name, c=0)) == 0, name
        assert getattr(hip.abi, name)(*_args(name, b=0, na=6)) == 0, name


@pytest.mark.parametrize('na', [0, 6, 260])
def test_an_anchor_count_outside_the_domain_is_refused(hip, na):
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, na=na)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert _short(name) in msg and 'multiple of 4, at most 256' in msg, msg


def test_more_than_8_slots_are_refused(hip):
    for name in ('eap_slot_masked_mean_wide_fwd_f32', 'eap_slot_masked_mean_wide_bwd_f32'):
        assert getattr(hip.abi, name)(*_args(name, ns=9)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert _short(name) in msg and 'at most 8 slots' in msg, msg
        assert getattr(hip.abi, name)(*_args(name, ns=0, na=6)) == 0, name          # no slot: nothing to do


def test_a_16_byte_operand_off_its_boundary_is_refused(hip):
    """every operand a kernel moves by float4 / int4, one at a time at 0x...4, 0x...8 and 0x...c, the other pointers of the call aligned and
    non-null: refused with the alignment message before anything is launched (the addresses are not memory)"""
    for name, (_, _, ptrs, wide) in ENTRIES.items():
        base = {p: 0x10000 * (i + 1) for i, p in enumerate(ptrs)}
        for p in wide:
            for off in (4, 8, 12):
                assert getattr(hip.abi, name)(*_args(name, dict(base, **{p: base[p] + off}))) == INVALID_VALUE, (name, p, off)
                msg = hip.abi.eap_last_error().decode()
                assert _short(name) in msg and 'must be 16-byte aligned' in msg, (name, p, msg)


# ---- the wrappers' routing ------------------------------------------------------------------------------------------------------------------

class _AsDevice(torch.Tensor):
    """a host tensor that answers is_cuda = True: the wrappers' device check passes and the torch expressions of the fallback run here"""
    is_cuda = property(lambda self: True)


def _as_device(t):
    return t.as_subclass(_AsDevice)


@pytest.fixture
def no_library(monkeypatch):
    from vgtk import _hip

    def refuse(name, *a, **k):
        raise AssertionError(f'{name}: the fallback must not reach the library')
    monkeypatch.setattr(_hip, 'call', refuse)


def test_the_predicate_of_the_wide_kernels():
    import vgtk.so3conv.heads as heads
    assert all(heads._anchor_rows_wide(na) for na in (68, 120, 240, 256))
    assert not any(heads._anchor_rows_wide(na) for na in (0, 60, 64, 66, 258, 260))
    assert not any(heads._anchor_rows_wide(na) and heads._anchor_rows_vectorise(na) for na in range(-4, 300))


def test_258_anchors_take_the_torch_expressions(no_library):
    import vgtk.so3conv as sptk
    gen = torch.Generator().manual_seed(258)
    b, c, n, na, ns = 2, 3, 5, 258, 2
    x = torch.randn(b, c, n, na, generator=gen)
    logits = torch.randn(b, 1, n, na, generator=gen)
    out, conf = sptk.anchor_attention_pool(_as_device(x), _as_device(logits), 3.0)
    cref = torch.softmax(logits.squeeze(1) * 3.0, -1)
    assert torch.equal(torch.Tensor(conf), cref) and torch.equal(torch.Tensor(out), (x * cref.unsqueeze(1)).sum(-1))
    member = torch.rand(b, n, generator=gen) > 0.4
    got = sptk.masked_max(_as_device(x), _as_device(member))
    assert torch.equal(torch.Tensor(got), (x * member.float().view(b, 1, n, 1)).max(2)[0])
    mask = torch.rand(b, ns, n, generator=gen)
    got = sptk.slot_masked_mean(_as_device(x), _as_device(mask))
    assert torch.equal(torch.Tensor(got), torch.einsum('bcna,bsn->bsca', x, mask) / mask.sum(-1).clamp(min=1e-8)[:, :, None, None])


def test_nine_slots_at_240_anchors_take_the_einsum(no_library):
    import vgtk.so3conv as sptk
    gen = torch.Generator().manual_seed(9)
    x, mask = torch.randn(2, 3, 5, 240, generator=gen), torch.rand(2, 9, 5, generator=gen)
    got = sptk.slot_masked_mean(_as_device(x), _as_device(mask))
    assert torch.equal(torch.Tensor(got), torch.einsum('bcna,bsn->bsca', x, mask) / mask.sum(-1).clamp(min=1e-8)[:, :, None, None])


def test_240_anchors_do_reach_the_wide_entries(monkeypatch):
    """the other side of the predicate: every wrapper names its _wide entry at 240 anchors (here to a stand-in that records and stops)"""
    import vgtk.so3conv as sptk
    from vgtk import _hip

    class Reached(Exception):
        pass

    def record(name, *a, **k):
        raise Reached(name)
    monkeypatch.setattr(_hip, 'call', record)
    x = _as_device(torch.randn(2, 3, 5, 240))
    for entry, run in (('eap_anchor_attn_pool_wide_fwd_f32', lambda: sptk.anchor_attention_pool(x, _as_device(torch.randn(2, 5, 240)), 3.0)),
                       ('eap_masked_max_wide_fwd_f32', lambda: sptk.masked_max(x, _as_device(torch.ones(2, 5)))),
                       ('eap_slot_masked_mean_wide_fwd_f32', lambda: sptk.slot_masked_mean(x, _as_device(torch.rand(2, 8, 5))))):
        with pytest.raises(Reached, match=entry):
            run()


# ---- the bounds: the emulation passes them, a wrong element fails them --------------------------------------------------------------------------

GRID = [(na, n) for na in W.NA_GRID for n in W.N_GRID]


def _last_off_by_one(a):
    a = np.array(a, order='C')
    a.reshape(-1)[-1] += np.float32(1.0)
    return a


def attn_ratios(c, n, na, family):
    """error / bound of the emulation per output, and of every mutation the family can show: {'emulation': {...}, mutation: {...}}"""
    t = W.attn_inputs(c, n, na, family)
    ref = W.attn_reference(t)
    res = {'emulation': {k: W.worst_ratio(v, *ref[k]) for k, v in W.attn_emulate(t).items()}}
    if family != 'equal_T3':
        # (a softmax does not see a shift of all its logits: with every logit of a point equal, any other such point gives the same confidence)
        nxt = np.roll(t['logits'].reshape(W.B * n, na), -1, axis=0).reshape(W.B, n, na)          # point p reads the logits of p + 1
        res['next_points_logits'] = {k: W.worst_ratio(v, *ref[k]) for k, v in W.attn_emulate(t, logits=nxt).items()}
    last = W.attn_emulate(t)
    last['out'][:, :, n - 1], last['conf'][:, n - 1], last['dx'][:, :, n - 1], last['dlogits'][:, n - 1] = 0.0, 0.0, 0.0, 0.0
    res['drop_last_point'] = {k: W.worst_ratio(v, *ref[k]) for k, v in last.items()}
    one = W.attn_emulate(t)                                                                          # the last element of every output off by 1
    one = {k: _last_off_by_one(v) for k, v in one.items()}
    res['one_element'] = {k: W.worst_ratio(v, *ref[k]) for k, v in one.items()}
    return res


def slot_ratios(c, n, na, ns, family):
    t = W.slot_inputs(c, n, na, ns, family)
    ref = W.slot_reference(t)
    ratios = lambda got: {k: W.worst_ratio(got[k], *ref[k]) for k in ('fwd', 'bwd')}
    res = {'emulation': ratios(W.slot_emulate(t))}
    dropped = W.slot_emulate(t, n_points=n - 1)
    dropped['bwd'][:, :, n - 1] = 0.0
    res['drop_last_point'] = ratios(dropped)
    if n > 1:                                          # with one point there is no other point to take the mask of
        res['shift_mask'] = ratios(W.slot_emulate(t, mask=np.roll(t['mask'], 1, axis=2)))
    if family == 'soft':                               # (two clouds' hard masks can hold equally many points)
        res['next_clouds_inv_den'] = ratios(W.slot_emulate(t, inv_den=np.roll(t['inv_den'], -1, axis=0)))
    one = W.slot_emulate(t)
    one = {k: _last_off_by_one(v) for k, v in one.items()}
    res['one_element'] = ratios(one)
    return res


def max_matches(c, n, na, family):
    """-> {'emulation': exact?, mutation: exact?} for the mutations the family is built to show"""
    t = W.max_inputs(c, n, na, family)
    ref = W.max_reference(t)
    same = lambda got: {k: (bool((got[k] == ref[k]).all()) if k == 'arg' else W.same_values(got[k], ref[k])) for k in ('out', 'arg', 'dx')}
    res = {'emulation': same(W.max_emulate(t))}
    if family in ('hard', 'soft'):                     # point n - 1 of cloud 0 holds the maximum of (channel 0, anchor 0)
        dropped = W.max_emulate(t, n_points=n - 1)
        dropped['dx'][:, :, n - 1] = 0.0
        res['drop_last_point'] = same(dropped)
    if family == 'soft' and n > 1:                     # every weight differs from its neighbour's
        res['shift_mask'] = same(W.max_emulate(t, mask=np.roll(t['mask'], 1, axis=1)))
    if family == 'ties' and n > 1:                     # n = 1 has no second point to tie with
        res['higher_index_on_tie'] = same(W.max_emulate(t, higher_on_tie=True))
    return res


@pytest.mark.parametrize('na,n', GRID)
def test_attention_pool_bounds(na, n):
    for c in W.C_GRID:
        for family in W.ATTN_FAMILIES:
            res = attn_ratios(c, n, na, family)
            for k, v in res.pop('emulation').items():
                assert v <= 1.0, (c, family, k, v)
            for k, v in res.pop('one_element').items():
                assert v > 1.0, (c, family, k, v)
            for mutation, r in res.items():
                # a wrong confidence is wrong in every output that reads it; behind a one-hot confidence dlogits is 0 whichever anchor is hot
                assert all(v > 1.0 for k, v in r.items() if not (k == 'dlogits' and family == 'wide_T3')), (c, family, mutation, r)


@pytest.mark.parametrize('na,n', GRID)
def test_slot_masked_mean_bounds(na, n):
    for c in W.C_GRID:
        for ns in W.NS_GRID:
            for family in W.SLOT_FAMILIES:
                res = slot_ratios(c, n, na, ns, family)
                for k, v in res.pop('emulation').items():
                    assert v <= 1.0, (c, ns, family, k, v)
                for mutation, r in res.items():
                    assert all(v > 1.0 for v in r.values()), (c, ns, family, mutation, r)


@pytest.mark.parametrize('na,n', GRID)
def test_masked_max_is_exact(na, n):
    for c in W.C_GRID:
        for family in W.MAX_FAMILIES:
            res = max_matches(c, n, na, family)
            assert all(res.pop('emulation').values()), (c, family)
            for mutation, r in res.items():
                if mutation == 'higher_index_on_tie':              # the value is the same, the point and the gradient are not
                    assert r['out'] and not r['arg'] and not r['dx'], (c, family, mutation, r)
                else:
                    assert not r['out'] and not r['dx'], (c, family, mutation, r)


# ---- InvPPOutBlock2DOurs ---------------------------------------------------------------------------------------------------------------------

PARAMS = {'dim_in': 8, 'mlp': [6], 'fc': [6], 'k': 6, 'kanchor': 60, 'temperature': 3.0}
MODES = {'attention': ('attention', None), 'max': ('max', None), 'mean': ('mean', None), 'sel_mode': ('max', 17)}


@pytest.mark.parametrize('tag', list(MODES))
def test_the_2d_head_has_the_reference_state_dict_and_attributes(golden, tag):
    import vgtk.so3conv as sptk
    g = golden('inv_head_2d.npz')
    pooling, sel = MODES[tag]
    head = sptk.InvPPOutBlock2DOurs(PARAMS, norm=1, pooling_method=pooling, sel_mode=sel)
    pre = f'{tag}_state_'
    assert {k[len(pre):] for k in g if k.startswith(pre)} == set(head.state_dict()), 'state_dict names differ from the reference class'
    assert (head.na, head.outDim, head.sel_mode) == (60, 6, sel)
    assert head.pooling_method == ('sel_mode' if sel is not None else pooling)
    assert hasattr(head, 'attention_layer') == (tag in ('attention', 'sel_mode'))
    if hasattr(head, 'attention_layer'):
        assert head.temperature == 3.0


def test_the_2d_head_refuses_sel_mode_new_and_host_tensors():
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    head = sptk.InvPPOutBlock2DOurs(PARAMS, norm=1, pooling_method='max', sel_mode=17)
    cloud = zptk.SphericalPointCloud(None, torch.randn(2, 8, 7, 240), None)
    with pytest.raises(NotImplementedError, match='L983-985'):
        head(cloud, sel_mode_new=torch.tensor([3, 5]))
    for pooling in ('attention', 'max', 'mean'):
        with pytest.raises(RuntimeError, match='CUDA'):
            sptk.InvPPOutBlock2DOurs(PARAMS, norm=1, pooling_method=pooling)(cloud)
    with pytest.raises(RuntimeError, match='CUDA'):
        head(cloud)
