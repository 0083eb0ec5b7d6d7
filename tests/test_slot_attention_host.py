"""CPU: vgtk.so3conv.SlotAttention (SPConvNets/utils/slot_attention_spec_v2.py:L6-193) as far as it goes without a device: the algebra the
class runs, restated in torch (tests/slot_attention_common.py), against tests/golden/slot_attention.npz, which the reference class
produced with its per-slot [B,S,N,d] keys and values; the class's state_dict; and the entries of csrc/slot_attention.hip on calls that
return before they launch."""
import pytest
import torch

import slot_attention_common as C

INVALID_VALUE = 1           # hipErrorInvalidValue
# entry -> (arity with the stream, arguments up to the first pointer as a function of (s, d, n) with b = 1, the name of the count argument)
ENTRIES = {
    'eap_slot_attn_stats_f32': (8, lambda s, d, n: (1, d, n, 1e-5), None),
    'eap_slot_attn_scores_fwd_f32': (12, lambda s, d, n: (1, s, d, n, 1e-8), 's (slots)'),
    'eap_slot_attn_pool_f32': (10,lambda s, d, n: (1, s, d, n), 's (slots)'),
    'eap_slot_attn_scores_bwd_f32': (14, lambda s, d, n: (1, s, d, n, 1e-8), 's (slots)'),
    'eap_slot_attn_input_grad_f32': (11, lambda s, d, n: (1, s, d, n), 'j (outer products)'),
}


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


@pytest.fixture(scope='module')
def G(golden):
    return C.load_fixture(golden)


def _call(hip, name, s, d, n):
    arity, head, _ = ENTRIES[name]
    head = head(s, d, n)
    return getattr(hip.abi, name)(*head, *((None,) * (arity - len(head))))


@pytest.mark.parametrize('tag', list(C.VARIANTS))
def test_restatement_in_float64_equals_the_reference(G, tag):
    """slots, attn_ori, dL/dx and every parameter gradient to 1e-12 of the largest reference value: the algebra and the helper"""
    b, n, d, s, hidden = C.VARIANTS[tag]
    state = C.state_of(G, tag)
    x, noise = torch.from_numpy(G[f'{tag}_x']), torch.from_numpy(G[f'{tag}_noise'])
    assert x.shape == (b, n, d) and noise.shape == (b, s, d) and x.dtype == torch.float32
    slots, attn, dx, grads = C.restated_run(state, x, noise, s, C.functional_weights(G, tag), torch.float64)
    figures = {'slots': C.rel_err(slots, G[f'{tag}_slots']), 'attn': C.rel_err(attn, G[f'{tag}_attn']), 'dx': C.rel_err(dx, G[f'{tag}_dx'])}
    figures.update({k: C.rel_err(v, G[f'{tag}_grad_{k}']) for k, v in grads.items()})
    print({k: f'{v:.1e}' for k, v in figures.items()})
    assert sorted(grads) == sorted(k[len(f'{tag}_grad_'):] for k in G if k.startswith(f'{tag}_grad_'))
    for k, v in figures.items():
        assert v < 1e-12, (k, v)
    assert float(G[f'{tag}_gap']) >= 5 * C.BAR_OUT                       # argmax(attn_ori) is decided by five times the output bar


@pytest.mark.parametrize('tag', list(C.VARIANTS))
def test_state_dict_is_the_references(G, tag):
    import vgtk.so3conv as sptk
    b, n, d, s, hidden = C.VARIANTS[tag]
    state = C.state_of(G, tag)
    model = sptk.SlotAttention(s, d, iters=C.ITERS, eps=C.EPS, hidden_dim=hidden)
    own = model.state_dict()
    assert list(own) == list(state) and [tuple(v.shape) for v in own.values()] == [tuple(v.shape) for v in state.values()]
    model.load_state_dict(state, strict=True)
    assert model.mlp[0][0].out_features == max(d, hidden) and (model.num_slots, model.iters, model.eps) == (s, C.ITERS, C.EPS)


def test_a_host_tensor_is_refused():
    import vgtk.so3conv as sptk
    model = sptk.SlotAttention(2, 8)
    with pytest.raises(RuntimeError, match='device tensors only'):
        model(torch.zeros(1, 5, 8))
    with pytest.raises(AssertionError):
        model(torch.zeros(1, 5, 8), num_slots=3)


def test_the_entries_are_bound_with_the_headers_arity(hip):
    for name, (arity, _, _) in ENTRIES.items():
        assert len(getattr(hip.abi, name).argtypes) == arity, name
    assert len(hip.abi.eap_slot_attn_pool_parts.argtypes) == 1
    assert [hip.abi.eap_slot_attn_pool_parts(n) for n in (0, 1, 1024, 1025, 2051, 4096)] == [0, 1, 1, 2, 3, 4]


@pytest.mark.parametrize('s,d,n,word', [(0, 20, 37, 'count'), (9, 20, 37, 'count'), (3, 0, 37, 'd (channels)'), (3, 20, 0, 'n (points)')])
def test_a_size_outside_the_range_is_refused_before_any_device_call(hip, s, d, n, word):
    """null pointers and a null stream, on a machine without a device: nothing but the argument check can have run"""
    for name, (_, _, count_name) in ENTRIES.items():
        if word == 'count' and count_name is None:
            continue                                                     # (the statistics take no slot count)
        count = 2 * s if name.endswith('input_grad_f32') else s          # j = 2 s outer products: 0 and 18, past its cap of 16
        assert _call(hip, name, count, d, n) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert name[len('eap_'):-len('_f32')] in msg and (count_name if word == 'count' else word) in msg, msg


def test_an_empty_batch_returns_before_a_pointer_is_touched(hip):
    for name, (arity, head, _) in ENTRIES.items():
        args = (0,) + head(3, 20, 37)[1:]
        assert getattr(hip.abi, name)(*args, *((None,) * (arity - len(args)))) == 0, name
