"""GPU: vgtk.so3conv.SlotAttention (SPConvNets/utils/slot_attention_spec_v2.py:L6-193) on csrc/slot_attention.hip: the module against the
fixture the reference class produced (tests/golden/slot_attention.npz), every entry through the C ABI against float64, the module's edge
cases against the float64 restatement of tests/slot_attention_common.py, run-to-run identity, and the memory the fused form may take."""
import numpy as np
import pytest
import torch

import slot_attention_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def G(golden):
    return C.load_fixture(golden)


def _model(state, s, d, hidden, dev, iters=C.ITERS):
    import vgtk.so3conv as sptk
    model = sptk.SlotAttention(s, d, iters=iters, eps=C.EPS, hidden_dim=hidden)
    model.load_state_dict(state, strict=True)
    return model.to(dev)


def _run(model, x, noise, w, layout='view'):
    """x [B,N,d] values on the device -> slots, attn, dx [B,N,d], {name: gradient}; layout 'view': the input is a transposed view of a
    contiguous [B,d,N] tensor, used in place; 'point_major': a contiguous [B,N,d] tensor"""
    if layout == 'view':
        leaf = x.transpose(1, 2).contiguous().requires_grad_(True)
        inputs = leaf.transpose(1, 2)
    else:
        leaf = inputs = x.clone().requires_grad_(True)
    slots, attn = model(inputs, noise=noise)
    names = [k for k, _ in model.named_parameters()]
    grads = torch.autograd.grad(C.functional(slots, attn, w), [leaf] + list(model.parameters()))
    dx = grads[0].transpose(1, 2) if layout == 'view' else grads[0]
    return slots.detach(), attn.detach(), dx, dict(zip(names, grads[1:]))


def _within_bars(got, want, what):
    """got / want: (slots, attn, dx, {name: gradient}); want in float64.  Each figure relative to the largest reference value."""
    cpu = lambda t: t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    figures = {'slots': (C.rel_err(cpu(got[0]), cpu(want[0])), C.BAR_OUT), 'attn': (C.rel_err(cpu(got[1]), cpu(want[1])), C.BAR_OUT),
               'dx': (C.rel_err(cpu(got[2]), cpu(want[2])), C.BAR_DX)}
    assert sorted(got[3]) == sorted(want[3])
    worst = max((C.rel_err(cpu(v), cpu(want[3][k])), k) for k, v in got[3].items())
    figures['parameters (worst: %s)' % worst[1]] = (worst[0], C.BAR_DPARAM)
    print(what, {k: f'{v[0]:.1e}' for k, v in figures.items()})
    for k, (err, bar) in figures.items():
        assert err < bar, (what, k, err)


# ---- the module against the reference's fixture ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout', ['view', 'point_major'])
@pytest.mark.parametrize('tag', list(C.VARIANTS))
def test_module_matches_reference_golden(dev, G, tag, layout):
    b, n, d, s, hidden = C.VARIANTS[tag]
    model = _model(C.state_of(G, tag), s, d, hidden, dev)
    x, noise = torch.from_numpy(G[f'{tag}_x']).to(dev), torch.from_numpy(G[f'{tag}_noise']).to(dev)
    got = _run(model, x, noise, C.functional_weights(G, tag, torch.float32, dev), layout)
    want = (G[f'{tag}_slots'], G[f'{tag}_attn'], G[f'{tag}_dx'], {k: G[f'{tag}_grad_{k}'] for k in got[3]})
    _within_bars(got, want, f'{tag} {layout}')
    assert np.array_equal(got[1].argmax(1).cpu().numpy(), np.asarray(G[f'{tag}_attn']).argmax(1)), 'the labels, argmax(attn_ori), at every point'


# ---- every entry through the C ABI against float64 --------------------------------------------------------------------------------------

# (n, d, s): 1 of each; the fixture's two; 2051 points cross the 64- and 256-point blocks and the 1024-point partials, 188 = 128 + 60
# is the orbit_attn == 1 width.  n % 4 != 0 in all four, which the scalar kernels take; (1284, 13, 5) moves 16-byte words over 6 blocks and
# 2 partials with a channel count that fills neither the 4 waves nor the 8-channel groups evenly, and runs again from storage that
# starts 4 bytes past a 16-byte boundary, which must take the scalar kernels.
ENTRY_SHAPES = [(1, 1, 1, 0), (37, 20, 3, 0), (130, 131, 2, 0), (2051, 188, 8, 0), (1284, 13, 5, 0), (1284, 13, 5, 1)]


def _offset(t, by):
    """the same values in storage that starts `by` floats past an allocation (allocations are at least 256-byte aligned)"""
    if not by:
        return t.contiguous()
    flat = torch.empty(t.numel() + by, dtype=t.dtype, device=t.device)
    out = flat[by:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * by and out.is_contiguous()
    return out


def _entry_figures(dev, n, d, s, by, shift=0.0):
    """-> {entry / output: (kernel error, float32 torch error, largest reference value)}, errors against the float64 evaluation of the
    same float32 operands on the same device"""
    from vgtk import _hip
    b = 2
    gen = torch.Generator(device=dev).manual_seed(1000 + n + d + s)
    r = lambda *shape: torch.randn(*shape, generator=gen, device=dev)
    x = _offset(torch.relu(r(b, d, n)) * 1.5 + 0.2 + shift, by)
    mean, rstd = (_offset(t, by) for t in C.ref_stats(x))
    u, c0 = r(b, s, d) * (2.0 / d ** 0.5), r(b, s) * 0.5
    attn = _offset(C.ref_scores_fwd(x, mean, rstd, u, c0), by)
    signed = _offset(r(b, s, n) * 0.1, by)
    gmsum, gwsum, gattn = r(b, s, d) * 0.3, r(b, s), _offset(r(b, s, n), by)
    gdots = _offset(C.ref_scores_bwd(x, mean, rstd, attn, gmsum, gwsum, gattn), by)
    rows, vecs = _offset(torch.cat([attn, gdots], 1), by), torch.cat([gmsum, u], 1)
    cases = {'stats': (_hip.slot_attn_stats, C.ref_stats, (x,), (C.LN_EPS,))}
    if not shift:
        cases.update({
            'scores_fwd': (_hip.slot_attn_scores_fwd, C.ref_scores_fwd, (x, mean, rstd, u, c0), (C.EPS,)),
            'pool(attn)': (_hip.slot_attn_pool, C.ref_pool, (x, mean, rstd, attn), ()),
            'pool(signed)': (_hip.slot_attn_pool, C.ref_pool, (x, mean, rstd, signed), ()),
            'scores_bwd': (_hip.slot_attn_scores_bwd, C.ref_scores_bwd, (x, mean, rstd, attn, gmsum, gwsum, gattn), (C.EPS,)),
            'scores_bwd(null gattn)': (_hip.slot_attn_scores_bwd, C.ref_scores_bwd, (x, mean, rstd, attn, gmsum, gwsum, None), (C.EPS,)),
            'input_grad': (_hip.slot_attn_input_grad, C.ref_input_grad, (x, mean, rstd, rows, vecs), ())})
    figures = {}
    for name, (kernel, expr, tensors, scalars) in cases.items():
        tup = lambda v: v if isinstance(v, tuple) else (v,)
        got, again = tup(kernel(*tensors, *scalars)), tup(kernel(*tensors, *scalars))
        f32 = tup(expr(*tensors, *scalars))
        f64 = tup(expr(*(None if t is None else t.double() for t in tensors), *scalars))
        for i, (k_, a_, t_, w_) in enumerate(zip(got, again, f32, f64)):
            assert k_.shape == w_.shape and k_.dtype == torch.float32 and torch.equal(k_, a_), name
            figures[f'{name}[{i}]' if len(got) > 1 else name] = (float((k_.double() - w_).abs().max()), float((t_.double() - w_).abs().max()),
                                                                 float(w_.abs().max()))
    return figures


@pytest.mark.parametrize('n,d,s,by', ENTRY_SHAPES)
def test_entries_against_float64(dev, n, d, s, by):
    """Bound, per entry and output: the kernel's largest error against float64 is at most 4 x the largest error of the same expression
    in float32 torch ops on the same device and operands, plus 1e-6 of the largest reference value.  The 4 pays for the differing
    summation order and exponential; it is not a measured number."""
    figures = _entry_figures(dev, n, d, s, by)
    if (n, d, s, by) == (2051, 188, 8, 0):               # the statistics once more with 100 added to every channel
        figures.update({k + ' +100': v for k, v in _entry_figures(dev, n, d, s, by, shift=100.0).items()})
    for k, (err_k, err_t, top) in figures.items():
        print(f'entry (n,d,s)=({n},{d},{s}) offset {by}: {k:28s} kernel {err_k:.3e}  torch f32 {err_t:.3e}  largest reference {top:.3e}')
    for k, (err_k, err_t, top) in figures.items():
        assert err_k <= 4 * err_t + 1e-6 * top, (k, err_k, err_t, top)


# ---- the module's edge cases against the float64 restatement ------------------------------------------------------------------------------

def _fresh_case(dev, b, n, d, s, hidden, iters, seed):
    import vgtk.so3conv as sptk
    torch.manual_seed(seed)
    model = sptk.SlotAttention(s, d, iters=iters, eps=C.EPS, hidden_dim=hidden)
    with torch.no_grad():
        for m in model.norm_input:
            m.weight.normal_(1.0, 0.3); m.bias.normal_(0.0, 0.3)
    x = torch.relu(torch.randn(b, n, d)) * 1.5 + 0.2
    noise = torch.randn(b, s, d)
    w = (torch.randn(b, s, d), torch.randn(b, s, d) * 0.5, torch.randn(b, s, n), torch.randn(b, s, n) * 0.5)
    return model.to(dev), x.to(dev), noise.to(dev), tuple(t.to(dev) for t in w)


@pytest.mark.parametrize('s,iters', [(1, 3), (3, 1), (9, 3)], ids=['one_slot', 'one_iteration', 'nine_slots_tensor_ops'])
def test_module_edge_cases(dev, s, iters):
    """S = 1: attention is 1 + eps and no gradient reaches the scores; iters = 1; S = 9 runs the same algebra as device tensor ops"""
    b, n, d, hidden = 2, 50, 12, 16
    model, x, noise, w = _fresh_case(dev, b, n, d, s, hidden, iters, seed=3 + s)
    got = _run(model, x, noise, w)
    state = {k: v.detach() for k, v in model.state_dict().items()}
    P = {k: v.double().requires_grad_(True) for k, v in state.items()}
    x64 = x.double().requires_grad_(True)
    slots, attn = C.restated_forward(P, x64, noise.double(), s, iters=iters)
    grads = torch.autograd.grad(C.functional(slots, attn, tuple(t.double() for t in w)), [x64] + list(P.values()))
    _within_bars(got, (slots, attn, grads[0], dict(zip(P, grads[1:]))), f'S={s} iters={iters}')
    if s == 1:
        assert torch.equal(got[1], torch.full_like(got[1], 1.0 + C.EPS))


def test_noise_none_draws_what_the_reference_draws(dev):
    model, x, noise, w = _fresh_case(dev, 2, 40, 12, 3, 16, 3, seed=5)
    with torch.no_grad():
        torch.manual_seed(123)
        a = model(x)
        torch.manual_seed(123)
        drawn = torch.randn(2, 3, 12, device=dev)
        b_ = model(x, noise=drawn)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])


def test_two_runs_are_bit_identical(dev, G):
    tag = 'orbit3'
    b, n, d, s, hidden = C.VARIANTS[tag]
    model = _model(C.state_of(G, tag), s, d, hidden, dev)
    x, noise = torch.from_numpy(G[f'{tag}_x']).to(dev), torch.from_numpy(G[f'{tag}_noise']).to(dev)
    w = C.functional_weights(G, tag, torch.float32, dev)
    first, second = _run(model, x, noise, w), _run(model, x, noise, w)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])
    for k in first[3]:
        assert torch.equal(first[3][k], second[3][k]), k


# ---- memory -------------------------------------------------------------------------------------------------------------------------------

def test_forward_and_backward_stay_within_six_inputs(dev):
    """(B,N,d,S) = (2,2048,64,4): the growth of the peak allocation over the state with x (and the model) allocated is at most 6 x bytes(x).
    The reference form saves at least 3 S = 12 input-sized tensors for the backward alone; the fused form needs the per-iteration gx
    tensors and [B,S,N] rows (S/d of x each).  A condition from the shapes, not a measurement."""
    b, n, d, s = 2, 2048, 64, 4
    model, x, noise, w = _fresh_case(dev, b, n, d, s, 128, 3, seed=11)
    leaf = x.transpose(1, 2).contiguous().requires_grad_(True)
    del x

    def step():
        slots, attn = model(leaf.transpose(1, 2), noise=noise)
        C.functional(slots, attn, w).backward()

    step()                                                 # (the libraries' workspaces are allocated once, here)
    leaf.grad = None
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    x_bytes = leaf.numel() * 4
    print(f'peak growth {growth} bytes = {growth / x_bytes:.2f} x bytes(x)')
    assert growth <= 6 * x_bytes, growth / x_bytes
