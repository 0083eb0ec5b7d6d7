"""CPU: PointnetSO3Conv's embed fused with the max over the points (vgtk.so3conv.pointnet_max, csrc/pointnet_max.hip) as far as it goes
without a device: the four C-ABI entries on calls that return before they launch (null pointers and a null stream, so nothing but the host
check can have run), the operator's refusal of host tensors, and the modules on host tensors -- which keep the reference's dense expression
-- against tests/golden/pointnet_max.npz, made by the reference's own classes."""
import numpy as np
import pytest
import torch

INVALID_VALUE = 1           # hipErrorInvalidValue
# name -> (argument count, scalars after (b, c, o, n, na) by position)
ENTRIES = {'eap_pointnet_max_fwd_f32': 17, 'eap_pointnet_max_bwd_data_f32': 12, 'eap_pointnet_max_bwd_weight_f32': 13}
LDW = {'eap_pointnet_max_bwd_data_f32': 8}           # position of the `int ldw` argument


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def _args(name, b, c, o, n, na):
    """(b, c, o, n, na, null pointers ... with ldw = c + 3 in its place, null stream)"""
    args = [b, c, o, n, na] + [None] * (ENTRIES[name] - 5)
    if name in LDW:
        args[LDW[name]] = c + 3
    return tuple(args)


def test_the_entries_have_the_headers_arity(hip):
    for name, count in ENTRIES.items():
        assert len(getattr(hip.abi, name).argtypes) == count, name
    assert len(hip.abi.eap_pointnet_max_parts.argtypes) == 1
    assert hip.abi.eap_abi_version() == 1


def test_an_empty_batch_returns_before_a_pointer_is_touched(hip):
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, 0, 8, 16, 40, 60)) == 0, name
        assert getattr(hip.abi, name)(*_args(name, 0, 0, 0, 0, 7)) == 0, name


@pytest.mark.parametrize('which,word', [(1, 'c '), (2, 'o '), (3, 'n ')])
def test_an_empty_dimension_is_refused_by_name(hip, which, word):
    for name in ENTRIES:
        sizes = [3, 8, 16, 40, 60]
        sizes[which] = 0
        assert getattr(hip.abi, name)(*_args(name, *sizes)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert msg.startswith(name[len('eap_'):-len('_f32')] + ': ' + word) and 'must be positive' in msg, msg


@pytest.mark.parametrize('na', [0, 2, 65, 68])
def test_an_anchor_count_off_the_rule_is_refused(hip, na):
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, 3, 8, 16, 40, na)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert msg.startswith(name[len('eap_'):-len('_f32')] + ': na ') and 'multiple of 4, at most 64' in msg, msg


def test_null_pointers_and_a_short_pitch_are_refused_after_the_sizes(hip):
    for name in ENTRIES:
        assert getattr(hip.abi, name)(*_args(name, 3, 8, 16, 40, 60)) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert name[len('eap_'):-len('_f32')] in msg and 'null' in msg, msg
    for name, at in LDW.items():
        args = list(_args(name, 3, 8, 16, 40, 60))
        args[at] = 7
        assert getattr(hip.abi, name)(*args) == INVALID_VALUE, name
        assert 'ldw' in hip.abi.eap_last_error().decode()
    assert hip.abi.eap_pointnet_max_bwd_data_f32(*_args('eap_pointnet_max_bwd_data_f32', 3, 8, 4096, 40, 60)) == INVALID_VALUE
    assert 'o ' in hip.abi.eap_last_error().decode() and '2048' in hip.abi.eap_last_error().decode()


def test_one_partial_per_128_points(hip):
    """csrc/pointnet_max.hip: a workgroup walks 16 chunks of 8 points"""
    assert [hip.abi.eap_pointnet_max_parts(n) for n in (0, 1, 128, 129, 130, 257, 4096)] == [0, 1, 1, 2, 2, 3, 32]


def test_the_operator_refuses_host_tensors():
    import vgtk.so3conv as sptk
    anchors = torch.from_numpy(sptk.get_anchors(60))
    with pytest.raises(RuntimeError, match='device tensors only'):
        sptk.pointnet_max(torch.zeros(1, 4, 9, 60), torch.zeros(1, 3, 9), torch.zeros(6, 7), torch.zeros(6), anchors)


@pytest.mark.parametrize('cls', ['conv', 'pose'])
@pytest.mark.parametrize('ka', [60, 20])
def test_the_modules_on_host_tensors_reproduce_the_reference(golden, ka, cls):
    """host tensors keep the dense expression: float32 to torch's rounding, float64 to 1e-12"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    G = golden('pointnet_max.npz')
    T = lambda k: torch.from_numpy(np.asarray(G[f'{ka}_{k}']))
    c, o = T('feats').shape[1], T('g').shape[1]
    net = sptk.PointnetSO3Conv(c, o, kanchor=ka) if cls == 'conv' else sptk.PointnetSO3PoseConv(c, o, kanchor=ka)
    state = {k[len(f'{ka}_{cls}_state_'):]: torch.from_numpy(v) for k, v in G.items() if k.startswith(f'{ka}_{cls}_state_')}
    assert list(net.state_dict().keys()) == list(state.keys()) == ['anchors', 'embed.weight', 'embed.bias']
    net.load_state_dict(state)
    for dtype, bar in ((torch.float32, 2e-6), (torch.float64, 1e-12)):
        net = net.to(dtype)
        x, f = T('xyz').to(dtype).requires_grad_(True), T('feats').to(dtype).requires_grad_(True)
        res = net(zptk.SphericalPointCloud(x, f, None))
        grads = torch.autograd.grad((res * T('g').to(dtype)).sum(), [f, x, net.embed.weight, net.embed.bias])
        for name, got in zip(('out', 'grad_feats', 'grad_xyz', 'grad_weight', 'grad_bias'), (res,) + grads):
            ref = T(f'{cls}_{name}').double()
            if dtype == torch.float64:
                # the fixture is float32 arithmetic: float64 agrees with it to float32's rounding, and with itself (the same expression in
                # float64 on the fixture's inputs) to 1e-12
                again = _dense_reference(net, T('xyz').double(), T('feats').double(), T('g').double())[name]
                assert float((got.detach() - again).abs().max()) <= bar * float(again.abs().max()), (name, dtype)
                bar_ref = 2e-5
            else:
                bar_ref = bar * 10
            assert got.shape == ref.shape, name
            assert float((got.detach().double() - ref).abs().max()) <= bar_ref * float(ref.abs().max()), (name, dtype)


def _dense_reference(net, xyz, feats, g):
    """the statements of modules.py:L393-413 on float64 tensors, with autograd"""
    x, f = xyz.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    w, b = net.embed.weight.detach().double().requires_grad_(True), net.embed.bias.detach().double().requires_grad_(True)
    xc = x - x.mean(2, keepdim=True)
    cat = torch.cat([f, torch.einsum('aji,bjn->bina', net.anchors.double(), xc)], 1)
    res = torch.max(torch.nn.functional.conv2d(cat, w, b), 2)[0]
    grads = torch.autograd.grad((res * g).sum(), [f, x, w, b])
    return dict(zip(('out', 'grad_feats', 'grad_xyz', 'grad_weight', 'grad_bias'), (res.detach(),) + grads))
