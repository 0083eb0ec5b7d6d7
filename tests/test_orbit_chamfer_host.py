"""CPU: the orbit chamfer entries (csrc/orbit_chamfer.hip) as far as they go without a device -- their prototypes as the header reader of
vgtk._hip binds them, the host checks on calls that return before anything is launched (null pointers, a null stream) -- and the comparator
of tests/orbit_chamfer_common.py pinned to the reference's materialised expression (oracle/orbit_ref.py) before tests/test_gpu_orbit_chamfer.py
trusts it on the device."""
import ctypes

import numpy as np
import pytest
import torch

import orbit_chamfer_common as C
from oracle import orbit_ref

INVALID_VALUE = 1           # hipErrorInvalidValue
# i = int, s = the stream, a digit = a pointer to elements of that many bytes
SIGNATURES = {
    # g s a m n | recon ori member | r2o_all idx r2o_in idx o2r_all idx o2r_in | stream
    'eap_orbit_chamfer_fwd_f32': 'iiiii' + '441' + '4444444' + 's',
    'eap_orbit_chamfer_fwd_f64': 'iiiii' + '881' + '8484848' + 's',
    # g s a m n | recon ori member | three indices | four gradients | grecon | stream
    'eap_orbit_chamfer_bwd_f32': 'iiiii' + '441' + '444' + '4444' + '4' + 's',
    'eap_orbit_chamfer_bwd_f64': 'iiiii' + '881' + '444' + '8888' + '8' + 's',
}


@pytest.fixture(scope='module')
def hip():
    from vgtk import _hip
    return _hip


def _signature(fn):
    names = {ctypes.c_int: 'i', ctypes.c_void_p: 's'}
    return ''.join(names[t] if t in names else str(t.width) for t in fn.argtypes)


def _call(hip, name, g, s, a, m, n, pointer=None):
    return getattr(hip.abi, name)(g, s, a, m, n, *([pointer] * (len(SIGNATURES[name]) - 6)), None)


def test_the_prototypes_parse_with_their_arity_and_widths(hip):
    for name, want in SIGNATURES.items():
        fn = getattr(hip.abi, name)
        assert len(fn.argtypes) == len(want), name
        assert _signature(fn) == want, name
        assert fn.restype is ctypes.c_int, name
    assert hip.abi.eap_abi_version() == 1


def test_no_group_returns_before_a_pointer_is_touched(hip):
    for name in SIGNATURES:
        assert _call(hip, name, 0, 1, 60, 256, 4096) == 0, name
        assert _call(hip, name, 0, 0, 0, 0, 0) == 0, name


@pytest.mark.parametrize('sizes,word', [((4, 2, 0, 5, 7), 'must be positive'), ((4, 2, 3, 0, 7), 'must be positive'), ((4, 2, 3, 5, 0), 'must be positive'),
                                        ((4, 0, 3, 5, 7), 'must be positive'), ((4, 3, 3, 5, 7), 'slots'),
                                        ((16, 2, 60, 256, 2300000), '2^31'), ((16, 2, 60, 800000, 64), '2^31')])
def test_sizes_off_the_rule_are_refused_by_name(hip, sizes, word):
    """A, M, N >= 1; the groups are whole clouds x slots; every tensor an int indexes stays below 2^31 elements"""
    for name in SIGNATURES:
        assert _call(hip, name, *sizes) == INVALID_VALUE, name
        msg = hip.abi.eap_last_error().decode()
        assert msg.startswith('orbit_chamfer_' + ('forward' if '_fwd_' in name else 'backward')) and word in msg, msg


def test_null_pointers_are_refused_after_the_sizes(hip):
    for name in SIGNATURES:
        assert _call(hip, name, 4, 2, 3, 5, 7) == INVALID_VALUE, name
        assert 'null' in hip.abi.eap_last_error().decode()


def test_the_python_entries_refuse_host_tensors():
    import chamfer
    from extensions.chamfer_dist import global_orbit_distances, orbit_reconstruction_distances
    recon, ori, labels = C.inputs('empty_slot', torch.float32)
    with pytest.raises(RuntimeError):
        chamfer.orbit_forward(recon.reshape(6, 3, 5, 3), ori)
    with pytest.raises(RuntimeError):
        orbit_reconstruction_distances(recon, ori, labels)
    with pytest.raises(RuntimeError):
        global_orbit_distances(recon[:, 0], ori)


# ---- the comparator itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(C.SHAPES))
def test_the_composition_reproduces_the_reference_expression(tag):
    """float64 on the host, the pairwise chamfer a plain-torch nearest-neighbour search: values to 1e-12 (sums of three squares and means of
    them, positive terms; the 99999 constants exact), the gradient to 1e-10 of its largest magnitude -- the bars of
    tests/test_gpu_chamfer_f64.py.  The stage-0 expression is the unmasked half of the same block with one slot per cloud."""
    recon, ori, labels = C.inputs(tag)
    if tag == 'stage0':
        labels = torch.ones_like(labels)
    rc, rg = recon.clone().requires_grad_(True), recon.clone().requires_grad_(True)
    want = orbit_ref.orbit_reconstruction_distances(rc, ori, labels)
    got = C.composition(C.torch_pair, rg, ori, labels)
    assert (want[3].detach() > 9e4).any() == (tag != 'stage0')         # points outside a slot carry the masked constant
    assert (want[2].detach() > 9e4).any() == (tag == 'empty_slot')     # and so does the whole of an empty slot
    for u, v in zip(got, want):
        assert u.shape == v.shape
        np.testing.assert_allclose(u.detach().numpy(), v.detach().numpy(), rtol=1e-12, atol=0)
    gen = torch.Generator().manual_seed(3)
    wts = [torch.randn(v.shape, dtype=torch.float64, generator=gen) for v in want]
    wts = [torch.where(v.detach() < 9e4, w, torch.zeros_like(w)) for v, w in zip(want, wts)]
    sum((v * w).sum() for v, w in zip(want, wts)).backward()
    sum((u * w).sum() for u, w in zip(got, wts)).backward()
    assert (rg.grad - rc.grad).abs().max().item() <= 1e-10 * rc.grad.abs().max().item()
    if tag == 'stage0':
        r2o, o2r = C.stage0_expression(C.torch_pair, recon[:, 0], ori)
        np.testing.assert_allclose(r2o.numpy(), want[1][:, 0].detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(o2r.numpy(), want[0][:, 0].detach().mean(-1).numpy(), rtol=1e-12, atol=0)


def test_the_seeded_slots_hold_points_where_they_are_meant_to():
    for tag, (b, s, a, m, n) in C.SHAPES.items():
        per_slot = C.inputs(tag)[2].sum(1)                      # [B,S]
        assert per_slot.sum().item() == b * n
        filled = per_slot[:, :s - 1] if tag == 'empty_slot' else per_slot
        assert (filled > 0).all(), tag
        if tag == 'empty_slot':
            assert (per_slot[:, s - 1] == 0).all()
    for shape in (C.REPRODUCIBLE, C.MEMORY):
        assert (C.seeded(shape)[2].sum(1) > 0).all()
    recon, ori, labels = C.tied(torch.float32)
    m, n = C.TIES[3], C.TIES[4]
    assert torch.equal(recon[:, :, :, m // 2:], recon[:, :, :, :m // 2]) and torch.equal(ori[:, :, n // 2:], ori[:, :, :n // 2])
    assert m // 2 > 256 and n // 2 > 1024                       # the copies sit in a later block and a later tile than their originals
