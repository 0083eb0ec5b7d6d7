"""GPU: the orbit chamfer node (extensions.chamfer_dist.OrbitChamferFunction on csrc/orbit_chamfer.hip) behind
orbit_reconstruction_distances and global_orbit_distances, and vgtk.so3conv.global_orbit_selection.

Two comparators.  The composition of two pairwise ChamferFunction calls on repeated copies of the cloud (tests/orbit_chamfer_common.py, pinned on
the host by tests/test_orbit_chamfer_host.py) evaluates every squared distance with the node's arithmetic and tie rule, so forward values are
compared with torch.equal.  The reference's materialised [B,S,A,M,N] expression (oracle/orbit_ref.py) in float64 on the CPU holds the node to
the bars tests/test_gpu_chamfer_f64.py holds the function to: outputs rtol 1e-12, gradient 1e-10 of its largest magnitude."""
import contextlib

import numpy as np
import pytest
import torch

import orbit_chamfer_common as C
from oracle import orbit_ref

pytestmark = pytest.mark.gpu

WIDTHS = {'f32': torch.float32, 'f64': torch.float64}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@contextlib.contextmanager
def recorded_calls():
    """the names of the C entries reached through vgtk._hip.call inside the block"""
    from vgtk import _hip
    names, real = [], _hip.call

    def spy(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    _hip.call = spy
    try:
        yield names
    finally:
        _hip.call = real


def on(dev, tensors):
    return tuple(t.to(dev) for t in tensors)


# ---- values and indices ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', C.MASKED)
@pytest.mark.parametrize('width', list(WIDTHS))
def test_the_node_equals_the_composition_bit_for_bit(dev, tag, width):
    import chamfer
    from extensions.chamfer_dist import ChamferFunction, orbit_reconstruction_distances
    recon, ori, labels = on(dev, C.inputs(tag, WIDTHS[width]))
    b, s, a, m, n = C.SHAPES[tag]
    with recorded_calls() as names:
        got = orbit_reconstruction_distances(recon, ori, labels)
    assert names == ['eap_orbit_chamfer_fwd_' + width]
    want = C.composition(ChamferFunction.apply, recon, ori, labels)
    for name, u, v in zip(('o2r_all', 'r2o_all', 'r2o_in', 'o2r_in'), got, want):
        assert u.shape == v.shape and u.dtype == v.dtype == WIDTHS[width], name
        assert torch.equal(u, v), (name, (u - v).abs().max().item())
    # the per-point maps and their indices
    member = (labels.transpose(1, 2) >= 0.5).to(torch.uint8).contiguous().view(b * s, n)
    r2o_all, r2o_all_idx, r2o_in, r2o_in_idx, o2r_all, o2r_idx, o2r_in = chamfer.orbit_forward(recon.reshape(b * s, a, m, 3), ori, member)
    w_r2o, w_r2o_idx, w_in, w_in_idx, w_o2r, w_o2r_idx = C.composition_maps(chamfer.forward, recon, ori, labels)
    assert torch.equal(r2o_all, w_r2o) and torch.equal(r2o_all_idx, w_r2o_idx)
    assert torch.equal(o2r_all, w_o2r) and torch.equal(o2r_idx, w_o2r_idx)
    assert torch.equal(o2r_in, torch.where(member[:, None].bool().expand_as(o2r_all), o2r_all, torch.full_like(o2r_all, C.MASKED_DISTANCE)))
    assert torch.equal(r2o_in, w_in)
    found = r2o_in < 9e4
    assert torch.equal(r2o_in_idx[found], w_in_idx[found]) and (r2o_in_idx[~found] == -1).all()
    assert (r2o_in[~found] == C.MASKED_DISTANCE).all()
    empty = member.sum(1) == 0                                   # [G]
    assert empty.any() == (tag == 'empty_slot')
    assert torch.equal(found, (~empty)[:, None, None].expand_as(found))
    assert (r2o_in_idx[found] >= 0).all() and (r2o_in_idx[found] < n).all()
    group = torch.arange(b * s, device=dev)[:, None, None].expand_as(r2o_in_idx)
    assert (member[group[found], r2o_in_idx[found].long()] == 1).all()          # every masked nearest neighbour is a point of the slot


@pytest.mark.parametrize('width', list(WIDTHS))
def test_stage0_equals_the_reference_expression_bit_for_bit(dev, width):
    from extensions.chamfer_dist import ChamferFunction, global_orbit_distances
    recon, ori, _ = on(dev, C.inputs('stage0', WIDTHS[width]))
    with recorded_calls() as names:
        got = global_orbit_distances(recon[:, 0], ori)
    assert names == ['eap_orbit_chamfer_fwd_' + width]
    want = C.stage0_expression(ChamferFunction.apply, recon[:, 0], ori)
    b, _, a, _, _ = C.SHAPES['stage0']
    for u, v in zip(got, want):
        assert tuple(u.shape) == (b, a) and u.dtype == WIDTHS[width] and torch.equal(u, v)


@pytest.mark.parametrize('width', list(WIDTHS))
def test_the_first_of_equal_candidates_wins(dev, width):
    """the second half of the input cloud and of every reconstruction repeats the first, a block (recon) or a tile (cloud) later: every
    nearest neighbour has an equal twin with a higher index, and the lower one must be named, in both directions and under the mask"""
    import chamfer
    recon, ori, labels = on(dev, C.tied(WIDTHS[width]))
    b, s, a, m, n = C.TIES
    member = (labels.transpose(1, 2) >= 0.5).to(torch.uint8).contiguous().view(b * s, n)
    r2o_all, r2o_all_idx, r2o_in, r2o_in_idx, o2r_all, o2r_idx, _ = chamfer.orbit_forward(recon.reshape(b * s, a, m, 3), ori, member)
    assert (r2o_all_idx >= 0).all() and (r2o_all_idx < n // 2).all()
    assert (r2o_in_idx >= 0).all() and (r2o_in_idx < n // 2).all()
    assert (o2r_idx >= 0).all() and (o2r_idx < m // 2).all()
    # and the twins see the same distances
    assert torch.equal(r2o_all[:, :, m // 2:], r2o_all[:, :, :m // 2]) and torch.equal(r2o_in[:, :, m // 2:], r2o_in[:, :, :m // 2])
    assert torch.equal(o2r_all[:, :, n // 2:], o2r_all[:, :, :n // 2]) and torch.equal(o2r_idx[:, :, n // 2:], o2r_idx[:, :, :n // 2])
    w = C.composition_maps(chamfer.forward, recon, ori, labels)
    assert torch.equal(r2o_all_idx, w[1]) and torch.equal(r2o_in_idx, w[3]) and torch.equal(o2r_idx, w[5])


# ---- against the reference's expression ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(C.SHAPES))
def test_float64_against_the_materialised_expression(dev, tag):
    """outputs rtol 1e-12, gradient 1e-10 of its largest magnitude, random weights zeroed on the 99999 entries (constants carry no gradient);
    stage0: the unmasked half of the same expression with one slot per cloud, through global_orbit_distances"""
    from extensions.chamfer_dist import global_orbit_distances, orbit_reconstruction_distances
    recon, ori, labels = C.inputs(tag)
    rc = recon.clone().requires_grad_(True)
    want = orbit_ref.orbit_reconstruction_distances(rc, ori, torch.ones_like(labels) if tag == 'stage0' else labels)
    rg = recon.clone().to(dev).requires_grad_(True)
    if tag == 'stage0':
        want = (want[1][:, 0], want[0][:, 0].mean(-1))
        got = global_orbit_distances(rg[:, 0], ori.to(dev))
    else:
        got = orbit_reconstruction_distances(rg, ori.to(dev), labels.to(dev))
    for u, v in zip(got, want):
        assert u.shape == v.shape and u.dtype == torch.float64
        np.testing.assert_allclose(u.detach().cpu().numpy(), v.detach().numpy(), rtol=1e-12, atol=0)
    gen = torch.Generator().manual_seed(3)
    wts = [torch.randn(v.shape, dtype=torch.float64, generator=gen) for v in want]
    wts = [torch.where(v.detach() < 9e4, w, torch.zeros_like(w)) for v, w in zip(want, wts)]
    sum((v * w).sum() for v, w in zip(want, wts)).backward()
    sum((u * w.to(dev)).sum() for u, w in zip(got, wts)).backward()
    err = (rg.grad.cpu() - rc.grad).abs().max().item() / rc.grad.abs().max().item()
    print(f'orbit node gradient, float64, {tag}: {err:.3e}')
    assert err <= 1e-10


@pytest.mark.parametrize('tag', C.MASKED)
def test_float32_gradient_against_the_compositions(dev, tag):
    """rtol 1e-5, atol 1e-6: the bars of tests/test_gpu_parity.py::test_orbit_reconstruction_distances.  The weights on an empty slot's
    99999 entries are NOT zeroed here: both sides must send nothing through them."""
    from extensions.chamfer_dist import ChamferFunction, orbit_reconstruction_distances
    recon, ori, labels = on(dev, C.inputs(tag, torch.float32))
    ra, rb = recon.clone().requires_grad_(True), recon.clone().requires_grad_(True)
    got = orbit_reconstruction_distances(ra, ori, labels)
    want = C.composition(ChamferFunction.apply, rb, ori, labels)
    gen = torch.Generator().manual_seed(3)
    wts = [torch.randn(v.shape, generator=gen).to(dev) for v in want]
    sum((u * w).sum() for u, w in zip(got, wts)).backward()
    sum((v * w).sum() for v, w in zip(want, wts)).backward()
    np.testing.assert_allclose(ra.grad.cpu().numpy(), rb.grad.cpu().numpy(), rtol=1e-5, atol=1e-6)
    if tag == 'empty_slot':
        # a gradient on the masked mean alone finds nothing to reach in the empty slot
        rz = recon.clone().requires_grad_(True)
        r2o_in = orbit_reconstruction_distances(rz, ori, labels)[2]
        assert (r2o_in[:, -1] == C.MASKED_DISTANCE).all()
        r2o_in.sum().backward()
        assert (rz.grad[:, -1] == 0).all() and (rz.grad[:, 0] != 0).any()


def test_the_float32_backward_is_bit_identical_run_to_run(dev):
    """hundreds of input points name each of the five reconstruction points; the global determinism switch is left as it is found"""
    import chamfer
    from extensions.chamfer_dist import orbit_reconstruction_distances
    was = torch.are_deterministic_algorithms_enabled()
    recon, ori, labels = on(dev, C.seeded(C.REPRODUCIBLE, torch.float32))
    b, s, a, m, n = C.REPRODUCIBLE
    o2r_idx = chamfer.orbit_forward(recon.reshape(b * s, a, m, 3), ori)[5]
    assert all(torch.bincount(o2r_idx[g, k].long(), minlength=m).max().item() >= 200 for g in range(b * s) for k in range(a))
    gen = torch.Generator().manual_seed(3)
    wts = None
    runs = []
    for _ in range(2):
        r = recon.clone().requires_grad_(True)
        with recorded_calls() as names:
            out = orbit_reconstruction_distances(r, ori, labels)
            wts = wts or [torch.randn(v.shape, generator=gen).to(dev) for v in out]
            torch.autograd.backward(list(out), wts)
        assert names == ['eap_orbit_chamfer_fwd_f32', 'eap_orbit_chamfer_bwd_f32']
        runs.append(r.grad)
    assert torch.equal(runs[0], runs[1]) and runs[0].abs().max().item() > 0
    assert torch.are_deterministic_algorithms_enabled() == was


# ---- memory ----------------------------------------------------------------------------------------------------------------------
def test_the_forward_holds_three_maps_not_copies_of_the_cloud(dev):
    """peak memory across orbit_reconstruction_distances with grad enabled, above the inputs, stays below 1.5 x G*A*N*12 bytes.  The bound is
    a count: the node allocates two [G,A,N] value maps and one index map (1.0 x that figure) and the [G,A,M] maps (M / N = 1.6 %); the
    composition held two [G*A,N,3] copies of the cloud plus two value and two index maps per call, more than 3 x."""
    from extensions.chamfer_dist import orbit_reconstruction_distances
    b, s, a, m, n = C.MEMORY
    recon, ori, labels = on(dev, C.seeded(C.MEMORY, torch.float32))
    recon.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    with torch.enable_grad():
        out = orbit_reconstruction_distances(recon, ori, labels)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    unit = b * s * a * n * 12
    print(f'peak above the inputs: {peak} bytes = {peak / unit:.3f} x G*A*N*12')
    assert out[0].requires_grad and peak < 1.5 * unit


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def test_a_cloud_that_needs_a_gradient_takes_the_composition(dev):
    from extensions.chamfer_dist import ChamferFunction, global_orbit_distances, orbit_reconstruction_distances
    recon, ori, labels = on(dev, C.inputs('empty_slot', torch.float32))
    want = C.composition(ChamferFunction.apply, recon, ori, labels)
    og = ori.clone().requires_grad_(True)
    with recorded_calls() as names:
        got = orbit_reconstruction_distances(recon, og, labels)
    assert names == ['eap_chamfer_fwd_f32'] * 2
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    (got[0].sum() + got[1].sum()).backward()
    assert og.grad is not None and og.grad.abs().max().item() > 0
    # stage 0 likewise
    recon0, ori0, _ = on(dev, C.inputs('stage0', torch.float32))
    og = ori0.clone().requires_grad_(True)
    with recorded_calls() as names:
        got = global_orbit_distances(recon0[:, 0], og)
    assert names == ['eap_chamfer_fwd_f32']
    for u, v in zip(got, C.stage0_expression(ChamferFunction.apply, recon0[:, 0], ori0)):
        assert torch.equal(u, v)
    sum(g.sum() for g in got).backward()
    assert og.grad is not None and og.grad.abs().max().item() > 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import chamfer
    from extensions.chamfer_dist import global_orbit_distances, orbit_reconstruction_distances
    recon, ori, labels = on(dev, C.inputs('empty_slot', torch.float32))
    b, s, a, m, n = C.SHAPES['empty_slot']
    for args in ((recon.cpu(), ori, labels), (recon, ori.cpu(), labels), (recon, ori, labels.cpu()),          # a host tensor
                 (recon.double(), ori, labels), (recon, ori.double(), labels),                                # mixed widths
                 (recon, ori, labels[:, :-1]), (recon, ori, labels[:, :, :-1]), (recon, ori, labels[:1])):    # labels that do not match
        with pytest.raises(RuntimeError):
            orbit_reconstruction_distances(*args)
    for args in ((recon[:, 0].cpu(), ori), (recon[:, 0], ori.cpu()), (recon[:, 0].double(), ori), (recon[:, 0], ori[:1])):
        with pytest.raises(RuntimeError):
            global_orbit_distances(*args)
    flat = recon.reshape(b * s, a, m, 3)
    member = torch.ones(b * s, n, dtype=torch.uint8, device=dev)
    for args in ((flat, ori, member.cpu()), (flat, ori, member.bool()), (flat, ori, member[:, :-1].contiguous()), (flat[:5], ori, member[:5]),
                 (flat.half(), ori.half(), member)):
        with pytest.raises(RuntimeError):
            chamfer.orbit_forward(*args)


# ---- the selection above stage 0 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('glb_single_cd', [0, 1])
def test_global_orbit_selection_matches_the_reference_statements(dev, glb_single_cd):
    """...pn_38_multi_stage.py:L444-461 written out on the same device tensors (batched_index_select on [B,A] values with [B,1] indices
    is values.gather(1, indices))"""
    import vgtk.so3conv as sptk
    from extensions.chamfer_dist import global_orbit_distances
    recon, ori, _ = on(dev, C.inputs('stage0', torch.float32))
    chamfer_recon_to_ori, chamfer_ori_to_recon = global_orbit_distances(recon[:, 0], ori)
    if glb_single_cd == 1:
        glb_chamfer = chamfer_ori_to_recon
    else:
        glb_chamfer = chamfer_recon_to_ori + chamfer_ori_to_recon
    minn_glb_chamfer, glb_orbit = torch.min(glb_chamfer, dim=-1)
    minn_chamfer_recon_to_ori = chamfer_recon_to_ori.gather(1, glb_orbit.unsqueeze(-1)).squeeze(-1)
    minn_chamfer_ori_to_recon = chamfer_ori_to_recon.gather(1, glb_orbit.unsqueeze(-1)).squeeze(-1)
    glb_recon_ori_dist = (torch.sqrt(minn_chamfer_recon_to_ori) + torch.sqrt(minn_chamfer_ori_to_recon)).mean() * 0.5
    glb_ori_to_recon_dist = torch.sqrt(minn_chamfer_ori_to_recon).mean()
    got = sptk.global_orbit_selection(chamfer_recon_to_ori, chamfer_ori_to_recon, glb_single_cd=glb_single_cd)
    assert len(got) == 4 and got[1].dtype == torch.int64 and tuple(got[1].shape) == (recon.shape[0],)
    assert torch.equal(got[1], glb_orbit)
    for u, v in zip((got[0], got[2], got[3]), (minn_glb_chamfer, glb_recon_ori_dist, glb_ori_to_recon_dist)):
        assert u.shape == v.shape and torch.equal(u, v)
