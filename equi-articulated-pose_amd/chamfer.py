"""Top-level `chamfer` module -- replaces the reference's compiled pybind module of the same name
(extensions/chamfer_dist/chamfer_cuda.cpp:L36-39: `forward`, `backward`) with calls into
libeap_hip.so.  float32 (the reference's build) or float64 (what its extensions/chamfer_dist/test.py
asks the kernels to be recompiled in); both clouds in the same width.

orbit_forward / orbit_backward are not the reference's: they are the typed calls of the shared-target search over the orbit
(csrc/orbit_chamfer.hip) that extensions.chamfer_dist.OrbitChamferFunction wraps."""
import torch

from vgtk import _hip


def _width(xyz1, xyz2, what):
    if xyz1.dtype != xyz2.dtype:
        raise RuntimeError(f'chamfer.{what}: both clouds in one width, not {xyz1.dtype} and {xyz2.dtype}')
    return _hip.suffix(xyz1)


def forward(xyz1, xyz2):
    """(xyz1 [B,n,3], xyz2 [B,m,3], float32 or float64) -> [dist1 [B,n], dist2 [B,m] (input width), idx1 i32 [B,n], idx2 i32 [B,m]]"""
    _hip.check_input(xyz1, xyz2)
    sfx = _width(xyz1, xyz2, 'forward')
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dev = xyz1.device
    d1 = torch.empty(b, n, dtype=xyz1.dtype, device=dev)
    d2 = torch.empty(b, m, dtype=xyz1.dtype, device=dev)
    i1 = torch.empty(b, n, dtype=torch.int32, device=dev)
    i2 = torch.empty(b, m, dtype=torch.int32, device=dev)
    _hip.call('eap_chamfer_fwd_' + sfx, xyz1, b, n, m, xyz1, xyz2, d1, d2, i1, i2)
    return [d1, d2, i1, i2]


def _orbit_sizes(recon, ori, member, what):
    """the checks shared by orbit_forward / orbit_backward -> (suffix, g, s, a, m, n)"""
    _hip.check_input(recon, ori, member)
    if recon.dtype != ori.dtype:
        raise RuntimeError(f'chamfer.{what}: recon and ori in one width, not {recon.dtype} and {ori.dtype}')
    sfx = _hip.suffix(recon)
    if recon.dim() != 4 or recon.shape[3] != 3 or ori.dim() != 3 or ori.shape[1] != 3:
        raise RuntimeError(f'chamfer.{what}: recon [G,A,M,3] and ori [B,3,N], not {tuple(recon.shape)} and {tuple(ori.shape)}')
    g, a, m, _ = recon.shape
    b, _, n = ori.shape
    if b < 1 or g % b:
        raise RuntimeError(f'chamfer.{what}: {g} groups are not a whole number of slots for each of {b} clouds')
    if member is not None and (member.dtype != torch.uint8 or tuple(member.shape) != (g, n)):
        raise RuntimeError(f'chamfer.{what}: member uint8 [G,N] = {(g, n)}, not {member.dtype} {tuple(member.shape)}')
    return sfx, g, g // b, a, m, n


def orbit_forward(recon, ori, member=None):
    """The shared-target search of csrc/orbit_chamfer.hip (eap_orbit_chamfer_fwd_*): recon [G,A,M,3], ori [B,3,N] planar (G = B*S, the cloud
    of group g is g // S), member uint8 [G,N] or None for "every point is in"
    -> [r2o_all [G,A,M], r2o_all_idx i32, r2o_in [G,A,M], r2o_in_idx i32, o2r_all [G,A,N], o2r_idx i32, o2r_in [G,A,N]];
    the three masked entries are None without member."""
    sfx, g, s, a, m, n = _orbit_sizes(recon, ori, member, 'orbit_forward')
    dev = recon.device
    val = lambda *shape: torch.empty(*shape, dtype=recon.dtype, device=dev)
    idx = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    r2o_all, r2o_all_idx, o2r_all, o2r_idx = val(g, a, m), idx(g, a, m), val(g, a, n), idx(g, a, n)
    r2o_in, r2o_in_idx, o2r_in = (val(g, a, m), idx(g, a, m), val(g, a, n)) if member is not None else (None, None, None)
    _hip.call('eap_orbit_chamfer_fwd_' + sfx, recon, g, s, a, m, n, recon, ori, member, r2o_all, r2o_all_idx, r2o_in, r2o_in_idx, o2r_all, o2r_idx,
              o2r_in)
    return [r2o_all, r2o_all_idx, r2o_in, r2o_in_idx, o2r_all, o2r_idx, o2r_in]


def orbit_backward(recon, ori, member, r2o_all_idx, r2o_in_idx, o2r_idx, g_r2o_all, g_r2o_in, g_o2r_all, g_o2r_in):
    """-> grad_recon [G,A,M,3]: the ordered gather of eap_orbit_chamfer_bwd_* (no atomics, the same bits every run).  Without member the
    masked index and the two masked gradients are None.  ori gets no gradient."""
    sfx, g, s, a, m, n = _orbit_sizes(recon, ori, member, 'orbit_backward')
    masked = (r2o_in_idx, g_r2o_in, g_o2r_in)
    if any((t is None) != (member is None) for t in masked):
        raise RuntimeError('chamfer.orbit_backward: the masked index and gradients go with member: all given or all None')
    grads = [t if t is None else t.contiguous() for t in (g_r2o_all, g_r2o_in, g_o2r_all, g_o2r_in)]
    idxs = (r2o_all_idx, r2o_in_idx, o2r_idx)
    _hip.check_input(*idxs, *grads)
    shapes = ((g, a, m), (g, a, m), (g, a, n))
    for t, shape in zip(idxs, shapes):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != shape):
            raise RuntimeError(f'chamfer.orbit_backward: int32 index {shape}, not {t.dtype} {tuple(t.shape)}')
    for t, shape in zip(grads, ((g, a, m), (g, a, m), (g, a, n), (g, a, n))):
        if t is not None and (t.dtype != recon.dtype or tuple(t.shape) != shape):
            raise RuntimeError(f'chamfer.orbit_backward: {recon.dtype} gradient {shape}, not {t.dtype} {tuple(t.shape)}')
    grecon = torch.empty_like(recon)
    _hip.call('eap_orbit_chamfer_bwd_' + sfx, recon, g, s, a, m, n, recon, ori, member, *idxs, *grads, grecon)
    return grecon


def backward(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2, ordered=None):
    """-> [grad_xyz1 [B,n,3], grad_xyz2 [B,m,3]]
    ordered: the gather that sums in a fixed order (eap_chamfer_bwd_ordered_*: no atomics, the same bits every run) instead of the
    reference's atomicAdd scatter (eap_chamfer_bwd_f32).  None: float64 always (it has no scatter), float32 when
    torch.are_deterministic_algorithms_enabled()."""
    grad_dist1 = grad_dist1.contiguous()
    grad_dist2 = grad_dist2.contiguous()
    _hip.check_input(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2)
    sfx = _width(xyz1, xyz2, 'backward')
    if grad_dist1.dtype != xyz1.dtype or grad_dist2.dtype != xyz1.dtype or idx1.dtype != torch.int32 or idx2.dtype != torch.int32:
        raise RuntimeError(f'chamfer.backward: gradients in the clouds\' width ({xyz1.dtype}) and int32 indices, not '
                           f'{grad_dist1.dtype}, {grad_dist2.dtype}, {idx1.dtype}, {idx2.dtype}')
    if ordered is None:
        ordered = sfx == 'f64' or torch.are_deterministic_algorithms_enabled()
    if not ordered and sfx != 'f32':
        raise RuntimeError('chamfer.backward: float64 has the ordered backward only (ordered=False is the float32 atomicAdd scatter)')
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    g1 = torch.empty_like(xyz1)
    g2 = torch.empty_like(xyz2)
    _hip.call('eap_chamfer_bwd_ordered_' + sfx if ordered else 'eap_chamfer_bwd_f32', xyz1, b, n, m, xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2,
              g1, g2)
    return [g1, g2]
