"""Top-level `chamfer` module -- replaces the reference's compiled pybind module of the same name
(extensions/chamfer_dist/chamfer_cuda.cpp:L36-39: `forward`, `backward`) with calls into
libeap_hip.so.  float32 (the reference's build) or float64 (what its extensions/chamfer_dist/test.py
asks the kernels to be recompiled in); both clouds in the same width."""
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
