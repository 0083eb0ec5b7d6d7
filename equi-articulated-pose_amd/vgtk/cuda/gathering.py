"""vgtk.cuda.gathering -- replaces the pybind module of vgtk/vgtk/cuda/gathering_cuda.cpp."""
import torch

from .. import _hip


def gather_points_forward(pts, idx):
    """(pts T [B,C,N], idx int32 [B,M]) -> float32 [B,C,M]; gathering_cuda.cpp:L29-43
    (the reference allocates a Float output whatever the input dtype)."""
    _hip.check_input(pts, idx)
    if idx.dtype != torch.int32:
        raise RuntimeError('gather_points_forward: idx must be int32')
    b, c, n = pts.shape
    m = idx.shape[1]
    out = torch.empty(b, c, m, dtype=torch.float32, device=pts.device)
    _hip.call('eap_gather_points_fwd_' + _hip.suffix(pts), out, b, c, n, m, pts, idx, out)
    return out


def gather_points_backward(grad_out, idx, npoint, ordered=None):
    """(grad T [B,C,M], idx int32 [B,M], int npoint) -> T [B,C,npoint]; gathering_cuda.cpp:L45-60.
    ordered: the sum over ascending j with idx[b,j] == q along inverse lists built on the device (eap_gather_points_bwd_ordered_*:
    no float atomics, the same bits every run) instead of the reference's atomicAdd scatter.  None:
    torch.are_deterministic_algorithms_enabled()."""
    _hip.check_input(grad_out, idx)
    if idx.dtype != torch.int32:
        raise RuntimeError('gather_points_backward: idx must be int32')
    b, c, m = grad_out.shape
    npoint = int(npoint)
    out = torch.empty(b, c, npoint, dtype=grad_out.dtype, device=grad_out.device)
    if _hip.use_ordered(ordered):
        # (the conditions of gather_ordered in csrc/native_ordered.hip and of the list builders: target rows, the grid)
        if npoint <= _hip.INV_LISTS_MAX_ROWS and b <= _hip.GRID_YZ_MAX and c <= 4 * _hip.GRID_YZ_MAX:
            lists = _hip.inv_lists(idx.view(b, m, 1), npoint) if b > 0 and m > 0 and npoint > 0 else (None,) * 4
            _hip.call('eap_gather_points_bwd_ordered_' + _hip.suffix(grad_out), out, b, c, npoint, m, grad_out, *lists, out)
            return out
        _hip.no_deterministic('gather_points_backward', f'{npoint} target rows, {b} clouds, {c} channels: the ordered kernel and its inverse lists take '
                              f'{_hip.INV_LISTS_MAX_ROWS} rows, {_hip.GRID_YZ_MAX} clouds and {4 * _hip.GRID_YZ_MAX} channels', requested=ordered is True)
    _hip.call('eap_gather_points_bwd_' + _hip.suffix(grad_out), out, b, c, npoint, m, grad_out, idx, out)
    return out
