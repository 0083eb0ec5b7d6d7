"""vgtk.cuda.grouping -- replaces the pybind module of vgtk/vgtk/cuda/grouping_cuda.cpp."""
import torch

from .. import _hip



def _same_dtype(op, **tensors):
    """All floating tensors of one call share a dtype (the reference dispatches on the first and reads the rest as that type)."""
    kinds = {name: t.dtype for name, t in tensors.items()}
    if len(set(kinds.values())) > 1:
        raise RuntimeError(f'{op}: ' + ', '.join(f'{n} {d}' for n, d in kinds.items()) + ' must have the same dtype')


def ball_query(new_xyz, xyz, radius, nsample):
    """(new_xyz T [B,3,M], xyz T [B,3,N], float radius, int nsample) -> int32 [B,M,nsample].
    grouping_cuda.cpp:L71-86."""
    _hip.check_input(new_xyz, xyz)
    if new_xyz.dtype != xyz.dtype:
        raise RuntimeError('ball_query: new_xyz and xyz must have the same dtype')
    b, _, m = new_xyz.shape
    n = xyz.shape[2]
    idx = torch.empty(b, m, nsample, dtype=torch.int32, device=xyz.device)
    _hip.call('eap_ball_query_' + _hip.suffix(xyz), xyz, b, n, m, radius, int(nsample), new_xyz, xyz, idx)
    return idx


def furthest_point_sampling(xyz, m):
    """(xyz T [B,3,N], int m) -> int32 [B,m]; grouping_cuda.cpp:L160-174."""
    _hip.check_input(xyz)
    sfx = _hip.suffix(xyz)
    b, _, n = xyz.shape
    idx = torch.empty(b, m, dtype=torch.int32, device=xyz.device)
    temp = torch.empty(b, n, dtype=xyz.dtype, device=xyz.device)
    _hip.call('eap_furthest_point_sampling_' + sfx, xyz, b, n, int(m), xyz, temp, idx)
    return idx


def anchor_query(sample_idx, grouped_idx, grouped_xyz, anchors, kernel_pts, nq):
    """-> [w T [B,P,A,K,NN]]; grouping_cuda.cpp:L88-108."""
    _hip.check_input(sample_idx, grouped_idx, grouped_xyz, anchors, kernel_pts)
    _same_dtype('anchor_query', grouped_xyz=grouped_xyz, anchors=anchors, kernel_pts=kernel_pts)
    sfx = _hip.suffix(grouped_xyz)
    b, _, np_, nn = grouped_xyz.shape
    na, ks = anchors.shape[0], kernel_pts.shape[0]
    w = torch.empty(b, np_, na, ks, nn, dtype=grouped_xyz.dtype, device=grouped_xyz.device)
    _hip.call('eap_anchor_query_' + sfx, w, b, np_, nn, na, ks, grouped_xyz, anchors, kernel_pts, w)
    return [w]


def initial_anchor_query(centers, xyz, kernel_pts, radius, sigma):
    """-> [w, cnt] T [B,K,NC,A]; grouping_cuda.cpp:L138-158."""
    _hip.check_input(centers, xyz, kernel_pts)
    _same_dtype('initial_anchor_query', centers=centers, xyz=xyz, kernel_pts=kernel_pts)
    sfx = _hip.suffix(centers)
    b, _, nc = centers.shape
    m = xyz.shape[0]
    ks, na, _ = kernel_pts.shape
    w = torch.empty(b, ks, nc, na, dtype=centers.dtype, device=centers.device)
    cnt = torch.empty_like(w)
    _hip.call('eap_initial_anchor_query_' + sfx, w, b, nc, m, na, ks, radius, sigma, centers, xyz, kernel_pts, w, cnt)
    return [w, cnt]
