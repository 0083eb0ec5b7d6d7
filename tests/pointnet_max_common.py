"""Shared by tests/test_gpu_pointnet_max.py: inputs, the float64 restatement of PointnetSO3Conv (vgtk/vgtk/so3conv/modules.py:L393-413) and of
its backward through a GIVEN arg-max, and the bounds.  The restatement is written once, generic over dtype and device: in float64 on the host
it is the reference, in float32 on the device it is `the same expression in float32 device torch ops` the coordinate gradient is held against.

u = 2^-24.  With S[b,o,n,a] = sum_c |W_f f| + sum_j |v x~| + |bias| from the float64 evaluation a value may be off by (C + 8) 2u S: twice what
either arithmetic can lose (the split-plane product 2^-22 per product, the fp32 chain (C + 4) u).  A gradient element that sums T products
may be off by (T + 8) 2u sum|terms|."""
import numpy as np
import torch

U = 2.0 ** -24


def anchors_of(na):
    import vgtk.so3conv.functional as L
    A = L.get_anchors(na)                    # the 20-, 40- and 60-anchor sets; any other count: that many of the 60 (the kernels take any table)
    return np.ascontiguousarray(A if A.shape[0] == na else np.concatenate([L.get_anchors(60)] * 2)[:na]).astype(np.float32)


def inputs(B, C, O, N, na, seed=0):
    """float32 numpy: feats [B,C,N,na], xyz [B,3,N], w [O,C+3], bias [O], anchors [na,3,3], g [B,O,na]"""
    rng = np.random.RandomState(1000 + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(feats=f(B, C, N, na), xyz=(0.4 * f(B, 3, N) + 0.2).astype(np.float32), w=(f(O, C + 3) / np.sqrt(C + 3)).astype(np.float32),
                bias=(0.3 * f(O)).astype(np.float32), anchors=anchors_of(na), g=f(B, O, na))


def planted(C=64, N=130, na=60, seed=3):
    """(1, C, N, N, na): channel o peaks at point o -- w[o,:C] a unit vector u_o, feats[:, n, :] = 50 u_n + noise -- so every point is some
    channel's arg"""
    d = inputs(1, C, N, N, na, seed)
    rng = np.random.RandomState(77 + seed)
    u = rng.standard_normal((N, C))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    assert (u @ u.T - np.eye(N)).max() < 0.8
    d['w'][:, :C] = u.astype(np.float32)
    d['w'][:, C:] *= 0.1
    d['feats'] = (50.0 * u.T[None, :, :, None] + 0.1 * d['feats']).astype(np.float32)
    return d


def centre_of(xyz, member=None):
    """float32, as the operator forms it (an input of the entry)"""
    if member is None:
        return xyz.mean(2)
    return (xyz * member.unsqueeze(1)).sum(2) / member.sum(1, keepdim=True).clamp(min=1.0)


def table_of(anchors, w, c):
    """v[o,a,:] = A_a W_x[o,:], float32 as the operator forms it (an input of the entry)"""
    return torch.einsum('aji,oi->oaj', anchors, w[:, c:]).contiguous()


def dense(feats, xc, w, v, bias, absolute=False):
    """y [B,O,N,na] of the entry's specification in the dtype of its arguments (absolute: S, the sum of the magnitudes)"""
    c = feats.shape[1]
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    y = torch.einsum('oc,bcna->bona', a(w[:, :c]), a(feats))
    if absolute:
        y = y + torch.einsum('oaj,bjn->bona', v.abs(), xc.abs())
    else:
        y = y + torch.einsum('oaj,bjn->bona', v, xc)
    return y + a(bias).view(1, -1, 1, 1)


def value_reference(d, centre, v, member=None):
    """float64 on the host from the entry's float32 inputs -> y64, the per-point bound, out64 and the bound per (b,o,a) over the members"""
    D = {k: torch.from_numpy(np.asarray(x)).double() for k, x in d.items()}
    xc = D['xyz'] - centre.double().cpu().unsqueeze(2)
    y = dense(D['feats'], xc, D['w'], v.double().cpu(), D['bias'])
    S = dense(D['feats'], xc, D['w'], v.double().cpu(), D['bias'], absolute=True)
    bound = (D['feats'].shape[1] + 8) * 2 * U * S
    if member is not None:
        off = (member.cpu() == 0).view(member.shape[0], 1, -1, 1)
        y_in, bound_in = y.masked_fill(off, float('-inf')), bound.masked_fill(off, 0.0)
    else:
        y_in, bound_in = y, bound
    return y, bound, y_in.max(2)[0], bound_in.max(2)[0]


def check_values(out, arg, y, out64, bound, member=None):
    """the value bound, and the arg bound: a member, whose y64 lies within twice the bound of the float64 maximum -> worst figures"""
    out, arg = torch.as_tensor(out).double(), torch.as_tensor(arg).long()
    B, O, N, na = y.shape
    assert bool((arg >= 0).all()) and bool((arg < N).all())
    if member is not None:
        assert bool(torch.gather(member.cpu().view(B, 1, N).expand(B, O, N), 2, arg).ne(0).all()), 'arg names a point that is no member'
    err = (out - out64).abs()
    at_arg = torch.gather(y, 2, arg.view(B, O, 1, na)).squeeze(2)
    gap = out64 - at_arg
    tiny = 1e-300
    fig_v, fig_a = float((err / bound.clamp(min=tiny)).max()), float((gap / (2 * bound).clamp(min=tiny)).max())
    assert fig_v <= 1.0, ('value', fig_v)
    assert fig_a <= 1.0, ('arg', fig_a)
    return fig_v, fig_a


def backward(feats, xyz, w, anchors, g, arg, member=None, absolute=False):
    """The gradients of <g, y gathered at arg> in the dtype / on the device of the arguments -> dict(dfeats, dxyz, dw [O,C+3], dbias).
    absolute: (sum of |terms|, number of terms) per element instead, the coordinate columns of dw counted product by product."""
    B, C, N, na = feats.shape
    O = w.shape[0]
    idx = arg.long()
    bi = torch.arange(B, device=feats.device).view(B, 1, 1)
    centre = xyz.mean(2) if member is None else (xyz * member.unsqueeze(1)).sum(2) / member.sum(1, keepdim=True).clamp(min=1.0)
    xc = xyz - centre.unsqueeze(2)
    fsel = torch.gather(feats.unsqueeze(1).expand(B, O, C, N, na), 3, idx.view(B, O, 1, 1, na).expand(B, O, C, 1, na)).squeeze(3)     # [B,O,C,na]
    xsel = xc.permute(0, 2, 1)[bi, idx]                                                                                              # [B,O,na,3]
    index = idx.unsqueeze(1)
    if absolute:
        ones = torch.ones_like
        terms, counts = {}, {}
        terms['dw'] = torch.cat([torch.einsum('boa,boca->oc', g.abs(), fsel.abs()),
                                 torch.einsum('boa,aji,boaj->oi', g.abs(), anchors.abs(), xsel.abs())], 1)
        counts['dw'] = torch.cat([torch.full((O, C), float(B * na)), torch.full((O, 3), float(3 * B * na))], 1).to(g)
        terms['dbias'], counts['dbias'] = g.abs().sum((0, 2)), torch.full((O,), float(B * na)).to(g)
        src = (w[:, :C].abs().view(1, O, C, 1) * g.abs().view(B, O, 1, na)).permute(0, 2, 1, 3)
        terms['dfeats'] = torch.zeros_like(feats).scatter_add_(2, index.expand(B, C, O, na), src)
        counts['dfeats'] = torch.zeros_like(feats).scatter_add_(2, index.expand(B, C, O, na), ones(src))
        return terms, counts
    res = {'dw': torch.cat([torch.einsum('boa,boca->oc', g, fsel), torch.einsum('boa,aji,boaj->oi', g, anchors, xsel)], 1), 'dbias': g.sum((0, 2))}
    src = (w[:, :C].view(1, O, C, 1) * g.view(B, O, 1, na)).permute(0, 2, 1, 3)                                                      # [B,C,O,na]
    res['dfeats'] = torch.zeros_like(feats).scatter_add_(2, index.expand(B, C, O, na), src)
    srcx = (w[:, C:].view(1, O, 3, 1) * g.view(B, O, 1, na)).permute(0, 2, 1, 3)
    dcoords = torch.zeros(B, 3, N, na, dtype=feats.dtype, device=feats.device).scatter_add_(2, index.expand(B, 3, O, na), srcx)
    dxc = torch.einsum('aji,bina->bjn', anchors, dcoords)
    total = dxc.sum(2, keepdim=True)
    res['dxyz'] = dxc - total / N if member is None else dxc - member.unsqueeze(1) * (total / member.sum(1).clamp(min=1.0).view(B, 1, 1))
    return res


def check_gradients(got, d, arg, dev, member=None):
    """got: dict(dfeats, dxyz, dw, dbias) of device float32 tensors; the float64 reference through y64 gathered at the kernel's own arg"""
    D = {k: torch.from_numpy(np.asarray(x)).double() for k, x in d.items()}
    m64 = None if member is None else member.double().cpu()
    arg = torch.as_tensor(arg).cpu()
    ref = backward(D['feats'], D['xyz'], D['w'], D['anchors'], D['g'], arg, m64)
    terms, counts = backward(D['feats'], D['xyz'], D['w'], D['anchors'], D['g'], arg, m64, absolute=True)
    figures = {}
    for k in ('dfeats', 'dw', 'dbias'):
        err = (got[k].detach().double().cpu() - ref[k]).abs()
        bound = (counts[k] + 8) * 2 * U * terms[k]
        assert bool((err <= bound).all()), (k, float((err / bound.clamp(min=1e-300)).max()))
        figures[k] = float((err / bound.clamp(min=1e-300)).max())
    assert bool((got['dfeats'].detach().cpu()[counts['dfeats'] == 0] == 0).all()), 'dfeats must be exactly 0 where no arg points'
    F = {k: torch.from_numpy(np.asarray(x)).to(dev) for k, x in d.items()}
    same32 = backward(F['feats'], F['xyz'], F['w'], F['anchors'], F['g'], arg.to(dev), None if member is None else member.to(dev))['dxyz']
    base = float((same32.double().cpu() - ref['dxyz']).abs().max())
    err = float((got['dxyz'].detach().double().cpu() - ref['dxyz']).abs().max())
    bar = 4 * base + 1e-6 * float(ref['dxyz'].abs().max())
    assert err <= bar, ('dxyz', err, bar)
    figures['dxyz'] = err / bar if bar else 0.0               # (one point: the centred coordinate is 0 and takes no gradient)
    return figures
