"""vgtk.so3conv.functional -- operator layer of the SE(3)-equivariant point convolution
(reference: vgtk/vgtk/so3conv/functional.py).  Same function names, argument order and return
structures as the reference; the compute runs in libeap_hip.so (HIP, gfx950):

    ball_query -> so3_prep (offsets, relative-rotation anchor) -> fused grouping
    (kernel weights + anchor permutation + gather + weighted sum) -> fp32-MFMA contraction

Differences a caller can observe (all documented in DESIGN.md):
  * `inter_w` is returned as a lazy `InterWeights` handle; call `.materialize()` (or set
    vgtk.so3conv.functional.MATERIALIZE_INTER_W = True) to get the [b,p,na,ks,nn] tensor the
    reference always builds (12 GB at B=8, P=4096).  Callers in SPConvNets only hand it back to
    the next conv, which ignores it for stride 1 (functional.py:L1025ff recomputes everything).
  * gradients flow to `feats` and `W` (what the reference trains); xyz / pose are treated as data.
  * device tensors only -- there is no CPU path.  float32 everywhere; float64 (every tensor of the call) for the plain inter and
    intra convs, the contraction and the grouping API: "the float64 regime" below, its own kernels (csrc/so3_f64.hip).
"""
import math
import os
import weakref

import numpy as np
import torch

import vgtk
import vgtk.functional as fr
import vgtk.pc as pctk
import vgtk.spconv as zpconv
import vgtk.cuda.grouping as cuda_nn

from .. import _hip
from . import norm_fold

inter_so3conv_feat_grouping = zpconv.inter_zpconv_grouping_naive
batched_index_select = zpconv.batched_index_select
batched_index_select_other = zpconv.batched_index_select_other

MATERIALIZE_INTER_W = False

# ------------------------------------------------------------------------------------------------
# constants (functional.py:L111-121, L2630-2659)
# ------------------------------------------------------------------------------------------------
GAMMA_SIZE = 3
ROOT = vgtk.__path__[0]
Rs, R_idx, canonical_relative = fr.icosahedron_so3(GAMMA_SIZE)
_KP = np.load(os.path.join(ROOT, 'data', 'anchors', 'constants.npz'))


def select_anchor(anchors, k):
    if k == 1:
        return anchors[29][None]
    elif k == 20:
        return anchors[::3]
    elif k == 40:
        return anchors.reshape(20, 3, 3, 3)[:, :2].reshape(-1, 3, 3)
    return anchors


def get_anchors(k=60):
    return select_anchor(Rs, k)


def get_intra_idx():
    return R_idx


def get_canonical_relative():
    return canonical_relative


def get_kernel_points_np(radius, aperature, kernel_size, multiplier=1):
    """Kernel points [n,3] on a cone around +z (functional.py:L73-89): shell i of `kernel_size` shells sits at height
    z_i = i * radius / (kernel_size - 1) and carries i * multiplier + 1 polar angles alpha (interior points of
    [0, aperature / 2]); the j-th of them contributes a circle of 2 j + 1 points of radius z_i tan(alpha)."""
    assert isinstance(kernel_size, int)
    shells = []
    for i, z in enumerate(np.linspace(0, radius, kernel_size, dtype=np.float32)):
        for j, alpha in enumerate(zpconv.get_angular_kernel_points_np(aperature, i * multiplier + 1)):
            n = 2 * j + 1
            phi = np.linspace(0, 2 * np.pi, n, endpoint=False, dtype=np.float32)
            rho = z * np.tan(alpha)
            shells.append(np.stack([rho * np.cos(phi), rho * np.sin(phi), np.full(n, z)], axis=1))
    return np.concatenate(shells, axis=0)


def get_spherical_kernel_points_np(radius, kernel_size, multiplier=3):
    """Kernel points [n,3] on concentric spheres (functional.py:L91-109): sphere i of radius i * radius / (kernel_size - 1)
    carries an m x m longitude / colatitude grid, m = i * multiplier + 1 (longitudes without, colatitudes with end point)."""
    assert isinstance(kernel_size, int)
    spheres = []
    for i, r in enumerate(np.linspace(0, radius, kernel_size, dtype=np.float32)):
        m = i * multiplier + 1
        lon = np.linspace(0, 2 * np.pi, m, endpoint=False, dtype=np.float32)[:, None]
        col = np.linspace(0, np.pi, m, endpoint=True, dtype=np.float32)[None, :]
        xyz = np.stack([r * np.cos(lon) * np.sin(col), r * np.sin(lon) * np.sin(col), np.broadcast_to(r * np.cos(col), (m, m))], axis=-1)
        spheres.append(xyz.reshape(m * m, 3))
    return np.concatenate(spheres, axis=0)


def get_sphereical_kernel_points_from_ply(radius, kernel_size):
    """kernel_size 1/2/3 -> 24/30/66 kernel points rescaled so the max norm is `radius`."""
    assert 0 < kernel_size <= 3
    pts = _KP['kpsphere%d' % {1: 24, 2: 30, 3: 66}[kernel_size]].astype('float32')
    r = np.sqrt((pts ** 2).sum(1).max())
    return pts * radius / r


def get_2D_res_anchors():
    """4 rotations about the y axis by multiples of 90 degrees (functional.py:L29-46) -> [4,3,3]."""
    mats = []
    for i in range(4):
        th = i * (np.pi / 2.)
        c, s_ = np.cos(th), np.sin(th)
        mats.append(torch.from_numpy(np.array([[c, 0., s_], [0., 1., 0.], [-s_, 0., c]], dtype=np.float64)).float().unsqueeze(0))
    return torch.cat(mats, dim=0)


RES_ROT_2D = get_2D_res_anchors()


def initial_anchor_query(frag, centers, kernels, r, sigma):
    """frag [m,3], centers [b,3,nc], kernels [ks,na,3] -> (w, cnt) [b,ks,nc,na] (functional.py:L129-130)."""
    return cuda_nn.initial_anchor_query(centers, frag, kernels, r, sigma)


def inter_so3conv_blurring(xyz, feats, n_neighbor, radius, stride, inter_idx=None, lazy_sample=True,
                           radius_expansion=1.0):
    """Low-pass blur / pool before a strided conv (functional.py:L133-141)."""
    sample_idx = sample_xyz = None
    if inter_idx is None:
        _, inter_idx, sample_idx, sample_xyz = zpconv.inter_zpconv_grouping_ball(xyz, stride, radius * radius_expansion,
                                                                               n_neighbor, lazy_sample)
    if stride == 1:
        return zpconv.inter_blurring_naive(inter_idx, feats), xyz
    return zpconv.inter_pooling_naive(inter_idx, sample_idx, feats), sample_xyz


def canonicalize_points(xyz, pose):
    """R^T (x - t) per point (functional.py:L206-214): xyz [b,3,p], pose [b,p,4,4] -> [b,3,p]."""
    rotations = pose[:, :, :3, :3]
    translations = pose[:, :, :3, -1]
    cana = torch.matmul(torch.transpose(rotations, 2, 3),
                        (xyz.contiguous().transpose(1, 2).contiguous() - translations).unsqueeze(-1)).squeeze(-1)
    return cana.contiguous().transpose(1, 2).contiguous()


def get_occupancy_features(pc, n_anchor, use_center=False):
    """pc [nb,np,3] -> ones [nb,1,np,na] (functional.py:L50-69; normals are not supported --
    the reference branch for them is broken: `ns.anchors` at L61)."""
    nb, np_, nd = pc.shape
    if nd != 3:
        raise NotImplementedError('get_occupancy_features: xyz-only point clouds')
    features = torch.ones(nb, 1, np_, n_anchor, dtype=torch.float32, device=pc.device)
    if use_center:
        features[:, :, 0, :] = 0.0
    return features


def _call_dtype(op, **tensors):
    """float32 or float64: the ONE width of a call's floating tensors (None entries are skipped).  RuntimeError naming the first tensor
    that is neither, or that differs from the first one given."""
    items = [(name, t) for name, t in tensors.items() if t is not None]
    first_name, first = items[0]
    if first.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f'{op}: {first_name} is {first.dtype}: float32 tensors, or float64 ones throughout')
    for name, t in items[1:]:
        if t.dtype != first.dtype:
            raise RuntimeError(f'{op}: {name} is {t.dtype} but {first_name} is {first.dtype}: every tensor of a call has one width '
                               f'(float32, or float64 throughout)')
    return first.dtype


# ------------------------------------------------------------------------------------------------
# per-(anchor set, kernel set, device) tables
# ------------------------------------------------------------------------------------------------
_TABLES = {}


def _group_tables(anchors):
    """mult table (uint8 [na,na]) + identity index when `anchors` is a group, else (None, None)."""
    # keyed on the tensor OBJECT and its version counter (a load_state_dict / copy_ into the buffer bumps
    # the version; a recycled allocation is a different object), never on the data pointer
    key = (id(anchors), anchors._version, str(anchors.device), anchors.shape[0])
    hit = _TABLES.get(key)
    if hit is not None and hit[0]() is anchors:
        return hit[1]
    A = anchors.detach().double().cpu().numpy()
    na = A.shape[0]
    prod = np.einsum('gij,ajk->gaik', A, A)
    score = np.einsum('gaij,cij->gac', prod, A)
    mult = score.argmax(-1)
    closed = np.allclose(score.max(-1), 3.0, atol=1e-4)
    ident = int(np.einsum('cii->c', A).argmax())
    has_identity = np.allclose(A[ident], np.eye(3), atol=1e-5)
    if closed and has_identity:
        out = (torch.from_numpy(mult.astype(np.uint8)).to(anchors.device).contiguous(), ident)
    else:
        out = (None, None)
    if len(_TABLES) > 256:
        _TABLES.clear()
    _TABLES[key] = (weakref.ref(anchors), out)
    return out


_MULTINV = {}


def _group_tables_inverse(mult):
    """multinv[r][a'] = a with mult[r][a] = a' (the inverse permutation of every row), cached per table."""
    key = (id(mult), mult._version)
    hit = _MULTINV.get(key)
    if hit is not None and hit[0]() is mult:
        return hit[1]
    na = mult.shape[0]
    multinv = torch.empty_like(mult)
    multinv.scatter_(1, mult.long(), torch.arange(na, device=mult.device, dtype=torch.uint8).repeat(na, 1))
    if len(_MULTINV) > 256:
        _MULTINV.clear()
    _MULTINV[key] = (weakref.ref(mult), multinv)
    return multinv


_COSETS = {}
STORE_ORDER_COLUMNS = True     # streamed forward: the transposed intermediate's columns in the grouping kernel's store order


def _coset_tables(table, ident):
    """For a byte table of LEFT multiplications of an anchor group (table[r][a] = index of g_r . a for some bijection
    r -> g_r: `mult` or its row-wise inverse), a re-ordering of the anchors that turns every row into block moves:

        order [4*nb]   anchor index at coset-major position i: blocks of 4 = left cosets a.H of a Klein four-group
                       H = {e, h1, h2, h3} (h_i h_j = h_{i ^ j}), position j of a block = a.h_j;
        code [na, 16]  for row r and block b: sigma | x << 4 with table[r][order[4 b + j]] == order[4 sigma + (j ^ x)]

    (left multiplication maps left cosets onto left cosets; inside a block it multiplies the H-part: an index XOR).  A
    kernel that keeps the anchor axis of its LDS operand in `order` reads the four permuted anchors of a block as ONE
    16-byte word + a shuffle (csrc/so3_inter_inv.hip, COSET; csrc/so3_inter_lists2.hip, PERM).  -> (order uint8 [64] padded
    with the last anchor, code uint8 [na,16], pos uint8 [64] = position of every anchor in `order`) on the table's device, or
    None when the group has no such subgroup / the structure check fails."""
    key = (id(table), table._version, int(ident))
    hit = _COSETS.get(key)
    if hit is not None and hit[0]() is table:
        return hit[1]
    T = table.detach().cpu().numpy().astype(np.int64)
    na = T.shape[0]
    out = None
    if na % 4 == 0 and na // 4 <= 16:
        elem = T[:, ident]                                   # row r multiplies by the element with this anchor index
        row_of = np.empty(na, np.int64)
        row_of[elem] = np.arange(na)
        times = lambda a, b: int(T[row_of[a], b])            # a . b as anchor indices
        invol = [a for a in range(na) if a != ident and times(a, a) == ident]
        H = None
        for i, h1 in enumerate(invol):
            for h2 in invol[i + 1:]:
                if times(h1, h2) == times(h2, h1) and times(h1, h2) not in (ident, h1, h2):
                    H = [ident, h1, h2, times(h1, h2)]
                    break
            if H:
                break
        if H:
            # blocks that belong together stay together: the normaliser K of H (the tetrahedral subgroup of the icosahedral
            # group, K / H cyclic of order 3) -- a left multiplication maps the three H-cosets of a K-coset onto the three
            # H-cosets of ONE other K-coset, i.e. three of a 16-anchor group's four source blocks are neighbours in memory
            inv = {a: next(b for b in range(na) if times(a, b) == ident) for a in range(na)}
            K = [g for g in range(na) if sorted(times(times(g, h), inv[g]) for h in H) == sorted(H)]
            reps, covered = [], set()
            for k in K:
                if k not in covered:
                    reps.append(k)
                    covered.update(times(k, h) for h in H)
            order, seen = [], set()
            for a in range(na):
                if a not in seen:
                    for k in reps:
                        blk = [times(times(a, k), h) for h in H]
                        if blk[0] not in seen:
                            order += blk
                            seen.update(blk)
            pos = np.empty(na, np.int64)
            pos[order] = np.arange(na)
            code = np.zeros((na, 16), np.uint8)
            ok = len(order) == na
            for r in range(na):
                for b in range(na // 4):
                    src = pos[T[r, order[4 * b]]]
                    sigma, x = src >> 2, src & 3
                    code[r, b] = sigma | (x << 4)
                    ok = ok and all(T[r, order[4 * b + j]] == order[4 * sigma + (j ^ x)] for j in range(4))
            if ok:
                padded = np.asarray(order + [order[-1]] * (64 - na), np.uint8)
                where = np.zeros(64, np.uint8)
                where[:na] = pos
                out = (torch.from_numpy(padded).to(table.device), torch.from_numpy(code).to(table.device).contiguous(),
                       torch.from_numpy(where).to(table.device))
    if len(_COSETS) > 256:
        _COSETS.clear()
    _COSETS[key] = (weakref.ref(table), out)
    return out


def rotated_kernels(anchors, kernels):
    """rk [na,ks,3] = A_a kappa_k  (functional.py:L2519)."""
    return torch.matmul(anchors, kernels.transpose(0, 1)).permute(0, 2, 1).contiguous()


class InterWeights:
    """Lazy stand-in for the reference's inter_w [b,p,na,ks,nn] (functional.py:L2508-2549)."""

    def __init__(self, gx, rk, sigma, r=None):
        # (float64 regime: gx is g float64 [b,p,nn,3] and r int32 [b,p,nn] the nearest-anchor index beside it)
        self.gx, self.rk, self.sigma, self.r = gx, rk, float(sigma), r

    @property
    def shape(self):
        b, p, nn, _ = self.gx.shape
        return torch.Size((b, p, self.rk.shape[0], self.rk.shape[1], nn))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def materialize(self):
        if self.gx.dtype == torch.float64:
            return _hip.so3_inter_weights_f64(self.gx, self.rk, self.sigma)
        return _hip.so3_inter_weights(self.gx, self.rk, self.sigma)


def _inter_w(handle):
    """what a conv returns as inter_w: the lazy handle, or the tensor where MATERIALIZE_INTER_W asks for it"""
    return handle.materialize() if MATERIALIZE_INTER_W else handle


def _as_gx(grouped_xyz):
    """[b,3,p,nn] -> float4 [b,p,nn,4] with r = 0."""
    b, _, p, nn = grouped_xyz.shape
    gx = torch.zeros(b, p, nn, 4, dtype=torch.float32, device=grouped_xyz.device)
    gx[..., :3] = grouped_xyz.permute(0, 2, 3, 1)
    return gx


def inter_so3conv_grouping_anchor(grouped_xyz, anchors, kernels, sigma, interpolate='linear'):
    """grouped_xyz [b,3,p,nn] -> materialised w [b,p,na,ks,nn] = relu(1 - |g - A_a k|^2/sigma)
    (functional.py:L2508-2549)."""
    if interpolate != 'linear':
        raise NotImplementedError('kernel function %s is not implemented!' % interpolate)
    _hip.check_input(grouped_xyz)
    if _call_dtype('inter_so3conv_grouping_anchor', grouped_xyz=grouped_xyz, anchors=anchors, kernels=kernels) == torch.float64:
        return _hip.so3_inter_weights_f64(grouped_xyz.permute(0, 2, 3, 1).contiguous(), rotated_kernels(anchors, kernels), float(sigma))
    return _hip.so3_inter_weights(_as_gx(grouped_xyz), rotated_kernels(anchors, kernels), float(sigma))


# ------------------------------------------------------------------------------------------------
# autograd ops
# ------------------------------------------------------------------------------------------------
class _Group(torch.autograd.Function):
    """X = grouping.group(feats) as a node of its own (the functional grouping API); grouping: one of the pairs below (_ListGrouping,
    _MapGrouping, _IntraGrouping, _F64Args).  The backward is the pair's transpose.
    inter: new_feats[b,c,k,p,a] = sum_n feats[b,c,idx_n,perm_n(a)] w(p,a,k,n)  (functional.py:L1221-1261);
    intra: out[b,c,t,p,a] = feats[b,c,p,intra_idx[a,t]]  (functional.py:L2553-2602, L2606-2627 for the (na, 4) anchor axis)."""

    @staticmethod
    def forward(ctx, feats, grouping):
        feats = feats.contiguous()
        ctx.grouping, ctx.n = grouping, feats.shape[2]
        return grouping.group(feats, 0, feats.shape[0])

    @staticmethod
    def backward(ctx, gout):
        return ctx.grouping.group_transposed(gout.contiguous(), ctx.n, 0, gout.shape[0]), None


class _Contract(torch.autograd.Function):
    """y[b,o,pa] = W[o,ck] x[b,ck,pa] on the matrix cores (BasicSO3Conv, modules.py:L48-55)."""

    @staticmethod
    def forward(ctx, W, x, epilogue=None):
        W = W.contiguous()
        x = x.contiguous()
        b, ck, pa = x.shape
        o = W.shape[0]
        y = torch.empty(b, o, pa, dtype=torch.float32, device=x.device)
        if epilogue is not None:
            if not epilogue.inference:
                raise RuntimeError('a folded epilogue is an inference-time fusion: build and use it under torch.no_grad()')
            res = None if epilogue.residual is None else epilogue.residual.contiguous().view(b, o, pa)
            epilogue.applied = _hip.matmul_epilogue(W, x, y, epilogue.scale, epilogue.shift, epilogue.slope, res)
        if epilogue is None or not epilogue.applied:
            _hip.matmul(W, x, y)
        ctx.save_for_backward(W, x)
        return y

    @staticmethod
    def backward(ctx, gy):
        W, x = ctx.saved_tensors
        gy = gy.contiguous()
        b, ck, pa = x.shape
        o = W.shape[0]
        gW = gx = None
        if ctx.needs_input_grad[1]:
            gx = torch.empty_like(x)          # W^T gy : [ck,o] [o,pa]
            if _hip.SPLIT_BF16_CONTRACTION and ck >= 128 and ck % 128 == 0 and o % 16 == 0:
                Wt = W.t().contiguous()       # the split kernel reads its shared operand k-contiguous: [ck, o]
                _hip.matmul(Wt, gy, gx)
            else:
                _hip.matmul(W.t(), gy, gx)
        if ctx.needs_input_grad[0]:
            gW = torch.empty_like(W)          # sum_b gy_b x_b^T : [o,pa] [pa,ck]
            _hip.matmul_reduce(gy, x.transpose(1, 2), gW)
        return gW, gx, None


# Feature-gradient strategy of the fused inter convolution: "auto" picks the re-associated
# (inverse-list) path when at most 1/INV_ROW_FRACTION of the support points are referenced by
# any neighbour list, else dX = W^T dY followed by the transposed grouping.
BACKWARD_MODE = 'auto'      # 'auto' | 'inverse' | 'dx'
INV_ROW_FRACTION = 4


INV_LISTS_MAX_ROWS = 16384      # csrc/inv_lists.hip sorts a cloud's support rows in LDS


def _inv_lists_supported(idx, n_sup, na, ks):
    return na % 4 == 0 and ks <= 32 and n_sup <= INV_LISTS_MAX_ROWS and (idx.shape[1] * idx.shape[2]) % 4 == 0


_SIDE_STREAMS = {}      # the inverse neighbour lists are built beside the forward's grouping / contraction kernels


def _side_stream(dev, second=False):
    """the device's side stream; second: another one, for work that can run beside the side stream's own (_ListHead's look at a norm)"""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), second)
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


def _norm_ill(weight, bias):
    """-> int32 scalar tensor: 1 if a channel has gamma != 0 and |beta| > NORM_IN_NODE_MAX_RATIO |gamma| (exact: the ratio is a power of two)"""
    return ((bias.abs() > NORM_IN_NODE_MAX_RATIO * weight.abs()) & (weight != 0)).any().to(torch.int32)


class _ListHead:
    """First half of the inverse neighbour lists of idx [b,p,nn] (csrc/inv_lists.hip): per cloud the
    referenced support rows (longest list first), their counts and offsets -- all on the device -- plus an
    ASYNCHRONOUS copy of the numbers the launch decisions need on the host (the largest number of referenced rows of a
    cloud; whether any cloud carries non-identity relative rotations; whether any cloud cannot take the dense product).
    Built in the forward, read in the backward: by then the copy has long landed, so nothing stalls."""

    def __init__(self, idx, n_sup, nonident, gx=None, prefill=False, dense_probe=None, norm=None):
        """prefill (with gx): also the second half (csrc/inv_lists.hip fill: the entries of every referenced row) right away,
        for all rows -- the launch needs no host value that way.  Everything runs on a SIDE stream: these
        are small latency-bound kernels (0.3 + 0.45 ms per layer) that nothing in the forward waits for, and the grouping and
        contraction kernels that follow on the main stream leave them room; the backward waits for `event`.
        dense_probe = (rotation blocks or None, ...): also the membership bits of the dense product (csrc/so3_dense.hip) and
        whether every cloud can take it (no list names a row twice, at most min(n_sup, 1024) referenced rows, every given pose rotation
        EXACTLY the identity -- the dense operand has no rotation in it).  The row count is not known on the host yet, so a support of
        more than 512 rows is probed with the 32-word table (vgtk._hip.so3_dense_member); decide() narrows it once the count is known.
        norm = the BatchNormLeakyReLU of a TrainEpilogue that may join the node: whether one of its channels is too ill-conditioned for the
        backward from the output (NORM_IN_NODE_MAX_RATIO) is decided here on the device and travels in the same copy (norm_ill())."""
        dev = idx.device
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev)
        self.memb = None
        side.wait_stream(main)                            # idx / gx / nonident were produced on the main stream
        for t in (idx, gx, nonident) + tuple(x[1] if isinstance(x, tuple) else x for x in (dense_probe or ())):
            if t is not None:
                t.record_stream(side)                     # (read on the side stream: the allocator must not recycle them under it)
        ill = None
        poses = tuple(r for r in (dense_probe or ()) if r is not None and not isinstance(r, tuple))
        clouds = tuple(r[1] for r in (dense_probe or ()) if isinstance(r, tuple))
        norm_wb = (None, None) if norm is None else (norm.weight.detach(), norm.bias.detach())
        if len(clouds) <= 1 and _hip.so3_dense_probe_takes(poses, clouds[0] if clouds else None, *norm_wb):
            # the host's words from one entry (csrc/list_probe.hip); the tensor expressions below say what they are
            with torch.cuda.stream(side):
                self.rows, self.off, self.cnt, self.n_rows = _hip.inv_lists_rows(idx, n_sup)
                dflags = None
                if dense_probe is not None:
                    self.memb, dflags = _hip.so3_dense_member(idx, self.rows, self.n_rows, n_sup)
                stats = _hip.so3_dense_probe(idx.shape[1], self.n_rows, nonident, dflags, self.memb, poses, clouds[0] if clouds else None,
                                             *norm_wb, NORM_IN_NODE_MAX_RATIO)
                if norm is None:
                    stats = stats[:4]
                self._finish(stats, idx, gx, n_sup, prefill, side, main)
            return
        if norm is not None:
            # a handful of one-block kernels over the [o] parameters, on a stream of their own: they run beside the list kernels below, which
            # take far longer, so the copy the forward waits for arrives no later than without them
            second = _side_stream(dev, True)
            second.wait_stream(main)                      # (the optimizer's update of the parameters ran on the main stream)
            with torch.cuda.stream(second):
                ill = _norm_ill(norm.weight.detach(), norm.bias.detach())
            ill.record_stream(side)
        with torch.cuda.stream(side):
            self.rows, self.off, self.cnt, self.n_rows = _hip.inv_lists_rows(idx, n_sup)
            flag = nonident.max() if nonident is not None else torch.ones((), dtype=torch.int32, device=dev)
            dense_bad = torch.ones((), dtype=torch.int32, device=dev)
            if dense_probe is not None:
                self.memb, dflags = _hip.so3_dense_member(idx, self.rows, self.n_rows, n_sup)
                dense_bad = dflags.max()
                eye = torch.eye(3, dtype=torch.float32, device=dev)
                for rot in dense_probe:
                    if isinstance(rot, tuple):
                        # ('orthonormal', [b,3,3] one rotation per cloud): the plain product stands for R_rel = R R^T = I, which holds
                        # for an orthonormal block only -- a predicted, not-quite-orthonormal 3x3 must stay on the list kernels
                        # (they form R_p R_n^T as the reference does, so3conv/functional.py:L1112-1120)
                        r = rot[1].double()
                        dense_bad = dense_bad + ((torch.matmul(r, r.transpose(-1, -2)) - eye.double()).abs().max() > 1e-6).to(torch.int32)
                    elif rot is not None:
                        dense_bad = dense_bad + (rot[:, :, :3, :3] != eye).any().to(torch.int32)
            # how many 16-row groups of the referenced rows a point's list touches, averaged per cloud, the largest cloud average x 16:
            # what the dense product with listed k-steps executes is proportional to it (csrc/so3_dense.hip dense_keys_kernel)
            groups16 = torch.zeros((), dtype=torch.int32, device=dev)
            if self.memb is not None:
                touched = ((self.memb & 0xffff) != 0).sum((1, 2)) + ((self.memb & -65536) != 0).sum((1, 2))       # [b]
                groups16 = (touched.max().to(torch.float32) * (16.0 / max(idx.shape[1], 1))).to(torch.int32)
            stats = [self.n_rows.max().to(torch.int32), flag.to(torch.int32), dense_bad.to(torch.int32), groups16]
            if ill is not None:
                # (the forward waits for this copy on the host before it goes on: no later in-place update of the parameters can overtake
                # the read above)
                side.wait_stream(second)
                stats.append(ill)
            self._finish(torch.stack(stats), idx, gx, n_sup, prefill, side, main)

    def _finish(self, stats, idx, gx, n_sup, prefill, side, main):
        """(under the side stream) the copy of the words to the host, the second half of the lists where asked for, the event"""
        self.host = torch.empty(stats.shape[0], dtype=torch.int32, pin_memory=True)
        self.host.copy_(stats, non_blocking=True)
        self.entries = _hip.inv_lists_fill(idx, gx, self.rows, self.off, n_sup) if (prefill and gx is not None) else None
        self.event = torch.cuda.Event()
        self.event.record(side)
        for t in (self.rows, self.off, self.cnt, self.n_rows, self.memb) + (self.entries or ()):      # allocated under the side stream, used (and freed) under the main one
            if t is not None:
                t.record_stream(main)

    def fill(self, idx, gx, n_sup):
        """the second half of the lists after all (a forward that probed for the dense product and did not take it)"""
        dev = idx.device
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev)
        with torch.cuda.stream(side):
            self.entries = _hip.inv_lists_fill(idx, gx, self.rows, self.off, n_sup)
            self.event = torch.cuda.Event()
            self.event.record(side)
        for t in self.entries:
            t.record_stream(main)

    def wait(self):
        """the current stream waits for the lists (device side; no host stall)"""
        torch.cuda.current_stream(self.rows.device).wait_event(self.event)

    def _settle(self):
        """Wait for the host copy.  A probe at the wide width whose clouds reference at most 512 rows is narrowed here, once: `memb` becomes
        its first 16 words per point (words 16-31 are zero then), and everything downstream -- keys, point order, masks, step lists -- is what
        a support of at most 512 rows gets.  (The lists have run by now: the copy needs no wait on the side stream.)"""
        self.event.synchronize()
        if self.memb is not None and int(self.host[0]) <= _hip.DENSE_NARROW_ROWS:
            self.memb = _hip.so3_dense_narrow(self.memb, _hip.DENSE_NARROW_ROWS)

    def decide(self):
        """-> (rcap, any_nonident) as Python values."""
        self._settle()
        rcap, flag = self.host[:2].tolist()
        return int(rcap), bool(flag)

    def norm_ill(self):
        """a channel of the `norm` given to __init__ has gamma != 0 and |beta| > NORM_IN_NODE_MAX_RATIO |gamma| (False without a norm);
        blocks on the host like decide() -- the forward has waited for that copy already when it asks"""
        if self.host.shape[0] <= 4:
            return False
        self._settle()
        return int(self.host[4]) != 0

    def groups_touched(self):
        """mean number of 16-row groups a point's list touches (the largest per-cloud mean); blocks on the host like decide()"""
        self._settle()
        return int(self.host[3]) / 16.0

    def dense_possible(self):
        """every cloud can take the dense product (see __init__); blocks on the host like decide()"""
        self._settle()
        return self.memb is not None and int(self.host[2]) == 0


def _inverse_lists(idx, gx, n_sup, ident, nonident=None):
    """Inverse neighbour lists of idx [b,p,nn] (which (point, slot) pairs reference each support row), the
    referenced rows compacted and ordered longest list first; entries of a row in (p, slot) order.
    Convenience form for tests and tools (blocks on the host for the row count); the fused conv uses
    _ListHead + _hip.inv_lists_fill without blocking.
    -> rows, off, cnt int32 [b,rcap]; ent_p int32 [b,p*nn]; ent_gx [b,p*nn,4]; rcap; all_ident."""
    if nonident is None:
        nonident = (gx[..., 3].contiguous().view(torch.int32) != ident).flatten(1).any(1).to(torch.int32)
    head = _ListHead(idx, n_sup, nonident)
    rcap, any_nonident = head.decide()
    head.wait()
    ent_p, ent_gx = _hip.inv_lists_fill(idx, gx, head.rows, head.off, rcap)
    return (head.rows[:, :rcap].contiguous(), head.off[:, :rcap].contiguous(), head.cnt[:, :rcap].contiguous(),
            ent_p, ent_gx, rcap, not any_nonident)


# Layout of the fused conv's intermediate X (where the kernels allow it, else the reference layout); the contraction
# is always a hand-written GEMM:
#   'transposed'  X as the plain [P*A, C*K] matrix, both GEMM operands k-contiguous: csrc/gemm_dma_f32.hip
#                 (141 TFLOP/s on the deepest layer; hipBLASLt on the same operands: 150 -- tools/gemm_only.py times both)
#   'blocked'     X blocked by anchor quads, contraction = csrc/gemm_f32.hip (eap_gemm_f32_xb)
#   'reference'   X [C*K, P*A] as the reference's einsum writes it
X_LAYOUT = 'transposed'


# The intermediate X [B, C*K, P*A] of the fused conv (24 GB at C = 128, B = 8) is scratch, not state: the re-associated
# backward never reads it, so it is produced and consumed X_CHUNK_CLOUDS clouds at a time and never saved.  Only the
# textbook backward (many referenced rows) needs it for dW = dY X^T; which regime a layer is in is known on the host
# only when its backward runs, so the layer's previous decision is the hint: after a 'dx' backward the next forward of
# the same weights keeps X, and a wrong guess costs one re-run of the grouping kernel in the backward.
X_CHUNK_CLOUDS = 8   # measured: 2 / 4 / 8 clouds per slab = 146.8 / 146.9 / 145.6 ms per step
_KEEP_X_HINT = {}           # id(W) -> (weakref(W), bool)


def _keep_x_hint(W):
    hit = _KEEP_X_HINT.get(id(W))
    return bool(hit is not None and hit[0]() is W and hit[1])


def _set_keep_x_hint(W, keep):
    if len(_KEEP_X_HINT) > 1024:
        _KEEP_X_HINT.clear()
    _KEEP_X_HINT[id(W)] = (weakref.ref(W), bool(keep))


class FoldedEpilogue:
    """What an inference-mode BatchNorm2d + leaky_relu (+ skip sum) after a contraction amounts to: per output channel
    y = leaky_relu(scale * (W x) + shift, slope) (+ residual) (vgtk.so3conv.blocks.BatchNormLeakyReLU.folded).  A
    contraction that can apply it in its own epilogue (csrc/gemm_bf16x3.hip) sets `applied`; otherwise the caller runs
    the norm as a pass of its own."""

    def __init__(self, scale, shift, slope, residual=None):
        self.scale, self.shift, self.slope, self.residual = scale.contiguous(), shift.contiguous(), float(slope), residual
        self.applied = False
        self.inference = not torch.is_grad_enabled()      # made under torch.no_grad(): the only place it may be applied


class TrainEpilogue:
    """A TRAINING-mode BatchNorm2d + leaky_relu right behind an inter conv (vgtk.so3conv.blocks.conv_norm_act; `x = conv(x); feat =
    relu(norm(x.feats))`, SPConvNets/utils/base_so3poseconv.py:L205-222).  When the conv's forward runs the dense product it takes the
    normalisation into its own node and sets `applied`:
      forward   product -> Yt -> statistics pass over Yt -> the re-ordering pass writes y' = leaky(BatchNorm(y)) (no pass of the norm's own,
                the conv output y is never written);
      backward  one reduction pass over (dL/dy', y') -> the gradient behind the norm is formed WHILE it is split into the backward product's
                planes (never written either).  The pre-activation is recovered from y' (leaky_relu with a positive slope is invertible):
                the node keeps its output, not the conv output.
    A conv with at most 32 contraction indices C*K whose input needs no gradient (the first layer) takes the norm into its node too, regime
    'narrow input' (_forward_narrow): it keeps the grouped input X and recomputes the conv output from it in every pass.
    Otherwise (list kernels, posed parts, ...) `applied` stays False and the caller runs the norm module as a pass of its own.
    A channel whose gamma is exactly 0 has a constant output: its input gradient is exactly 0 either way, its d gamma is reported as 0.
    Conditioning: the recovery (pre - beta) / gamma is a float32 subtraction of two numbers of size |beta| that leaves one of size
    |gamma xhat|, so xhat comes back with an absolute error of up to 8 x 2^-24 (|xhat| + |beta / gamma| + |mean| invstd) per channel, and
    d gamma, d beta and gx with the sums of it (tests/test_fused_norm_host.py derives the bound, tests/test_gpu_conv_norm_conditioning.py
    holds the kernels and the node to it channel by channel).  A layer with a channel that has gamma != 0 and |beta| >
    NORM_IN_NODE_MAX_RATIO |gamma| (128) therefore does NOT take the norm into the dense node: `applied` stays False.  The flag is formed
    on the device beside _ListHead's host words and arrives in the copy the forward waits for anyway; gamma = 0 does not raise it.  The
    'narrow input' node recomputes xhat from X and is free of the effect."""

    def __init__(self, norm):
        self.norm = norm
        self.applied = False
        self.inference = False
        self.residual = None

    def moments(self, s1, s2, pivot, count):
        """pivoted sums of the conv output per channel -> (scale, shift, slope) of the fused pass; updates the running statistics exactly as
        vgtk.so3conv.blocks._BNAct.forward does; leaves what the backward needs in self.saved"""
        norm = self.norm
        gamma = norm.weight.detach().double()
        scale, shift, mean, invstd, total = norm_fold.fold((s1, s2, pivot, count), gamma, norm.bias.detach(), norm.running_mean, norm.running_var,
                                                           True, norm.momentum, norm.eps, sync=norm.sync)
        self.stats = (mean, invstd)          # float64 [o]: what a node that recomputes the conv output normalises with in its backward
        inv_gamma = torch.where(gamma == 0, torch.zeros_like(gamma), 1.0 / gamma).float()
        # (copies, not views of the parameters: the backward must see the values this forward normalised with)
        self.saved = (scale, norm.bias.detach().float().clone(), inv_gamma.contiguous(), total)
        return scale.contiguous(), shift.contiguous(), float(norm.negative_slope)

    def takes_partials(self, t):
        """the moments of `t`'s node come from moments_from_partials: the switch is on, the tensors are on the device, and no exchange stands
        between the sums and the coefficients (SyncBatchNorm over several ranks keeps the tensor expressions of `moments`)"""
        norm = self.norm
        return bool(_hip.NATIVE_NORM_GLUE and t.is_cuda and not norm_fold._syncing(norm.sync) and norm.weight.dtype == torch.float32
                    and norm.bias.dtype == torch.float32 and (norm.running_mean is None or norm.running_mean.dtype == torch.float32))

    def moments_from_partials(self, ps, pq, pivot, count):
        """`moments` from the partial sums float32 [o, parts] as the statistics kernels leave them and a float32 pivot (any stride), in one
        launch (csrc/norm_fold.hip: the same float64 arithmetic; the partials are summed there).  Same results, same self.stats / self.saved."""
        norm = self.norm
        running = (None, None) if norm.running_mean is None else (norm.running_mean, norm.running_var)
        scale, shift, mean, invstd, beta, inv_gamma = _hip.norm_fold_train(ps, pq, pivot, count, norm.weight.detach().contiguous(),
                                                                          norm.bias.detach().contiguous(), norm.eps, norm.momentum, *running)
        self.stats = (mean, invstd)
        self.saved = (scale, beta, inv_gamma, count)
        return scale, shift, float(norm.negative_slope)


def _contract_into(W, x, y, layout, epilogue=None, b0=0, x_bound=None):
    """y[b,o,pa] = W . x for the intermediate in one of its three layouts (epilogue: see FoldedEpilogue; b0 = first
    cloud of this slab, for the residual; x_bound = (words [b, p], anchors per point, factor) bounding x per point, see
    _grouped_bound)."""
    b, c, ks, p, na = x.shape
    o = W.shape[0]
    if layout == 2:
        xt = x.view(b, p * na, c * ks).transpose(1, 2)  # the memory behind the nominal shape is X^T [b, pa, ck]
    if epilogue is not None and layout == 2:
        res = None if epilogue.residual is None else epilogue.residual[b0:b0 + b]
        if _hip.matmul_epilogue(W, xt, y, epilogue.scale, epilogue.shift, epilogue.slope, res, b_bound=x_bound):
            epilogue.applied = True
            return
        if b0 > 0 and epilogue.applied:
            raise RuntimeError('folded epilogue: the slabs of one contraction took different kernels')
    if layout == 2:                              # Y = W . (X^T)^T, both operands k-contiguous (csrc/gemm_dma_f32.hip)
        _hip.matmul(W, xt, y, b_bound=x_bound)
    elif layout == 1:                            # blocked by 4: a storage without strides to read the numbers from -- the positional call
        _hip.gemm(0, 0, o, p * na, c * ks, W, c * ks, 0, x, p * na, c * ks * p * na, y, p * na, o * p * na, b, b_blocked=True)
    else:
        _hip.matmul(W, x.view(b, c * ks, p * na), y)


def _grouped_bound(feats, idx):
    """A bound on the grouped tensor per point without a pass over it: X[c,k,p,a] = sum over the neighbours of a feature times
    an interpolation weight in [0, 1] (so3conv/functional.py:L1112-1261), so |X[.,.,p,.]| <= sum_n max_{c,a} |feats[c,idx[p,n],a]|
    -- the two-plane contraction takes the scales of its operand's columns from it (vgtk/_hip.py SPLIT_PLANES).
    -> int32 [b, p] (float bit patterns) or None."""
    if not (_hip.SPLIT_BF16_CONTRACTION and _hip.SPLIT_PLANES == 2):
        return None
    return _hip.so3_grouped_bound(feats, idx)


BACKWARD_LOG = None      # a list while someone wants to know the backward regime of every inter conv (bench.py, tests)
FORWARD_LOG = None       # the same for the forward: {'channels', 'dense': the dense product ran, 'parts'}


# The dense product over the referenced rows (csrc/so3_dense.hip): 'auto' takes it when every cloud of the batch can (no pose
# rotation, no padded lists) and a cloud references few enough rows: it does rows / nsample times the flops of the list kernels on
# a pipe ~4.5 x as fast.  Both directions take it up to DENSE_ROW_FACTOR x nsample rows at any width it supports ('off' never; 'force'
# whenever the shapes are taken: tests).
DENSE_MODE = os.environ.get('EAP_DENSE', 'auto')      # (a numerics mode, README.md "Numerics": 'off' = the fp32 list kernels)
DENSE_ROW_FACTOR = 5.0
# ... and beyond that row count (up to the 1024 row slots the wide membership words hold) while a point's list touches few enough 16-row groups: with
# the listed k-steps the product executes ~ groups_touched x 16 / nsample times the algorithmic flops (x 3 on the fp16 pipe at ~1.3 PFLOP/s)
# against the list kernels' 0.46 of the fp32 peak -- it wins below ~24 groups; 16 leaves margin for the per-block overheads
DENSE_MAX_GROUPS = 16.0
# the same bound for clouds of more than 512 referenced rows (the 32-word tables); a knob of its own so that it can be raised for them alone.
# Measured at 24 (the 64 -> 128 layer of 8 x 4096-point clouds with the 512-point radii, ~21 groups touched): the 128-row product costs what
# the list kernels cost and the leg does not gain (profiles/dense_wide_rows.txt) -- 16 stays
DENSE_MAX_GROUPS_WIDE = 16.0
# the forward at widths that fill 128-row blocks only (the 64 -> 128 layer): with every k-step it tied with grouping + contraction
# (round 5: 9.0 against 9.1 ms); with the empty k-steps skipped (round 6) the product wins: 4.2 + 1.3 + 0.9 ms against 5.7 + 3.3, same run
# 129.2 against 128.0 clouds/s before the operand kernel, more after it
DENSE_FWD_NARROW = True
# a training-mode BatchNorm + leaky_relu behind a conv whose forward runs the dense product joins the conv's node (TrainEpilogue)
FUSE_CONV_NORM = True
# ... unless one of its channels has gamma != 0 and |beta| > NORM_IN_NODE_MAX_RATIO |gamma|.  The node's backward recovers xhat from the
# OUTPUT, (pre - beta) / gamma in float32: an absolute error of up to 8 x 2^-24 (|xhat| + |beta / gamma| + |mean| invstd), typically a
# quarter of that (derived and emulated in tests/test_fused_norm_host.py).  At 128 the typical loss 2 x 2^-24 (max |xhat| + 128) ~ 1.6e-5
# reaches the 2e-5 the suite grants d gamma / d beta anywhere; the separate module normalises the stored conv output and has no such term.
NORM_IN_NODE_MAX_RATIO = 128.0


def _dense_rows(rcap, n):
    """row slots of the dense product: whole groups of 16 (csrc/so3_dense.hip, dense index)"""
    return (rcap + 15) & ~15


def _dense_wanted(head, o, p, na, ks, nn, n):
    """-> (rp, forward too): rows per cloud of the dense product (0: not taken) and whether the forward takes it as well.
    Blocks on the host for the row count."""
    if DENSE_MODE == 'off' or head is None or head.memb is None:
        return 0, False
    rcap, _ = head.decide()
    rp = _dense_rows(rcap, n)
    if rp <= 0 or rp > n or not head.dense_possible() or not _hip.so3_dense_supported(p, na, ks, rp, o):
        return 0, False
    if DENSE_MODE == 'force':
        return rp, True
    if rp > DENSE_ROW_FACTOR * nn and not (rp <= _hip.DENSE_MAX_ROWS and
                                           head.groups_touched() <= (DENSE_MAX_GROUPS if rp <= _hip.DENSE_NARROW_ROWS else DENSE_MAX_GROUPS_WIDE)):
        return 0, False
    return rp, (o % 256 == 0) or DENSE_FWD_NARROW


def _weight_grad_from_z(z, fc, b, c, o, ks, ra, ldz=None):
    """dW[o,(c,k)] = sum_{b,(r,a)} Z[b,o,k,(r,a)] Fc[b,c,(r,a)] for Z [b, o*ks, ra] (row pitch ldz >= ra) and the referenced feature
    rows Fc [b, c, ra] (any order of the (row, anchor) axis, the same in both)."""
    ldz = ra if ldz is None else ldz
    # (measured and dropped: 64 feature channels zero-padded to 128 rows to reach the split kernel -- 0.66 -> 0.53 ms per step, and the
    # kernel-against-kernel bar of tests/test_gpu_lists_and_modules.py::test_permuted_clouds_on_the_two_tile_kernel, 2e-6, went to 3.2e-6)
    z = z.view(b, o * ks, ldz)[..., :ra]
    dt = torch.empty(c, o * ks, dtype=torch.float32, device=z.device)
    if _hip.matmul_reduce_takes_split(fc, z.transpose(1, 2), dt):
        # the transposed product Fc_b Z_b^T [c, o*ks] has the tile shape the split-bf16 kernel takes (>= 128 rows,
        # >= 256 columns); Z_b Fc_b^T with its 64-128 columns would stay on the fp32 pipe
        _hip.matmul_reduce(fc, z.transpose(1, 2), dt)
        return dt.view(c, o, ks).permute(1, 0, 2).reshape(o, c * ks).contiguous()
    d = dt.view(o * ks, c)                                              # sum_b Z_b Fc_b^T in the same o*ks*c floats
    _hip.matmul_reduce(z, fc.transpose(1, 2), d)
    return d.view(o, ks, c).permute(0, 2, 1).reshape(o, c * ks).contiguous()


# Posed clouds whose points carry ONE rotation per rigid part (articulated objects: every point takes the pose of its part): the
# reference rotates an entry's offset by R_rel = R_p R_r^T and permutes the neighbour's anchor axis by the group element nearest to
# R_rel (so3conv/functional.py:L1112-1160; csrc/so3_inter.hip so3_prep_kernel) -- both depend on (part of p, part of r) only.  The dense
# product then runs once per part over that part's query points: its k-side table takes R_rel^T per ROW (a row's part is fixed), the
# stored operand is built from the rows' features with their anchor axis permuted per row.  DENSE_MAX_PARTS bounds the launches.
DENSE_MAX_PARTS = 6
_POSE_PARTS = {}            # (storage pointer, version, shape) of a pose tensor -> (weakref, _PoseParts or None)


class _PoseParts:
    """The points of every cloud grouped by their pose rotation (bit-equal 3x3 blocks): part slots 0 .. n-1 per cloud, largest part
    first; slot i of the batch is one launch over pts[i] int64 [b, p_i] (p_i = the largest part i of any cloud rounded to 32;
    entries past a cloud's own part size repeat a valid point and are marked in col_map[i] int32 [b, p_i] = -1)."""

    def __init__(self, labels, reps, sizes, p):
        dev = labels.device
        b = labels.shape[0]
        self.labels, self.reps, self.sizes, self.n = labels, reps, sizes, len(sizes[0])
        self.single = self.n == 1
        order = torch.argsort(labels, dim=1, stable=True)                   # points sorted by part
        self.pts, self.col_map, self.width = [], [], []
        start = [0] * b
        for i in range(self.n):
            width = (max(sizes[bi][i] for bi in range(b)) + 31) // 32 * 32
            st = torch.tensor(start, dtype=torch.int64, device=dev)[:, None]
            sz = torch.tensor([sizes[bi][i] for bi in range(b)], dtype=torch.int64, device=dev)[:, None]
            t = torch.arange(width, dtype=torch.int64, device=dev)[None, :]
            valid = t < sz
            pts = order.gather(1, (st + torch.where(valid, t, torch.zeros_like(t))).clamp(max=p - 1))
            self.pts.append(pts.contiguous())
            self.col_map.append(torch.where(valid, pts, torch.full_like(pts, -1)).to(torch.int32).contiguous())
            self.width.append(width)
            start = [start[bi] + sizes[bi][i] for bi in range(b)]


def _pose_parts(rot):
    """-> _PoseParts of pose [b,p,4,4], or None when a cloud has more than DENSE_MAX_PARTS distinct rotations.  One host read per pose
    tensor (remembered by tensor identity + version: the layers of a backbone share their poses)."""
    key = (rot.data_ptr(), rot._version, tuple(rot.shape))
    hit = _POSE_PARTS.get(key)
    if hit is not None and hit[0]() is rot:
        return hit[1]
    b, p = rot.shape[:2]
    dev = rot.device
    r9 = rot[:, :, :3, :3].reshape(b * p, 9).contiguous()
    bits = r9.view(torch.int32).to(torch.int64)
    mul = torch.tensor([0x9E3779B97F4A7C15 - (1 << 64), 0xC2B2AE3D27D4EB4F - (1 << 64), 0x165667B19E3779F9, 0x27D4EB2F165667C5, 0x85EBCA77C2B2AE63 - (1 << 64),
                        0x2545F4914F6CDD1D, 0x5851F42D4C957F2D, 0x14057B7EF767814F, 0x3C6EF372FE94F82B], dtype=torch.int64, device=dev)
    h = (bits * mul).sum(1)
    h = (h ^ (h >> 31)) & ((1 << 55) - 1)
    keys = h + (torch.arange(b, dtype=torch.int64, device=dev).repeat_interleave(p) << 55)
    uniq, inv, counts = torch.unique(keys, return_inverse=True, return_counts=True)     # (sorted: a cloud's parts are consecutive)
    result = None
    if uniq.numel() <= b * DENSE_MAX_PARTS:
        nu = uniq.numel()
        first = torch.full((nu,), b * p, dtype=torch.int64, device=dev).scatter_reduce(0, inv, torch.arange(b * p, dtype=torch.int64, device=dev), 'amin')
        rep = r9[first]                                                                     # [nu, 9]
        same = (rep[inv] == r9).all().to(torch.int64)                                       # (a hash collision would show here)
        host = torch.cat([same[None], uniq >> 55, counts]).tolist()
        ok, cloud, cnt = host[0], host[1:1 + nu], host[1 + nu:]
        per = [[] for _ in range(b)]
        for u in range(nu):
            per[cloud[u]].append((cnt[u], u))
        n = max(len(x) for x in per)
        if ok and n <= DENSE_MAX_PARTS and min(len(x) for x in per) >= 1:
            slot = [0] * nu
            sizes = [[0] * n for _ in range(b)]
            rep_idx = [[per[bi][0][1]] * n for bi in range(b)]
            for bi in range(b):
                for i, (c_, u) in enumerate(sorted(per[bi], key=lambda x: (-x[0], x[1]))):
                    slot[u], sizes[bi][i], rep_idx[bi][i] = i, c_, u
            labels = torch.tensor(slot, dtype=torch.int64, device=dev)[inv].view(b, p)
            reps = rep[torch.tensor(rep_idx, dtype=torch.int64, device=dev)].view(b, n, 3, 3)
            result = _PoseParts(labels, reps, sizes, p)
    if len(_POSE_PARTS) > 16:
        _POSE_PARTS.clear()
    _POSE_PARTS[key] = (weakref.ref(rot), result)
    return result


class _PartsDense:
    """Per part slot of a _PoseParts: the dense product's geometry over that part's query points (row rotations in its k-side table)
    and the per-row anchor permutation of the stored operand."""

    def __init__(self, parts, xyz, memb, rows, rp, rk, sigma, nn, n_rows, mult, anchors):
        b, p = parts.labels.shape
        dev = xyz.device
        self.parts, self.rp, self.ks, self.na = parts, int(rp), rk.shape[1], rk.shape[0]
        ld = rows.stride(0)
        rows_all = torch.as_strided(rows, (b, ld), (ld, 1))
        row_part = parts.labels.gather(1, rows_all.clamp(min=0, max=p - 1).long())                     # [b, ld] (empty slots: anything)
        R_row = parts.reps.double().gather(1, row_part[:, :, None, None].expand(b, ld, 3, 3))        # R_j of every row slot
        self.geo, self.perm = [], []
        A = anchors.double() if anchors is not None else None
        for i in range(parts.n):
            R_i = parts.reps[:, i].double()                                                           # [b,3,3]
            M = torch.matmul(R_row, R_i[:, None].transpose(-1, -2))                                   # R_rel^T = R_j R_i^T   [b,ld,3,3]
            pts = parts.pts[i]
            q_xyz = xyz.gather(2, pts[:, None, :].expand(b, 3, pts.shape[1])).contiguous()
            valid = (parts.col_map[i] >= 0)
            memb_i = (memb.gather(1, pts[:, :, None].expand(b, pts.shape[1], memb.shape[2])) * valid[:, :, None].to(memb.dtype)).contiguous()
            self.geo.append(_hip.DenseGeometry(q_xyz, xyz, memb_i, rows, rp, rk, sigma, nn, n_rows, row_rot=M.float().contiguous()))
            if mult is None:
                self.perm.append(None)
            else:
                # the group element nearest to R_rel = M^T: argmax_g tr(R_rel A_g) (so3_prep_kernel; first maximum)
                t = torch.einsum('brji,gji->brg', M[:, :rp], A)
                ridx = t.float().argmax(dim=2)                                                        # [b,rp]
                self.perm.append(mult.long()[ridx])                                                   # [b,rp,na]: F_i[.., r, a] = F[.., r, perm[r, a]]


def _dense_g(fc4, W, geo):
    """G = W F over the referenced rows as the dense forward's stored operand: fc4 [b,c,rp,na] -> (g [b,o,ks,ld], ld or None, None), or
    (None, None, (scale, planes)) when one kernel made the operand directly (vgtk._hip.so3_dense_gplanes).  The
    small GEMM runs on the split-operand kernels where its shapes allow: its columns (row, anchor) padded to whole 128-column
    tiles (the padding of F is zero, G's padded columns are skipped by the split that follows)."""
    b, c, rp, na = fc4.shape
    o, ks = W.shape[0], geo.ks
    ra = rp * na
    W3 = W.view(o, c, ks).permute(0, 2, 1).reshape(o * ks, c).contiguous()
    operand = _hip.so3_dense_gplanes(fc4, W3, geo)        # (round 6: product and planes in one kernel where the shape is taken)
    if operand is not None:
        return None, None, operand
    ld = _hip.dense_pitch(ra) if (c % 16 == 0 and c >= 16 and (o * ks) % 128 == 0) else ra
    if ld == ra:
        fc = fc4.reshape(b, c, ra)                                                  # [b,c,(r,a)]; empty slots: zeros
    else:
        fc = torch.zeros(b, c, ld, dtype=torch.float32, device=fc4.device)
        fc[:, :, :ra] = fc4.reshape(b, c, ra)
    g = torch.empty(b, o * ks, ld, dtype=torch.float32, device=fc4.device)
    _hip.matmul(W3, fc, g)
    return g.view(b, o, ks, ld), (None if ld == ra else ld), None


def _dense_operand(feats, W, rows, geo):
    """the dense forward's stored operand from the support features: _dense_g over the referenced rows"""
    return _dense_g(_hip.rows_gather(feats, rows, geo.rp), W, geo)


def _dense_forward_parts(feats, W, rows, pd, p):
    """the dense forward of posed clouds, one launch per part slot (see _PartsDense) -> y [b,o,p,a]"""
    b, c, n, na = feats.shape
    o = W.shape[0]
    fc0 = _hip.rows_gather(feats, rows, pd.rp)                                      # [b,c,rp,na]
    y = torch.empty(b, o, p, na, dtype=torch.float32, device=feats.device)
    for i, geo in enumerate(pd.geo):
        perm = pd.perm[i]
        fc4 = fc0 if perm is None else fc0.gather(3, perm[:, None].expand(b, c, pd.rp, na))
        g, ldg, operand = _dense_g(fc4, W, geo)
        _hip.so3_dense_fwd(g, geo, pd.parts.width[i], c, ldg=ldg, out=y, col_map=pd.parts.col_map[i], operand=operand, o=o)
    return y


def _dense_forward(feats, W, rows, geo, p):
    """y [b,o,p,a] = sum_(k,r) G[o,(k,r),a] Wd[p,(k,r),a] with G = W F over the referenced rows (csrc/so3_dense.hip)."""
    g, ldg, operand = _dense_operand(feats, W, rows, geo)
    return _hip.so3_dense_fwd(g, geo, p, feats.shape[1], ldg=ldg, operand=operand, o=W.shape[0])


class _InterConvArgs:
    """The inputs of _InterConv that carry no gradient, as one record, made where the conv is called."""

    def __init__(self, idx, gx, rk, mult, sigma, ident, nonident=None, anchors=None, epilogue=None, geometry=None, amap=None, shift=None):
        self.idx, self.gx, self.rk, self.mult, self.sigma, self.ident, self.nonident = idx, gx, rk, mult, float(sigma), ident, nonident
        # amap uint8 [b,p,nn,na]: the per-entry anchor map of an anchor set that is not a group (_anchor_map) -- the 'anchor map' regime
        self.amap = amap
        # shift uint8 [b,p,nn]: the per-entry residual index of the `use_2d` variant, really permuted (_conv_2d) -- the 'residual map'
        # regime: feats [b,c,n,na*4], rk [na*4,ks,3]
        self.shift = shift
        self.anchors = anchors.detach().contiguous() if (anchors is not None and mult is not None) else None   # the rotations `mult` was built from
        # epilogue: a FoldedEpilogue or a TrainEpilogue;
        # geometry = (q_xyz, xyz, q_rot, rot): what the dense product over the referenced rows is built from (csrc/so3_dense.hip)
        self.epilogue, self.geometry = epilogue, geometry
        # torch.is_grad_enabled() AT THE CALL (inside forward() autograd always has it off; and under torch.no_grad()
        # needs_input_grad still reports the parameters although nothing will be differentiated)
        self.grad_mode = torch.is_grad_enabled()


class _DensePlan:
    """Whether an inter conv takes the dense product over its referenced rows, decided once in the forward: rp = row slots per cloud (0: not
    taken), forward = the forward runs it too (else the backward alone), parts = the _PoseParts when it runs once per rigid part, probed = the
    batch was probed for it; head = the _ListHead of the neighbour lists (None when neither the probe nor a backward needs one)."""

    def __init__(self, args, n, o, lists_ok, needs_grad, keep, folded, norm=None):
        # (folded: the FoldedEpilogue of an inference call or None; norm: the module of a TrainEpilogue that joins the node if the forward
        # runs the product -- the probe then also looks at its conditioning, _ListHead.norm_ill)
        # whether the batch can take the product is known on the host once the lists' first half has run -- one host wait per layer,
        # only for layers whose width fills the dense kernel's blocks
        idx, geometry = args.idx, args.geometry
        p, nn = idx.shape[1], idx.shape[2]
        na, ks = args.rk.shape[0], args.rk.shape[1]
        self.args, self.parts, self._geo = args, None, None
        probe = None
        # (a folded inference epilogue does not stop it: the dense forward's re-ordering pass applies it; posed parts leave
        # `epilogue.applied` False and the caller runs the norm as a pass of its own)
        # (without gradients only the forward can use the product, and 'auto' takes it at o % 256 == 0 only: no probe -- and no host wait --
        # for an inference call it could not change)
        if (DENSE_MODE != 'off' and geometry is not None and lists_ok and (folded is None or o % 256 == 0 or DENSE_FWD_NARROW)
                and (needs_grad or o % 256 == 0 or DENSE_FWD_NARROW or DENSE_MODE == 'force')
                and _hip.so3_dense_supported(p, na, ks, 16, o)):
            probe = (geometry[2], geometry[3])
            if (geometry[3] is not None and geometry[0] is geometry[1] and geometry[2] is geometry[3] and p == n):
                self.parts = _pose_parts(geometry[3])      # (one host read per pose tensor)
                if self.parts is not None:
                    probe = ()                             # the rotations are accounted for per part: no "exactly the identity" requirement
                    if self.parts.single:
                        # one rotation per cloud: every relative rotation R R^T is the identity -- the plain product -- PROVIDED the
                        # block is orthonormal (checked on the device with the other conditions)
                        probe = (('orthonormal', self.parts.reps[:, 0].contiguous()),)
                        self.parts = None
        # inverse neighbour lists (device only; the host-side numbers arrive asynchronously), started before the grouping so that
        # they run beside it; the entries too when the previous backward of this layer took the lists
        self.head = None
        if (lists_ok and needs_grad) or probe is not None:
            self.head = _ListHead(idx, n, args.nonident, args.gx, prefill=(not keep) and probe is None, dense_probe=probe,
                                  norm=norm if probe is not None else None)
        self.probed = probe is not None
        self.rp, self.forward = _dense_wanted(self.head, o, p, na, ks, nn, n) if self.probed else (0, False)

    def geo(self):
        """the product's DenseGeometry (_PartsDense when it runs per part), built by whoever needs it first: the forward if it runs the
        product, else the backward"""
        if self._geo is None:
            args, head = self.args, self.head
            head.wait()
            rest = (head.memb, head.rows, self.rp, args.rk, args.sigma, args.idx.shape[2], head.n_rows)
            if self.parts is None:
                self._geo = _hip.DenseGeometry(args.geometry[0], args.geometry[1], *rest)
            else:
                self._geo = _PartsDense(self.parts, args.geometry[1], *rest, args.mult, args.anchors)
        return self._geo


# ---- the forward regimes of _InterConv -----------------------------------------------------------------------------------------------

def _forward_dense(feats, W, plan, p, train_ep, folded):
    """The forward as the dense product: plain, with the training-mode norm in the node (train_ep), with a folded inference norm, or once per
    rigid part -> (y [b,o,p,a], bn): bn = what the node's BatchNorm backward needs, None unless train_ep joined the node."""
    geo, rows = plan.geo(), plan.head.rows
    if plan.parts is not None:
        return _dense_forward_parts(feats, W, rows, geo, p), None
    moments = affine = None
    partials = False
    if train_ep is not None:
        partials = train_ep.takes_partials(feats)
        ep, moments = train_ep, (train_ep.moments_from_partials if partials else train_ep.moments)
    elif folded is not None and folded.residual is None:
        # an inference-mode norm folded into one per-channel map: applied by the re-ordering pass too
        ep, affine = folded, (folded.scale, folded.shift, folded.slope)
    else:
        return _dense_forward(feats, W, rows, geo, p), None
    g, ldg, operand = _dense_operand(feats, W, rows, geo)
    y = _hip.so3_dense_fwd_bnact(g, geo, p, feats.shape[1], ldg, moments, operand=operand, o=W.shape[0], affine=affine, partials=partials)
    ep.applied = True
    return y, (None if train_ep is None else train_ep.saved + (float(train_ep.norm.negative_slope), bool(train_ep.norm.sync)))


# ---- group and contract: the textbook regimes -----------------------------------------------------------------------------------------
# Five regimes are a grouping into the intermediate X, the contraction Y = W X, and the textbook backward dW = sum_b dY_b X_b^T, dX = W^T dY
# through the grouping's transpose: the list kernels when the backward is 'textbook dX', the 'anchor map' and the 'residual map' (float32:
# X is scratch, X_CHUNK_CLOUDS clouds at a time, or kept whole for the backward's dW), the float64 inter and intra convs (slabs under
# F64_X_BYTES_MAX, X never kept).  A regime is its grouping pair; _group_contract and _backward_textbook are the skeleton around any pair.

class _Grouping:
    """A grouping and its transpose over the clouds [b0, b1) of a batch, the tensors that carry no gradient held as attributes:
        group(feats, b0, b1)             -> X [b1-b0, c, mid, p, a] (nominal shape: `layout` says what the memory behind it is)
        group_transposed(gx, n, b0, b1)  -> [b1-b0, c, n, a] from gx [b1-b0, c, mid, p, a] (reference layout)
    mid = kernel points or taps; layout = 0 / 1 / 2: reference / blocked / transposed (X_LAYOUT); log: the float64 node around the pair
    writes a FORWARD_LOG / BACKWARD_LOG entry; what: how a refusal names the conv and its middle axis."""
    layout, log, what = 0, False, ('so3conv', 'kernel points')

    def points(self, feats):
        """p of X for these features"""
        return self.idx.shape[1]


class _ListGrouping(_Grouping):
    """The list kernels (csrc/so3_inter.hip, csrc/so3_inter_lists2.hip) over an _InterConvArgs: the anchor axis unpermuted or permuted
    through the group's table `mult`.  store_order: the transposed X with its columns in the order the kernel's lanes hold them -- scratch
    for a contraction with W's columns permuted to match (_forward_lists), never what a backward regroups."""

    def __init__(self, a, layout=0):
        self.a, self.idx, self.mid, self.layout, self.store_order = a, a.idx, a.rk.shape[1], layout, False
        self.coset = _coset_tables(a.mult, a.ident) if (a.mult is not None and a.nonident is not None and layout == 2) else None

    def group(self, feats, b0, b1):
        a = self.a
        return _hip.so3_inter_group_fwd(feats[b0:b1], a.idx[b0:b1], a.gx[b0:b1], a.rk, a.mult, a.sigma,
                                        None if a.nonident is None else a.nonident[b0:b1], blocked=self.layout, coset=self.coset,
                                        store_order=self.store_order)

    def group_transposed(self, gx, n, b0, b1):
        a = self.a
        return _hip.so3_inter_group_bwd(gx, a.idx[b0:b1], a.gx[b0:b1], a.rk, a.mult, a.sigma, n, a.ident)


class _MapGrouping(_Grouping):
    """The per-entry maps of an _InterConvArgs, reference layout, the transpose accumulated without float atomics: `amap` uint8 [b,p,nn,na]
    of an anchor set that is not a group (_anchor_map; csrc/so3_inter_map.hip: many-to-one in the support row AND the anchor), or `shift`
    uint8 [b,p,nn], the residual index of the `use_2d` variant (_conv_2d; csrc/so3_inter_res.hip: feats [b,c,n,na*4], all four residual
    planes at once, many-to-one in the support row and, on ties, in the residual plane)."""

    def __init__(self, a):
        self.a, self.idx, self.mid = a, a.idx, a.rk.shape[1]
        if a.shift is None:
            self.regime, self.table, self.fwd, self.bwd = 'anchor map', a.amap, _hip.so3_inter_group_fwd_map, _hip.so3_inter_group_bwd_map
        else:
            self.regime, self.table, self.fwd, self.bwd = 'residual map', a.shift, _hip.so3_inter_group_fwd_res, _hip.so3_inter_group_bwd_res

    def group(self, feats, b0, b1):
        a = self.a
        return self.fwd(feats[b0:b1], a.idx[b0:b1], a.gx[b0:b1], a.rk, self.table[b0:b1], a.sigma)

    def group_transposed(self, gx, n, b0, b1):
        a = self.a
        return self.bwd(gx, a.idx[b0:b1], a.gx[b0:b1], a.rk, self.table[b0:b1], a.sigma, n)


def _inter_grouping(a, layout=0):
    """the float32 pair of an _InterConvArgs: through its per-entry map where it carries one, else the list kernels"""
    return _MapGrouping(a) if (a.amap is not None or a.shift is not None) else _ListGrouping(a, layout)


class _IntraGrouping(_Grouping):
    """The 12-tap gather of the intra convs, out[b,c,t,p,a] = feats[b,c,p,idx32[a,t]], and its transpose: kind 'f32' (csrc/so3_intra.hip),
    '2d' (the (na, 4) anchor axis, an anchor's residuals moved as one quad) or 'f64'."""
    what = ('intra_so3conv', 'taps')
    KERNELS = {'f32': ('so3_intra_group_fwd', 'so3_intra_group_bwd'), '2d': ('so3_intra_group2d_fwd', 'so3_intra_group2d_bwd'),
               'f64': ('so3_intra_group_fwd_f64', 'so3_intra_group_bwd_f64')}

    def __init__(self, intra_idx, kind):
        self.idx32, self.mid = intra_idx.to(torch.int32).contiguous(), intra_idx.shape[1]
        self.fwd, self.bwd = (getattr(_hip, name) for name in self.KERNELS[kind])

    def points(self, feats):
        return feats.shape[2]

    def group(self, feats, b0, b1):
        return self.fwd(feats[b0:b1], self.idx32)

    def group_transposed(self, gx, n, b0, b1):
        return self.bwd(gx, self.idx32)


def _slabs(b, step):
    """[(b0, b1), ...]: b clouds, `step` at a time"""
    return [(b0, min(b, b0 + step)) for b0 in range(0, b, step)]


def _f32_slabs(b, keep):
    """X_CHUNK_CLOUDS clouds at a time; a kept X is one slab of all clouds"""
    return _slabs(b, max(1, b if keep else X_CHUNK_CLOUDS))


def _empty_output(grouping, feats, W):
    """y [b,o,p,a] of the conv of feats [b,c,n,a] around `grouping`"""
    return torch.empty(feats.shape[0], W.shape[0], grouping.points(feats), feats.shape[3], dtype=feats.dtype, device=feats.device)


def _group_contract(grouping, feats, W, y, slabs, keep, contract):
    """The forward of every regime: per slab (b0, b1) the grouping into X, then contract(W, X, y[b0:b1] as [b1-b0, o, p*a], b0).
    -> X when `keep` (the backward's dW = dY X^T wants it; `slabs` is one slab of all clouds then), else None: X is scratch, one slab at a
    time."""
    x = None
    for b0, b1 in slabs:
        x = grouping.group(feats, b0, b1)
        contract(W, x, y[b0:b1].view(b1 - b0, y.shape[1], -1), b0)
        x = x if keep else None
    return x


def _backward_textbook(grouping, gy, W, feats, x, need_f, need_w, slabs):
    """The backward of every regime: per slab dW += dY X^T, then dX = W^T dY followed by the grouping's transpose -> (gF, gW).
    x = the forward's intermediate of the whole batch, or None (not kept): regrouped slab by slab, for dW only.
    float32: `slabs` is the whole batch -- the products reduce through a workspace, dX from W^T written out (a few MB: the product is then
    'nn' with a shared A operand, which the split-operand kernels take; with the transposition left to the GEMM it ran on the fp32 matrix
    pipe: 15.6 of the 61.6 ms step at 16 x 512 points).  float64: any slabs, dW accumulated in cloud order, dX from the view of W."""
    b, c, n, _ = feats.shape
    (o, ck), p, a = W.shape, gy.shape[2], gy.shape[3]
    pa, layout = p * a, grouping.layout
    gF = gW = None
    for b0, b1 in slabs:
        nb = b1 - b0
        gys = gy[b0:b1].view(nb, o, pa)
        if need_w:
            xs = x if x is not None else grouping.group(feats, b0, b1)      # wrong guess (or the first step): one more run of the grouping
            gW = torch.empty_like(W) if gW is None else gW
            # (measured and dropped: every cloud's dY_b X^T_b on the split-operand 'nn' kernel instead of the batch-reducing fp32 kernel --
            # 512 x 3072 outputs over K = 30720 are 48 workgroups without a split of K: 15.5 -> 48 ms at 16 x 512 points)
            if layout == 2:     # X^T [pa, ck]: dW = dY X^T is a plain row-major product
                _hip.matmul_reduce(gys, xs.view(nb, pa, ck), gW, accumulate=b0 > 0)
            elif layout == 1:   # blocked by 4: a storage without strides to read the numbers from -- the positional call
                _hip.gemm_reduce(0, 1, o, ck, pa, gys, pa, o * pa, xs, pa, ck * pa, gW, ck, nb, b_blocked=True)
            else:
                _hip.matmul_reduce(gys, xs.view(nb, ck, pa).transpose(1, 2), gW, accumulate=b0 > 0)
            xs = None                                                        # (released before W^T dY is allocated)
        if need_f:
            gx = torch.empty(nb, ck, pa, dtype=gy.dtype, device=gy.device)   # W^T gy
            _hip.matmul(W.t() if gy.dtype == torch.float64 else W.t().contiguous(), gys, gx)
            g = grouping.group_transposed(gx.view(nb, c, grouping.mid, p, a), n, b0, b1)
            del gx
            if nb == b:
                gF = g
            else:
                gF = torch.empty_like(feats) if gF is None else gF
                gF[b0:b1] = g
            del g                                                            # (not held beside the next slab's X)
    return gF, gW


def _forward_lists(feats, W, args, layout, keep, folded, head, fill):
    """The forward on the list kernels: grouping into the intermediate X (layout 0 / 1 / 2: reference / blocked / transposed, see X_LAYOUT),
    then the contraction -> (y [b,o,p,a], x): x = the intermediate when it is kept for a textbook backward (keep), else None -- X is then
    scratch, X_CHUNK_CLOUDS clouds at a time.  fill: the second half of head's lists is still to be made."""
    b, c, n, na = feats.shape
    ks, mult = args.rk.shape[1], args.mult
    if fill:
        head.fill(args.idx, args.gx, n)                # (the probe postponed it; a dense backward does not need the entries)
    grouping = _ListGrouping(args, layout)
    y = _empty_output(grouping, feats, W)
    x_bound = _grouped_bound(feats, args.idx) if layout == 2 else None          # [b, p] words
    # where X is scratch between the grouping and the contraction its columns may be in the order the grouping kernel's
    # lanes hold them (1 KB store runs, csrc/so3_inter_lists2.hip LAYOUT 4) with W's columns permuted to match
    tp = (not keep and STORE_ORDER_COLUMNS and layout == 2 and _hip.so3_group_fwd_tp_takes(c, na, ks)
          and (mult is None or (grouping.coset is not None and _hip.so3_group_perm_lists2_takes(c, na, ks, n))))
    grouping.store_order = tp
    Wc = W.index_select(1, _hip.so3_group_fwd_tp_columns(c, ks, W.device)) if tp else W

    def contract(Wc, x, ys, b0):
        _contract_into(Wc, x, ys, layout, folded, b0, x_bound=None if x_bound is None else (x_bound[b0:b0 + x.shape[0]], na, 1.0))
    return y, _group_contract(grouping, feats, Wc, y, _f32_slabs(b, keep), keep, contract)


# ---- regime 'narrow input': C*K <= 32 contraction indices, no input gradient, training-mode norm in the node (csrc/narrow_conv.hip) ----
# The conv output y = W X is a C*K-term dot product per element (24 at the first layer) and 2.7 x the size of X at O = 64: the node keeps
# X [b, C*K, P*A] (reference layout) and recomputes y in each of its four passes; neither y nor y' is saved, no lists are built, and the
# only host wait is the one the moments already have (SyncBatchNorm's exchange).

def _forward_narrow(feats, W, args, train_ep):
    """-> (y' [b,o,p,a], x [b, ck, p*a], bn): grouping as always (identity poses, one rotation per cloud, permuted poses: only the grouping
    sees them), moments of W X through TrainEpilogue.moments (running statistics, SyncBatchNorm), one pass that writes y'."""
    idx, rk = args.idx, args.rk
    b, c, _, na = feats.shape
    p, ks, o = idx.shape[1], rk.shape[1], W.shape[0]
    x = _hip.so3_inter_group_fwd(feats, idx, args.gx, rk, args.mult, args.sigma, args.nonident).view(b, c * ks, p * na)
    if train_ep.takes_partials(x):
        scale, shift, slope = train_ep.moments_from_partials(*_hip.narrow_conv_stats(W, x, partials=True), b * p * na)
    else:
        s1, s2, pivot = _hip.narrow_conv_stats(W, x)
        scale, shift, slope = train_ep.moments(s1, s2, pivot, b * p * na)
    y = _hip.narrow_conv_bnact_fwd(W, x, scale, shift, slope).view(b, o, p, na)
    train_ep.applied = True
    mean, invstd = train_ep.stats
    return y, x, (scale, shift, mean.float(), invstd.float(), train_ep.saved[3], slope, bool(train_ep.norm.sync))


def _native_norm_bwd(gy, count, sync):
    """the backward's per-channel sums and coefficients come from csrc/norm_fold.hip (see _hip.NATIVE_NORM_GLUE): not when the sums of several
    ranks are exchanged first (the element count is then a tensor too)"""
    return bool(_hip.NATIVE_NORM_GLUE and gy.is_cuda and isinstance(count, int) and not norm_fold._syncing(sync))


def _backward_narrow(gy, W, x, bn, need_w):
    """-> (gW, d gamma, d beta): one reduction pass over (dL/dy', X), then dW = sum gx X^T with the gradient behind the norm formed in
    registers (vgtk.so3conv.blocks._BNAct.backward's arithmetic)"""
    scale, shift, mean, invstd, count, slope, sync = bn
    b, o = gy.shape[0], gy.shape[1]
    gy = gy.view(b, o, -1)
    if _native_norm_bwd(gy, count, sync):
        # sums, d gamma, d beta, k2 and k3 in one launch (csrc/norm_fold.hip)
        g_bn_w, g_bn_b, k2, k3 = _hip.norm_fold_bwd(*_hip.narrow_conv_bwd_reduce(gy, x, W, scale, shift, mean, invstd, slope, partials=True), scale, count)
        return (_hip.narrow_conv_bwd_dw(gy, x, W, scale, shift, mean, invstd, k2, k3, slope) if need_w else None), g_bn_w, g_bn_b
    sg, sgx = _hip.narrow_conv_bwd_reduce(gy, x, W, scale, shift, mean, invstd, slope)
    gW = None
    if need_w:
        k2, k3 = norm_fold.backward_coefficients(scale, sg, sgx, count, True, sync)
        gW = _hip.narrow_conv_bwd_dw(gy, x, W, scale, shift, mean, invstd, k2, k3, slope)
    return gW, sgx.float(), sg.float()


# ---- the gradient tail: dF and dW from Z --------------------------------------------------------------------------------------------
# Z [b, o*ks, ldz] holds per row the (referenced row, anchor) pairs of a cloud: rp * na columns, (row, anchor) order from the list kernels,
# (anchor, row) order (`anchor_major`) from the dense product; ldz >= rp * na is the row pitch.  The two halves are launched in the order
# the regime wants (the per-part backward gathers the feature rows once, in front, and scatters the summed row gradient once, at the end).

def _weight_operand(W, c, ks, pad_c=None):
    """W [o, (c,k)] as the feature-gradient GEMM's shared operand W2 [c, (o,k)], zero-extended to pad_c rows"""
    o = W.shape[0]
    W2 = W.view(o, c, ks).permute(1, 0, 2).reshape(c, o * ks).contiguous()
    if pad_c is not None and pad_c != c:
        W2 = torch.cat([W2, torch.zeros(pad_c - c, o * ks, dtype=torch.float32, device=W.device)])
    return W2


def _rows_grad_from_z(z, W2, c, rp, na, ldz, anchor_major, z_bound=None, reorder=None):
    """dF over the referenced rows: W2 . Z -> [b,c,rp,na] (a view where the layout allows).  z_bound: a bound on Z's columns (see _hip.gemm
    b_bound); reorder: the anchor axis of Z is coset-major, `reorder` = the position of every anchor in it."""
    b, (pad_c, oks) = z.shape[0], W2.shape
    gFc = torch.empty(b, pad_c, ldz, dtype=torch.float32, device=z.device)
    _hip.matmul(W2, z.view(b, oks, ldz), gFc, b_bound=z_bound)
    if anchor_major:
        return gFc[:, :c, :rp * na].reshape(b, c, na, rp).transpose(2, 3)
    gFc = gFc.view(b, c, rp, na)
    return gFc if reorder is None else _hip.anchor_reorder(gFc, reorder)


def _weight_grad_rows(z, fc4, o, ks, ldz, anchor_major, reorder=None):
    """dW from Z and the referenced feature rows fc4 [b,c,rp,na] (reorder: Z's coset-major anchor order, see _coset_tables)"""
    b, c, rp, na = fc4.shape
    if reorder is not None:
        fc4 = _hip.anchor_reorder(fc4, reorder)
    fc = fc4.transpose(2, 3).contiguous() if anchor_major else fc4
    return _weight_grad_from_z(z, fc.view(b, c, rp * na), b, c, o, ks, rp * na, ldz)


# ---- the backward regimes of _InterConv ----------------------------------------------------------------------------------------------
# Strategy: when few support rows are referenced (the reference's first-nsample-in-index-
# order ball query with large radii), BOTH gradients follow from
#     Z[o,k,q,a'] = sum_{(p,n)->q} dY[o,p,a] w(p,a,k,n)          (csrc/so3_inter_inv.hip; csrc/so3_dense.hip as a dense product)
#     dF[c,q,a'] = sum_{o,k} W[o,(c,k)] Z[o,k,q,a']       dW[o,(c,k)] = sum_{q,a'} Z[o,k,q,a'] F[c,q,a']
# two small GEMMs over the referenced rows only -- no dX = W^T dY, no scatter, and the
# [O x P*A] x [P*A x C*K] weight-gradient GEMM shrinks by P / (referenced rows).

# The tail on PACKED Z (vgtk/_hip.py "the gradient tail on PACKED Z"): the product writes cloud i's column (a, r) at a * live16[i] + r, so the
# live columns are one prefix of the row; dF, dW, the bound words, the gathered feature rows and the row scatter all end at that prefix.  No
# zero fill of the dead slots, no product over them, no transposed copy of the gathered rows.  Taken by the identity-pose node with its norm
# inside, where both GEMMs are on the split kernels (128-channel inputs: the 64-channel layer's dW runs on the fp32 pipe, which has no
# per-cloud end of the contraction -- it keeps the zero-filled layout).  False: the zero-filled layout everywhere.
DENSE_TAIL_PACKED = True


def _dense_tail_packed_takes(W, feats, head, geo, c, pad_c, ldz, need_f, need_w):
    na, o, ks, rp = feats.shape[3], W.shape[0], geo.ks, geo.rp
    if not (need_f and need_w and pad_c == c and c % 128 == 0 and rp % 16 == 0 and ldz == _hip.dense_pitch(na * rp) and geo.n_rows is not None
            and head.n_rows is geo.n_rows and feats.is_cuda):
        return False
    return _hip.dense_tail_packed_takes(c, o * ks, na * rp, ldz)


def _dense_tail_packed(z, W, feats, head, geo, colmax, p, ldz, need_f, need_w):
    """dF and dW from packed Z [b,o,ks,ldz] -> (gF, gW)"""
    b, c, n, na = feats.shape
    o, ks, rp = W.shape[0], geo.ks, geo.rp
    ra = na * rp
    words, ncols = _hip.so3_dense_zbound_packed(colmax, head.cnt, head.n_rows, rp, p, ldz)
    zm = z.view(b, o * ks, ldz)
    gFc = torch.empty(b, c, ldz, dtype=torch.float32, device=z.device)
    _hip.matmul_tail(_weight_operand(W, c, ks), zm, gFc, ncols, (words.view(torch.int32), 4, 1.0))
    gF = _hip.rows_scatter_packed(gFc, c, head.rows, head.n_rows, rp, n, na)
    fc = _hip.rows_gather_packed(feats, head.rows, head.n_rows, rp, ldz)             # [b,c,ldz]
    dt = torch.empty(c, o * ks, dtype=torch.float32, device=z.device)
    _hip.matmul_reduce_tail(fc[..., :ra], zm[..., :ra].transpose(1, 2), dt, ncols)
    return gF, dt.view(c, o, ks).permute(1, 0, 2).reshape(o, c * ks).contiguous()


def _backward_dense(gy, W, feats, head, geo, bn, yact, need_f, need_w):
    """Z by the dense product (bn: through the node's BatchNorm + leaky_relu first, yact = the node's output) -> (gF, gW, g_bn_w, g_bn_b)"""
    b, c, n, na = feats.shape
    o, ks, p, rp = W.shape[0], geo.ks, gy.shape[2], geo.rp
    if BACKWARD_LOG is not None:
        BACKWARD_LOG.append({'channels': (c, o), 'support_rows': n, 'referenced_rows_max': int(rp), 'regime': 'dense rows',
                             **({'norm': 'in the node'} if bn is not None else {})})
    ra = na * rp
    # Z's rows padded to whole 128-column tiles where that puts the feature-gradient GEMM on the split-operand kernels
    # (the padding is never written: garbage columns of gFc nobody reads; the weight gradient contracts over ra columns)
    # (c = 64: W2 padded to 128 zero-extended rows for the same reason -- the 64-row product ran on the fp32 pipe: 0.92 ms)
    pad_c = 128 if (c == 64 and bn is not None) else c
    ldz = _hip.dense_pitch(ra) if (pad_c % 128 == 0 and (o * ks) % 16 == 0 and need_f) else ra
    gF = gW = g_bn_w = g_bn_b = z_bound = None
    if bn is not None:
        # the BatchNorm + leaky_relu backward of the node (csrc/bn_act.hip header): one reduction pass over (dL/dy', y'), then gx is
        # formed inside the split of the product's stored operand
        k1, beta, inv_gamma, count, slope, sync = bn
        native = _native_norm_bwd(gy, count, sync)
        if native:
            # the sums, the coefficients and the bounds in one entry (csrc/norm_fold.hip); colmax [b,na] = bound.amax(1)
            pg, pgx, gmax, xmax = _hip.bn_act_bwd_reduce_fromy(gy, yact, beta, inv_gamma, slope, partials=True)
            g_bn_w, g_bn_b, _, _, coef, bound, colmax = _hip.norm_fold_bwd(pg, pgx, k1, count, beta, inv_gamma, gmax, xmax)
        else:
            sg, sgx, gmax, xmax = _hip.bn_act_bwd_reduce_fromy(gy, yact, beta, inv_gamma, slope)
            g_bn_w, g_bn_b = sgx.float(), sg.float()
            k2, k3 = norm_fold.backward_coefficients(k1, sg, sgx, count, True, sync)
            coef = torch.stack([k1, k2, k3, beta, inv_gamma]).contiguous()      # [5, o]
            bound = (k1.abs()[None, :, None] * gmax + k2.abs()[None, :, None] + k3.abs()[None, :, None] * xmax).contiguous()
        if DENSE_TAIL_PACKED and native and _dense_tail_packed_takes(W, feats, head, geo, c, pad_c, ldz, need_f, need_w):
            z = _hip.so3_dense_bwd_bn(gy, yact, geo, ldz, coef, bound, slope, packed=True)
            return (*_dense_tail_packed(z, W, feats, head, geo, colmax, p, ldz, need_f, need_w), g_bn_w, g_bn_b)
        z = _hip.so3_dense_bwd_bn(gy, yact, geo, ldz, coef, bound, slope)
        if ldz % 4 == 0 and rp % 4 == 0 and native:
            # (the same bound as below in one launch: eap_so3_dense_zbound_f32)
            z_bound = (_hip.so3_dense_zbound(colmax, head.cnt, head.n_rows, rp, p, ldz).view(torch.int32), 4, 1.0)
        elif ldz % 4 == 0 and rp % 4 == 0:
            # a bound on Z's columns for the feature-gradient GEMM below (it then runs with two fp16 planes per operand instead of
            # three bf16 planes, without a pass over Z): |Z[o,k,(a,r)]| = |sum_p gx[o,p,a] w| <= max_o bound[o,a] x (points listing row r)
            live = torch.arange(rp, device=gy.device)[None, :] < head.n_rows[:, None]                      # (slots past a cloud's rows: zero columns)
            cntf = torch.where(live, head.cnt[:, :rp], torch.zeros_like(head.cnt[:, :rp])).clamp(min=0, max=p).to(torch.float32)
            cols = bound.amax(1)[:, :, None] * cntf[:, None, :]                                           # [b,na,rp]
            words = torch.zeros(b, ldz // 4, dtype=torch.float32, device=gy.device)
            words[:, :ra // 4] = cols.view(b, na, rp // 4, 4).amax(3).view(b, ra // 4)
            z_bound = (words.view(torch.int32), 4, 1.0)
    else:
        z = _hip.so3_dense_bwd(gy, geo, ldz)                                 # [b,o,ks,ldz] rows = [na,rp]: the lists' Z, anchor axis in front
    if need_f:
        gFr = _rows_grad_from_z(z, _weight_operand(W, c, ks, pad_c), c, rp, na, ldz, True, z_bound)
        gF = _hip.rows_scatter(gFr.contiguous(), head.rows, n)
    if need_w:
        gW = _weight_grad_rows(z, _hip.rows_gather(feats, head.rows, rp), o, ks, ldz, True)
    return gF, gW, g_bn_w, g_bn_b


def _backward_dense_parts(gy, W, feats, head, pd, need_f, need_w):
    """the dense backward of posed clouds, one product per part slot (_PartsDense): Z_i over the part's query points, the two small
    GEMMs per part, the rows' anchor axis permuted back before the sum over the parts -> (gF, gW)"""
    b, c, n, na = feats.shape
    o, ks, rp = W.shape[0], pd.ks, pd.rp
    ra = na * rp
    if BACKWARD_LOG is not None:
        BACKWARD_LOG.append({'channels': (c, o), 'support_rows': n, 'referenced_rows_max': int(rp), 'regime': 'dense rows', 'parts': pd.parts.n})
    ldz = _hip.dense_pitch(ra) if (c % 128 == 0 and (o * ks) % 16 == 0 and need_f) else ra
    W2 = _weight_operand(W, c, ks) if need_f else None
    fc0 = _hip.rows_gather(feats, head.rows, rp) if need_w else None                        # [b,c,rp,na]
    gFr = gW = None
    # (the row maxima the BatchNorm backward left are those of ALL points: an upper bound for every part's columns)
    rowmax = _hip.take_rowmax_hint(gy)
    for i, geo in enumerate(pd.geo):
        perm = pd.perm[i]
        z = _hip.so3_dense_bwd(gy, geo, ldz, colmap=pd.parts.col_map[i], rowmax=rowmax)      # [b,o,ks,ldz] rows = [na,rp]
        pe = None if perm is None else perm[:, None].expand(b, c, rp, na)
        if need_f:
            t = _rows_grad_from_z(z, W2, c, rp, na, ldz, True)                                # gradient of F_i[.., r, a] = F[.., r, perm[r, a]]
            if gFr is None:
                gFr = torch.zeros(b, c, rp, na, dtype=torch.float32, device=gy.device)
            if pe is None:
                gFr += t
            else:
                gFr.scatter_add_(3, pe, t.contiguous())
        if need_w:
            gw = _weight_grad_rows(z, fc0 if pe is None else fc0.gather(3, pe), o, ks, ldz, True)
            gW = gw if gW is None else gW + gw
        del z
    gF = _hip.rows_scatter(gFr, head.rows, n) if need_f else None
    return gF, gW


def _backward_lists(gy, W, feats, idx, gx, rk, mult, args, head, rcap, any_nonident, need_f, need_w):
    """Z by the inverse-list kernels (csrc/so3_inter_inv.hip, csrc/so3_inter_lists2.hip) over the first rcap referenced rows -> (gF, gW)"""
    b, c, n, na = feats.shape
    p, ks, o = idx.shape[1], rk.shape[1], W.shape[0]
    gF = gW = None
    # slots past a cloud's last referenced row are empty (rows = -1): a multiple of 4 rows makes K = rcap * na of the
    # gradient GEMMs a multiple of 16.  (A multiple of 32 would put the dF GEMM on the split kernel -- measured: the 18 %
    # more rows at 136 referenced rows cost what the faster kernel gains.)
    rcap = min((rcap + 3) & ~3, n)
    head.wait()
    rows = head.rows[:, :rcap].contiguous()
    off, cnt = head.off[:, :rcap].contiguous(), head.cnt[:, :rcap].contiguous()
    ent_p, ent_gx = head.entries if head.entries is not None else _hip.inv_lists_fill(idx, gx, head.rows, head.off, rcap)
    multinv = _group_tables_inverse(mult) if (mult is not None and any_nonident) else None
    coset = _coset_tables(multinv, args.ident) if multinv is not None else None
    z_order = z_pos = None
    if coset is not None and _hip.so3_group_perm_lists2_takes(o, na, ks, p):
        # permuted clouds on the two-tile kernel (csrc/so3_inter_lists2.hip, PERM): gy and Z with a coset-major anchor
        # axis, the per-entry words prepared once; the small tensors around the two GEMMs change their anchor order
        z_order, z_pos = coset[0], coset[2]
        ent_pc, ent_gx2 = _hip.so3_perm_entries(ent_p, ent_gx, coset[1], args.anchors, args.ident, na, p)
        z = _hip.so3_inter_group_inv_perm2(_hip.anchor_reorder(gy, z_order), rows, off, cnt, ent_pc, ent_gx2, rk, z_order,
                                           args.sigma, idx.shape[2])
    else:
        z = _hip.so3_inter_group_inv(gy, rows, off, cnt, ent_p, ent_gx, rk, multinv, args.sigma, idx.shape[2],
                                     args.ident, args.anchors, coset)              # [b,o,ks,rcap,na]
    if need_f:
        gFr = _rows_grad_from_z(z, _weight_operand(W, c, ks), c, rcap, na, rcap * na, False, reorder=z_pos)
        gF = _hip.rows_scatter(gFr, rows, n)                                    # unreferenced rows: zero gradient
    if need_w:
        # (rows_gather: [b,c,rcap,na]; unused slots: zeros)
        gW = _weight_grad_rows(z, _hip.rows_gather(feats, rows, rcap), o, ks, rcap * na, False, reorder=z_order)
    return gF, gW


class _InterConv(torch.autograd.Function):
    """Fused inter conv  y = W . group(feats)  (functional.py:L1221-1261 + modules.py:L48-55)
    with the re-associated feature gradient (csrc/so3_inter_inv.hip).  forward and backward decide the regime and dispatch to the
    _forward_* / _backward_* functions above; the regimes that group and contract hand their pair to _group_contract / _backward_textbook."""

    DIFFERENTIABLE = 4      # feats, W, bn_weight, bn_bias come first: needs_input_grad is indexed by these positions only

    @staticmethod
    def forward(ctx, feats, W_param, bn_weight, bn_bias, args):
        # (bn_weight, bn_bias: the parameters of a TrainEpilogue's norm -- inputs of the node so that it can hand back their gradients;
        # args: an _InterConvArgs)
        feats = feats.contiguous()
        W = W_param.contiguous()
        idx, rk, mult, nonident = args.idx, args.rk, args.mult, args.nonident
        # X is internal to this Function: where the kernels allow it, it is kept blocked by anchor
        # quads ([b,p,a/4,c,k,4]) -- coalesced row-end stores in the grouping kernel -- and the GEMMs
        # read it as a blocked B operand (include/eap_hip.h, "blocked intermediate")
        can = X_LAYOUT != 'reference' and _hip.so3_inter_group_fwd_can_block(
            feats.shape[1], feats.shape[2], feats.shape[3], rk.shape[1], mult is not None, nonident is not None)
        layout = 0 if not can else (2 if X_LAYOUT == 'transposed' else 1)
        _, c, n, na = feats.shape
        p, ks, o = idx.shape[1], rk.shape[1], W.shape[0]
        needs_grad = (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) and args.grad_mode
        train_ep = args.epilogue if isinstance(args.epilogue, TrainEpilogue) else None
        folded = None if train_ep is not None else args.epilogue      # (the list kernels know nothing of a TrainEpilogue: `applied` stays False there)
        if folded is not None and (needs_grad or not folded.inference):
            raise RuntimeError('a folded epilogue is an inference-time fusion: build and use it under torch.no_grad()')
        if args.amap is not None or args.shift is not None:
            # an anchor set that is not a group, really permuted ('anchor map'), or the 60 x 4 anchor axis of the `use_2d` variant with really
            # permuted residual indices ('residual map', feats [b,c,n,na*4]): a per-entry map has no inverse-list or dense form
            # (X in the reference layout, kept only for the backward's dW = dY X^T)
            grouping, keep = _MapGrouping(args), bool(needs_grad and ctx.needs_input_grad[1])
            if FORWARD_LOG is not None:
                FORWARD_LOG.append({'channels': (c, o), 'dense': False, 'parts': None, 'regime': grouping.regime})
            y = _empty_output(grouping, feats, W)
            x = _group_contract(grouping, feats, W, y, _f32_slabs(feats.shape[0], keep), keep,
                                lambda W, x, ys, b0: _contract_into(W, x, ys, 0, folded, b0))
            ctx.bn, ctx.conv_args, ctx.head, ctx.layout, ctx.plan = None, args, None, 0, None
            ctx.W_param = weakref.ref(W_param)
            ctx.save_for_backward(W, x, idx, args.gx, rk, None, nonident, feats, None)
            return y
        # at most 32 contraction indices and no gradient into the input (the first layer): nothing the inverse lists could serve -- the
        # backward is dW alone, straight from the kept X
        narrow = c * ks <= _hip.NARROW_CONV_MAX_CK and not ctx.needs_input_grad[0]
        if narrow and train_ep is not None and FUSE_CONV_NORM and _hip.narrow_conv_takes(o, c * ks, p * na):
            if FORWARD_LOG is not None:
                FORWARD_LOG.append({'channels': (c, o), 'dense': False, 'parts': None, 'regime': 'narrow input'})
            y, x, bn = _forward_narrow(feats, W, args, train_ep)
            wanted = args.grad_mode and any(ctx.needs_input_grad[1:_InterConv.DIFFERENTIABLE])
            ctx.bn, ctx.conv_args, ctx.head, ctx.layout, ctx.plan = (bn if wanted else None), args, None, 0, None
            ctx.narrow = True
            ctx.W_param = weakref.ref(W_param)
            ctx.save_for_backward(W, x if wanted else None, idx, None, rk, None, None, feats, None)
            return y
        lists_ok = BACKWARD_MODE != 'dx' and _inv_lists_supported(idx, n, na, ks) and not narrow
        keep = needs_grad and (not lists_ok or _keep_x_hint(W_param))
        plan = _DensePlan(args, n, o, lists_ok, needs_grad, keep, folded, train_ep.norm if (train_ep is not None and FUSE_CONV_NORM) else None)
        head = plan.head if needs_grad else None
        if FORWARD_LOG is not None:
            FORWARD_LOG.append({'channels': (c, o), 'dense': bool(plan.forward), 'parts': None if plan.parts is None else plan.parts.n})
        if plan.forward:
            # (a frozen conv under a trainable norm -- gradients wanted for the norm's parameters only -- keeps the separate module:
            # the node's backward is the conv's dense backward)
            bn_only = args.grad_mode and not needs_grad and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
            # (a norm with a channel past NORM_IN_NODE_MAX_RATIO keeps the separate module too: its backward has the stored input)
            join = FUSE_CONV_NORM and not bn_only and train_ep is not None and not plan.head.norm_ill()
            y, ctx.bn = _forward_dense(feats, W, plan, p, train_ep if join else None, folded)
            x, layout = None, 0
        else:
            fill = head is not None and plan.probed and not keep and plan.rp == 0
            y, x = _forward_lists(feats, W, args, layout, keep, folded, head, fill)
            ctx.bn = None
        ctx.conv_args, ctx.head, ctx.layout = args, head, layout
        ctx.plan = plan if (plan.rp > 0 and needs_grad) else None
        ctx.W_param = weakref.ref(W_param)
        # feats: needed by the re-associated weight gradient (saved, not copied: autograd's version check
        # then catches an in-place update of the previous block's output); y: the node's output when it holds the norm (TrainEpilogue)
        ctx.save_for_backward(W, x, idx, args.gx, rk, mult, nonident, feats, y if (ctx.bn is not None and needs_grad) else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        W, x, idx, gx, rk, mult, nonident, feats, yact = ctx.saved_tensors       # (x, mult, nonident, yact: None where the forward had none)
        args, head, plan = ctx.conv_args, ctx.head, ctx.plan
        gy = gy.contiguous()
        n = feats.shape[2]
        need_f, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_bn_w = g_bn_b = None
        if getattr(ctx, 'narrow', False):
            if BACKWARD_LOG is not None:
                BACKWARD_LOG.append({'channels': (feats.shape[1], W.shape[0]), 'support_rows': n, 'referenced_rows_max': 0,
                                     'regime': 'narrow input', 'norm': 'in the node'})
            gF = None
            gW, g_bn_w, g_bn_b = _backward_narrow(gy, W, x, ctx.bn, need_w)
        elif args.amap is not None or args.shift is not None:
            grouping = _MapGrouping(args)
            if BACKWARD_LOG is not None:
                BACKWARD_LOG.append({'channels': (feats.shape[1], W.shape[0]), 'support_rows': n, 'referenced_rows_max': 0,
                                     'regime': grouping.regime})
            gF, gW = _backward_textbook(grouping, gy, W, feats, x, need_f, need_w, [(0, feats.shape[0])])
        elif plan is not None and plan.parts is not None:
            gF, gW = _backward_dense_parts(gy, W, feats, head, plan.geo(), need_f, need_w)
        elif plan is not None:
            gF, gW, g_bn_w, g_bn_b = _backward_dense(gy, W, feats, head, plan.geo(), ctx.bn, yact, need_f, need_w)
        else:
            rcap, any_nonident = 0, True
            if head is not None:
                rcap, any_nonident = head.decide()
                if BACKWARD_MODE == 'auto' and rcap * INV_ROW_FRACTION > n:
                    head.entries = None                        # (prefilled on last step's hint, not needed after all: 20 bytes per entry)
                    head = None
            if BACKWARD_LOG is not None:      # diagnostics for bench.py / tests: which regime each layer's backward took
                BACKWARD_LOG.append({'channels': (feats.shape[1], W.shape[0]), 'support_rows': n, 'referenced_rows_max': int(rcap),
                                     'regime': 'inverse lists' if head is not None else 'textbook dX'})
            Wp = ctx.W_param()
            if Wp is not None:
                _set_keep_x_hint(Wp, head is None)            # the next forward of this layer keeps X iff this backward needed it
            if head is not None:
                gF, gW = _backward_lists(gy, W, feats, idx, gx, rk, mult, args, head, rcap, any_nonident, need_f, need_w)
            else:
                gF, gW = _backward_textbook(_ListGrouping(args, ctx.layout), gy, W, feats, x, need_f, need_w, [(0, feats.shape[0])])
        return (gF, gW, g_bn_w, g_bn_b) + (None,) * (len(ctx.needs_input_grad) - _InterConv.DIFFERENTIABLE)


INTRA_DW_SLICE = 64      # channels whose 12-tap gather is materialised at a time for the intra weight gradient


def _intra_inverse_table(idx32):
    """inv[idx[a,t], t] = a: every column idx[:, t] is a permutation of the anchors"""
    na, nt = idx32.shape
    inv = torch.empty_like(idx32)
    inv.scatter_(0, idx32.long(), torch.arange(na, device=idx32.device, dtype=torch.int32)[:, None].expand(na, nt).contiguous())
    return inv.contiguous()


def _intra_kernels(feats, idx32):
    """(implicit conv, grouping) launchers for the features' anchor axis: the table's rows, or rows x residuals with the residual
    innermost (IntraSO3Conv2D, functional.py:L2606-2627), where the kernels move an anchor's residuals as one 16-byte quad"""
    if feats.shape[3] == idx32.shape[0]:
        return _hip.so3_intra_conv, _hip.so3_intra_group_fwd
    return _hip.so3_intra_conv2d, _hip.so3_intra_group2d_fwd


class _IntraConv(torch.autograd.Function):
    """Intra SO(3) conv  y[b,o,p,a] = sum_{c,t} W[o, c*T + t] F[b,c,p,idx[a,t]]  (functional.py:L2553-2602 +
    modules.py:L48-55) WITHOUT the [B,C,T,P,A] gathered tensor (48 GB at C = 512, B = 8) in either direction:
      forward   implicit GEMM, the gather folded into the operand load (eap_so3_intra_conv_f32);
      dF        the same kernel: every column idx[:,t] is a permutation of the anchors, so
                dF[b,c,p,a'] = sum_{o,t} W[o, c*T + t] dY[b,o,p, inv_t(a')] -- weights regrouped to [C, O*T], gather
                table inv[a', t];
      dW        sum_{b,p,a} dY[b,o,p,a] F[b,c,p,idx[a,t]]: the gather is materialised for INTRA_DW_SLICE channels at
                a time (eap_so3_intra_group_fwd) and contracted by the k-split reduce GEMM (3 GB of scratch instead
                of 48).
    The (60, 4) anchor axis of IntraSO3Conv2D, y[b,o,p,a,r] = sum_{c,t} W[o, c*T + t] F[b,c,p,idx[a,t],r] (functional.py:L2606-2627; the
    gathered tensor would be 193 GB), takes the same three steps on the quad kernels (_intra_kernels), with as many channels per dW slice
    as keep its bytes: 16 of 240 entries for 64 of 60."""

    @staticmethod
    def forward(ctx, feats, W, idx32):
        feats, W = feats.contiguous(), W.contiguous()
        ctx.save_for_backward(feats, W, idx32)
        return _intra_kernels(feats, idx32)[0](feats, W, idx32)

    @staticmethod
    def backward(ctx, gy):
        feats, W, idx32 = ctx.saved_tensors
        gy = gy.contiguous()
        b, c, p, tot = feats.shape
        o, (na, nt) = W.shape[0], idx32.shape
        conv, group = _intra_kernels(feats, idx32)
        gF = gW = None
        if ctx.needs_input_grad[0]:
            W2 = W.view(o, c, nt).permute(1, 0, 2).reshape(c, o * nt).contiguous()
            gF = conv(gy, W2, _intra_inverse_table(idx32))
        if ctx.needs_input_grad[1]:
            gW = torch.empty(o, c, nt, dtype=torch.float32, device=gy.device)
            pa = p * tot
            step = max(1, INTRA_DW_SLICE * na // tot)
            for c0 in range(0, c, step):
                c1 = min(c, c0 + step)
                g = group(feats[:, c0:c1].contiguous(), idx32)                          # [b, cs, nt, p, tot]
                d = torch.empty(o, (c1 - c0) * nt, dtype=torch.float32, device=gy.device)
                _hip.matmul_reduce(gy.view(b, o, pa), g.view(b, (c1 - c0) * nt, pa).transpose(1, 2), d)
                gW[:, c0:c1] = d.view(o, c1 - c0, nt)
                del g, d                                                                # one slice of scratch at a time, not two
            gW = gW.view(o, c * nt)
        return gF, gW, None


def intra_so3conv(feats, W, intra_idx):
    """feats [b,c,p,na], W [o, c*T], intra_idx [na,T] -> [b,o,p,na]; what IntraSO3Conv.forward runs."""
    dtype = _call_dtype('intra_so3conv', feats=feats, W=W)
    if not feats.is_cuda:
        raise RuntimeError('intra_so3conv: device tensors only')
    if dtype == torch.float64:
        return _GroupContractF64.apply(feats, W, _IntraGrouping(intra_idx, 'f64'))
    return _IntraConv.apply(feats, W, intra_idx.to(torch.int32).contiguous())


def intra_so3conv2d(feats, W, intra_idx):
    """feats [b,c,p,na*4], W [o, c*T], intra_idx [na,T] -> [b,o,p,na*4], the residual innermost; what IntraSO3Conv2D.forward runs."""
    if feats.dtype != torch.float32 or not feats.is_cuda:
        raise RuntimeError('intra_so3conv2d: float32 device tensors only (the float64 regime does not cover the 2-D variant)')
    if feats.shape[3] != 4 * intra_idx.shape[0]:
        raise RuntimeError(f'intra_so3conv2d: an anchor axis of {feats.shape[3]} entries is not {intra_idx.shape[0]} anchors x 4 residuals')
    return _IntraConv.apply(feats, W, intra_idx.to(torch.int32).contiguous())


def _aligned16(t):
    """A contiguous tensor whose first element sits on a 16-byte boundary: `t` itself when it already does, else a copy (a
    contiguous VIEW into a larger storage -- a slice of autograd's gradient buffer, say -- can start at any 4-byte offset,
    and the streaming kernels move 16-byte words)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _NarrowContract(torch.autograd.Function):
    """_Contract for at most four output channels (the pose head's translation components, the attention logit): no matrix
    core has work for 1-4 rows, the op is a streaming pass over x in each direction (csrc/narrow_contract.hip)."""

    @staticmethod
    def forward(ctx, W, x):
        W, x = W.contiguous(), _aligned16(x)
        b, c, n = x.shape
        o = W.shape[0]
        y = torch.empty(b, o, n, dtype=torch.float32, device=x.device)
        _hip.call('eap_narrow_contract_fwd_f32', x, b, o, c, n, W, x, y)
        ctx.save_for_backward(W, x)
        return y

    @staticmethod
    def backward(ctx, gy):
        W, x = ctx.saved_tensors
        gy = _aligned16(gy)
        b, c, n = x.shape
        o = W.shape[0]
        gW = gx = None
        if ctx.needs_input_grad[1]:
            gx = torch.empty_like(x)
            _hip.call('eap_narrow_contract_dx_f32', x, b, o, c, n, W, gy, gx)
        if ctx.needs_input_grad[0]:
            slabs = int(_hip.abi.eap_narrow_contract_dw_slabs(n))
            part = torch.empty(slabs * b, o, c, dtype=torch.float32, device=x.device)
            _hip.call('eap_narrow_contract_dw_f32', x, b, o, c, n, gy, x, part)
            gW = part.sum(0, dtype=torch.float64).float()
        return gW, gx


def so3_contract(W, x, epilogue=None):
    """W [O, C*K], x [b, C*K, P*A] -> [b, O, P*A] (epilogue: a FoldedEpilogue the product may apply, inference only)."""
    dtype = _call_dtype('so3_contract', x=x, W=W)
    if dtype == torch.float64 and epilogue is not None:
        raise RuntimeError('so3_contract: a folded epilogue is float32 only, a float64 contraction takes none')
    _hip.check_input(x)
    if not W.is_cuda:
        raise RuntimeError('so3_contract: W must be a device tensor')
    if dtype == torch.float64:
        return _ContractF64.apply(W, x)
    if epilogue is None and W.shape[0] <= 4 and _hip.abi.eap_narrow_contract_supported(x.shape[0], W.shape[0], x.shape[1], x.shape[2]):
        return _NarrowContract.apply(W, x)
    return _Contract.apply(W, x, epilogue)


# ------------------------------------------------------------------------------------------------
# the float64 regime (csrc/so3_f64.hip): chosen by the dtype of the tensors, one plain kernel per step
# ------------------------------------------------------------------------------------------------
# The reference's Python path is dtype-generic; a model after .double() runs L1025-1261 in float64 with ONE quirk this regime keeps: the
# neighbour coordinates pass through float32 (group_nd -> gather_points_forward returns float32 for any input, gathering_cuda.cpp:L38-39),
# so g = R_rel (float(x_n) - x_p), the subtraction and everything after it in float64.  For inputs that are float32 numbers widened (a
# float64 run as the checker of a float32 one) that is a no-op.
# The grouped intermediate X [b,c,ks,p,na] is 8 b c ks p na bytes (6 GB per cloud at c = 128, p = 4096): clouds are processed in slabs
# that keep it under F64_X_BYTES_MAX (at least one cloud), X is recomputed in the backward, never saved.  Every cloud's output and feature
# gradient depend on that cloud alone, and dW adds every cloud's product in index order (eap_gemm_f64_reduce): the results do not
# depend on the slab size, bit for bit.
F64_X_BYTES_MAX = 4 << 30


def _f64_slabs(b, bytes_per_cloud):
    """[(b0, b1), ...]: the clouds in slabs whose intermediate stays under F64_X_BYTES_MAX (one cloud where a single one exceeds it)"""
    return _slabs(b, max(1, int(F64_X_BYTES_MAX // max(int(bytes_per_cloud), 1))))


class _F64Args(_Grouping):
    """The grouping pair of the float64 inter conv (csrc/so3_f64.hip; the transpose over inverse neighbour lists, no atomics), made of the
    inputs that carry no gradient: idx int32 [b,p,nn], g float64 [b,p,nn,3], r int32 [b,p,nn], rk
    float64 [na,ks,3], mult uint8 [na,na] and its row-wise inverse (None: no anchor permutation), sigma."""

    def __init__(self, idx, g, r, rk, mult, multinv, sigma):
        self.idx, self.g, self.r, self.rk, self.mult, self.multinv, self.sigma = idx, g, r, rk, mult, multinv, float(sigma)
        self.lists, self.mid, self.log = None, rk.shape[1], True

    def inverse_lists(self, n):
        """(rows, off, cnt, ent) of the whole batch (csrc/inv_lists.hip, index only; csrc/so3_f64.hip the entries), built once"""
        if self.lists is None:
            if n > INV_LISTS_MAX_ROWS:
                raise NotImplementedError(f'float64 backward of the inter conv: at most {INV_LISTS_MAX_ROWS} support points per cloud '
                                          f'(the inverse neighbour lists are sorted in LDS), got {n}')
            rows, off, cnt, _ = _hip.inv_lists_rows(self.idx, n)
            self.lists = (rows, off, cnt, _hip.inv_lists_entries(self.idx, rows, off))
        return self.lists

    def group(self, feats, b0, b1):
        return _hip.so3_inter_group_fwd_f64(feats[b0:b1], self.idx[b0:b1], self.g[b0:b1], self.r[b0:b1], self.rk, self.mult, self.sigma)

    def group_transposed(self, gx, n, b0, b1):
        lists = tuple(t[b0:b1] for t in self.inverse_lists(n))
        return _hip.so3_inter_group_bwd_f64(gx, lists, self.g[b0:b1], self.r[b0:b1], self.rk, self.multinv, self.sigma, n, self.idx.shape[2])


def _neighbourhood_f64(xyz, pose, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz, q_pose):
    """_neighbourhood in float64: the existing float64 ball query (float radius, as the reference's signature), the tables in the module's
    dtype, eap_so3_prep_f64 -> _F64Args.  An anchor set that is not a group (kanchor 20 / 40) is taken where the float32 path continues
    without permutation (no pose, identity poses, one rotation per cloud); really permuted it has no float64 kernel."""
    q_xyz = xyz if q_xyz is None else q_xyz
    _call_dtype('so3conv', xyz=xyz, q_xyz=q_xyz, anchors=anchors, kernels=kernels, pose=pose, q_pose=q_pose)
    if not (anchors.is_cuda and kernels.is_cuda):
        raise RuntimeError('so3conv: anchors and kernels must be device tensors')
    ball_idx = cuda_nn.ball_query(q_xyz.contiguous(), xyz.contiguous(), radius, n_neighbor)
    rk = rotated_kernels(anchors, kernels)
    mult = multinv = rot = q_rot = None
    ident = 0
    if pose is not None:
        rot = pose.contiguous()
        q_rot = rot if q_pose is None else q_pose.contiguous()
        _check_pose(rot, torch.float64)
        if permute:
            mult, ident = _group_tables(anchors)
            if mult is None:
                if _anchor_map(ball_idx, q_rot.float(), rot.float(), anchors.float()) is not None:
                    raise NotImplementedError('anchor permutation with per-point poses over an anchor set that is not a group (kanchor 20 / 40) '
                                              'has no float64 kernel: float32, or poses that leave the anchors in place')
                ident = 0
            else:
                multinv = _group_tables_inverse(mult)
    g, r, _ = _hip.so3_prep_f64(q_xyz.contiguous(), xyz.contiguous(), ball_idx, q_rot, rot, anchors.contiguous(), ident)
    return _F64Args(ball_idx, g, r, rk, mult, multinv, sigma)


def _log_f64(forward, c, o, n):
    """the FORWARD_LOG / BACKWARD_LOG entry of a float64 inter conv"""
    if forward and FORWARD_LOG is not None:
        FORWARD_LOG.append({'channels': (c, o), 'dense': False, 'parts': None, 'regime': 'float64'})
    if not forward and BACKWARD_LOG is not None:
        BACKWARD_LOG.append({'channels': (c, o), 'support_rows': n, 'referenced_rows_max': 0, 'regime': 'float64'})


class _GroupContractF64(torch.autograd.Function):
    """The inter and intra convs in float64, one node around a pair (_F64Args, _IntraGrouping): grouping -> Y = W X; backward dW = sum_z
    gY_z X_z^T with X regrouped (never saved), dX = W^T gY -> the grouping's transpose, a slab of clouds at a time (F64_X_BYTES_MAX)."""

    @staticmethod
    def forward(ctx, feats, W_param, grouping):
        feats, W = feats.contiguous(), W_param.contiguous()
        b, c, n, na = feats.shape
        if W.shape[1] != c * grouping.mid:
            raise RuntimeError(f'{grouping.what[0]}: W {tuple(W.shape)} for {c} channels x {grouping.mid} {grouping.what[1]}')
        if grouping.log:
            _log_f64(True, c, W.shape[0], n)
        y = _empty_output(grouping, feats, W)
        _group_contract(grouping, feats, W, y, _f64_slabs(b, 8 * W.shape[1] * y.shape[2] * na), False,
                        lambda W, x, ys, b0: _contract_into(W, x, ys, 0))
        ctx.grouping = grouping
        ctx.save_for_backward(feats, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        feats, W = ctx.saved_tensors
        if ctx.grouping.log:
            _log_f64(False, feats.shape[1], W.shape[0], feats.shape[2])
        slabs = _f64_slabs(feats.shape[0], 8 * W.shape[1] * gy.shape[2] * gy.shape[3])
        gF, gW = _backward_textbook(ctx.grouping, gy.contiguous(), W, feats, None, ctx.needs_input_grad[0], ctx.needs_input_grad[1], slabs)
        return gF, gW, None


class _ContractF64(torch.autograd.Function):
    """_Contract in float64: y[b,o,pa] = W[o,ck] x[b,ck,pa] on v_mfma_f64_16x16x4_f64 (BasicSO3Conv, modules.py:L48-55)."""

    @staticmethod
    def forward(ctx, W, x):
        W, x = W.contiguous(), x.contiguous()
        y = torch.empty(x.shape[0], W.shape[0], x.shape[2], dtype=torch.float64, device=x.device)
        _hip.matmul(W, x, y)
        ctx.save_for_backward(W, x)
        return y

    @staticmethod
    def backward(ctx, gy):
        W, x = ctx.saved_tensors
        gy = gy.contiguous()
        gW = gx = None
        if ctx.needs_input_grad[1]:
            gx = torch.empty_like(x)
            _hip.matmul(W.t(), gy, gx)
        if ctx.needs_input_grad[0]:
            gW = torch.empty_like(W)
            _hip.matmul_reduce(gy, x.transpose(1, 2), gW)
        return gW, gx


# ------------------------------------------------------------------------------------------------
# grouping entry points
# ------------------------------------------------------------------------------------------------
def _strided_centres(xyz, pose, stride, lazy_sample):
    """Centres of a strided conv (functional.py:L931-934 -> spconv/functional.py:L468-477): ceil(p / stride)
    points, furthest-point sampled (native FPS kernel) or, with lazy_sample, the first ones.
    -> sample_idx int32 [b,p2], sample_xyz [b,3,p2], sampled_pose [b,p2,4,4] or None."""
    n_sample = math.ceil(xyz.shape[2] / stride)
    sample_idx, sample_xyz = pctk.furthest_sample(xyz, n_sample, lazy_sample)
    # (group_nd returns float32 for any input, as the reference's: a float64 cloud gets its centres back in float64 -- float32 numbers widened)
    sample_xyz = sample_xyz.to(xyz.dtype)
    sampled_pose = None if pose is None else batched_index_select(pose, 1, sample_idx.long()).contiguous()
    return sample_idx, sample_xyz.contiguous(), sampled_pose


def _check_inputs(xyz, feats, W=None, on_device=True, float32_only=None):
    """-> the call's dtype (_call_dtype).  float32_only: the name of a variant the float64 regime does not cover -- float64 is refused"""
    dtype = _call_dtype('so3conv', feats=feats, xyz=xyz, W=W)
    if dtype == torch.float64 and float32_only is not None:
        raise RuntimeError(f'{float32_only}: float32 only -- the float64 regime covers the plain inter and intra convs, not this variant')
    _hip.check_input(xyz)
    if on_device and not (feats.is_cuda and (W is None or W.is_cuda)):
        raise RuntimeError('so3conv: feats must be a device tensor' if W is None else 'so3conv: feats and W must be device tensors')
    return dtype


def _check_pose(rot, dtype=torch.float32):
    """pose [b,p,4,4] of the call's width (a float64 call: on the device; its width was checked with the other tensors, _call_dtype)"""
    if dtype == torch.float64:
        if rot.shape[-2:] != (4, 4) or not rot.is_cuda:
            raise RuntimeError('so3conv: pose must be a float64 device tensor [b,p,4,4] in a float64 call')
    elif rot.shape[-2:] != (4, 4) or rot.dtype != torch.float32:
        raise RuntimeError('so3conv: pose must be float32 [b,p,4,4]')


def _anchor_map(idx, q_rot, rot, anchors):
    """The anchor index of a conv that permutes by poses over an anchor set that is NOT a group (kanchor 20 / 40: subsets of the
    icosahedral rotations, L2641-2649).  There the reference's argmax_j tr(R_rel^T A_a A_j^T) (L1199-1204) depends on the actual R_rel --
    no [na,na] table stands for it -- and it is no permutation, so it is searched per entry (csrc/so3_anchor_map.hip).
    -> amap uint8 [b,p,nn,na], or None when every entry of the batch maps every anchor onto itself (identity poses, one rotation per
    cloud): the conv then runs exactly as without permutation.  One host read."""
    na = anchors.shape[0]
    if na % 4 != 0 or na > 64:
        raise NotImplementedError('anchor permutation with per-point poses over an anchor set that is not a group: a multiple of 4 anchors, at most 64')
    amap, nontrivial = _hip.so3_anchor_map(idx, q_rot, rot, anchors.contiguous())
    return amap if int(nontrivial.max()) != 0 else None


def _permutation_tables(anchors, idx, q_rot, rot):
    """What a conv that permutes the anchor axis by the relative rotations of (q_rot, rot) over the lists idx needs: (mult, ident, None)
    of _group_tables for a closed anchor set, (None, 0, amap) of _anchor_map otherwise"""
    mult, ident = _group_tables(anchors)
    if mult is None:
        return None, 0, _anchor_map(idx, q_rot, rot, anchors)
    return mult, ident, None


def _neighbourhood(xyz, pose, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz, q_pose, epilogue=None):
    """The shared front of the inter convs: ball query around the centres q_xyz (default: every point), rotated kernels, pose checks, the
    anchor group's tables when the poses permute the anchor axis, offsets + relative-rotation anchors (so3_prep) -> _InterConvArgs."""
    q_xyz = xyz if q_xyz is None else q_xyz
    ball_idx = cuda_nn.ball_query(q_xyz, xyz, radius, n_neighbor)
    rk = rotated_kernels(anchors, kernels)
    mult, ident, amap = None, 0, None
    rot = q_rot = None
    if pose is not None:
        rot = pose.contiguous()
        q_rot = rot if q_pose is None else q_pose.contiguous()
        _check_pose(rot)
        if permute:
            mult, ident, amap = _permutation_tables(anchors, ball_idx, q_rot, rot)
    gx, nonident = _hip.so3_prep(q_xyz, xyz, ball_idx, q_rot, rot, anchors.contiguous(), ident)
    return _InterConvArgs(ball_idx, gx, rk, mult, sigma, ident, nonident, anchors, epilogue, (q_xyz.contiguous(), xyz.contiguous(), q_rot, rot),
                          amap=amap)


def _inter_group(xyz, pose, feats, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz=None, q_pose=None):
    if _check_inputs(xyz, feats) == torch.float64:
        a = _neighbourhood_f64(xyz, pose, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz, q_pose)
        return a.idx, _inter_w(InterWeights(a.g, a.rk, sigma, a.r)), _Group.apply(feats, a)
    a = _neighbourhood(xyz, pose, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz, q_pose)
    return a.idx, _inter_w(InterWeights(a.gx, a.rk, sigma)), _Group.apply(feats, _inter_grouping(a))


def inter_so3conv_fused(xyz, pose, feats, W, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz=None, q_pose=None,
                        epilogue=None):
    """ball query + prep + fused (grouping . contraction) -> (ball_idx, InterWeights, y [b,o,p,a]).
    What InterSO3PoseConv / InterSO3Conv.forward run; q_xyz / q_pose = the sampled centres of a strided conv
    (default: every point is a centre).  epilogue: a FoldedEpilogue the contraction may apply (inference only)."""
    if _check_inputs(xyz, feats, W) == torch.float64:
        if epilogue is not None:
            raise RuntimeError('so3conv: conv_norm_act epilogues (FoldedEpilogue, TrainEpilogue) are float32 only, a float64 conv takes none')
        a = _neighbourhood_f64(xyz, pose, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz, q_pose)
        return a.idx, _inter_w(InterWeights(a.g, a.rk, sigma, a.r)), _GroupContractF64.apply(feats, W, a)
    a = _neighbourhood(xyz, pose, n_neighbor, anchors, kernels, radius, sigma, permute, q_xyz, q_pose, epilogue)
    bn_w = bn_b = None
    if isinstance(epilogue, TrainEpilogue):
        bn_w, bn_b = epilogue.norm.weight, epilogue.norm.bias
    return a.idx, _inter_w(InterWeights(a.gx, a.rk, sigma)), _InterConv.apply(feats, W, bn_w, bn_b, a)


def inter_so3conv_fused_art_mode(xyz, pose, feats, W, seg_labels, n_neighbor, anchors, kernels, radius, sigma, permute):
    """The stride-1 branch of inter_so3poseconv_grouping_strided_arti_mode (functional.py:L1420-1520) + the contraction:
    xyz [b, ns, 3, p] holds the cloud in ns articulation states; every state gets its own ball query, and point p takes the
    neighbour list and the (UNROTATED) offset vectors of state seg_labels[b, p]; the relative rotations of the poses only
    select the anchor permutation.  -> (InterWeights, y [b,o,p,a]).  Runs on the fused kernels: per-state ball query +
    offsets (eap_so3_prep_f32 without poses), the selection by label, the relative-rotation anchors from a second prep call
    on the selected lists, then the same autograd node as the regular conv."""
    if xyz.dim() != 4 or xyz.shape[2] != 3:
        raise RuntimeError('use_art_mode: xyz must be [b, n_states, 3, p]')
    if seg_labels is None:
        raise RuntimeError('use_art_mode: the per-point state labels `seg` are required')
    _check_inputs(xyz, feats, W, on_device=False, float32_only='use_art_mode')
    b, ns, _, p = xyz.shape
    flat = xyz.reshape(b * ns, 3, p).contiguous()
    idx_all = cuda_nn.ball_query(flat, flat, radius, n_neighbor)                                     # [b*ns, p, nn]
    gx_all, _ = _hip.so3_prep(flat, flat, idx_all, None, None, anchors.contiguous(), 0)              # offsets x_n - x_p per state
    nn = idx_all.shape[2]
    pick = seg_labels.long().view(b, 1, p, 1)
    ball_idx = idx_all.view(b, ns, p, nn).gather(1, pick.expand(b, 1, p, nn)).squeeze(1).contiguous()
    gx = gx_all.view(b, ns, p, nn, 4).gather(1, pick.unsqueeze(-1).expand(b, 1, p, nn, 4)).squeeze(1).contiguous()
    rk = rotated_kernels(anchors, kernels)
    mult = nonident = amap = None
    ident = 0
    if pose is not None and permute:
        rot = pose.contiguous()
        _check_pose(rot)
        mult, ident, amap = _permutation_tables(anchors, ball_idx, rot, rot)
        # the nearest anchor of every pair's relative rotation (4th word of gx) and the per-cloud "not all identity" flag; the
        # rotated offsets this call also produces are not used in this mode
        first = xyz[:, 0].contiguous()
        g_rot, nonident = _hip.so3_prep(first, first, ball_idx, rot, rot, anchors.contiguous(), ident)
        gx = torch.cat([gx[..., :3], g_rot[..., 3:]], dim=-1).contiguous()
    y = _InterConv.apply(feats, W, None, None, _InterConvArgs(ball_idx, gx, rk, mult, sigma, ident, nonident, anchors, amap=amap))
    return _inter_w(InterWeights(gx, rk, sigma)), y


# ------------------------------------------------------------------------------------------------
# the `use_2d` variant (functional.py:L1718-2130, modules.py:L249-255; scripts/train/eyeglasses.sh): an anchor axis of
# (na, 4) -- every anchor times four residual rotations about the y axis
# ------------------------------------------------------------------------------------------------
_RES_2D = {}
SLOW_2D_CHUNK = 64      # query points per slab of the tensor form of the really permuted 2-D conv
FORCE_GENERAL_2D = False    # test knob: the tensor form at any size, even when no residual index is permuted
KERNEL_2D_MIN_POINTS = SLOW_2D_CHUNK + 1     # clouds of at least this many points take the 'residual map' kernels, see _conv_2d


def _res_rot_2d(device):
    r = _RES_2D.get(str(device))
    if r is None:
        r = _RES_2D[str(device)] = RES_ROT_2D.to(device)
    return r


def residual_rotation_index(pose, ball_idx, chunk=512):
    """rotated_anchor_idx int64 [b,p,nn,4] of the 2-D variant (functional.py:L1934-1938): per entry and residual rotation z the
    index j maximising tr(R_rel^T RES_z RES_j^T), R_rel = R_p R_n^T -- the reference's expression, evaluated on the device a slab
    of points at a time."""
    res = _res_rot_2d(pose.device)
    rot = pose[:, :, :3, :3].contiguous()
    b, p = rot.shape[:2]
    out = []
    for s0 in range(0, p, chunk):
        idx = ball_idx[:, s0:s0 + chunk].long()
        grouped = batched_index_select_other(rot, idx, dim=1)                                       # [b,pc,nn,3,3]
        rel = torch.matmul(rot[:, s0:s0 + chunk].unsqueeze(2), grouped.transpose(3, 4).contiguous())
        ra = torch.matmul(rel.transpose(-1, -2).contiguous().unsqueeze(3), res)                      # [b,pc,nn,4,3,3]
        d = torch.matmul(ra.unsqueeze(4), res.unsqueeze(0).transpose(2, 3).contiguous())            # [b,pc,nn,4,4,3,3]
        out.append(torch.argmax(d[..., 0, 0] + d[..., 1, 1] + d[..., 2, 2], dim=-1))
    return torch.cat(out, dim=1)


def _conv_2d(xyz, pose, feats, W, n_neighbor, anchors, kernels, radius, sigma, permute, contract=True):
    """Stride-1 branch of inter_so3poseconv_grouping_strided_2D (+ the contraction when `contract`).  feats [b,c,p,na*4].

    With the residual index unpermuted -- permute_modes == 0, or every entry's relative rotation closest to the identity among
    the four residual rotations (identity poses: what the shipped model feeds) -- output anchor (a, z) reads feature anchor (a, z)
    only, with the weights of rotation A_a RES_z: FOUR ordinary convolutions on the fused kernels, one per residual rotation,
    over the anchor sets {A_a RES_z}_a (the poses still rotate the offsets).

    With a really permuted residual index (one rotation per rigid part, one per point) -- the 'residual map' regime: the index as one
    byte per entry (eap_so3_residual_index_f32; one host read of its per-cloud flags, as _anchor_map), the grouping through it for all
    240 anchors at once and its transpose without float atomics (csrc/so3_inter_res.hip), ONE autograd node (_InterConv for the module,
    _Group for the functional grouping API).

    KERNEL_2D_MIN_POINTS: a cloud of at most one slab (p <= SLOW_2D_CHUNK) keeps the reference's expression in device tensor ops -- there
    it materialises everything exactly once, a few MB, and it is the form the 40-point reference-made fixture pins (the fixture's test
    asserts that the materialised weights were asked for).  FORCE_GENERAL_2D selects that tensor form at any size, a slab of
    SLOW_2D_CHUNK query points at a time: the comparator the tests hold the kernels against, with residual_rotation_index as the tensor
    statement of the index."""
    _check_inputs(xyz, feats, float32_only='use_2d')
    b, c, p, na4 = feats.shape
    na = anchors.shape[0]
    if na4 != 4 * na:
        raise RuntimeError(f'use_2d: feats must carry {na} x 4 anchors, got {na4}')
    res = _res_rot_2d(feats.device)
    tot = torch.matmul(anchors.unsqueeze(1), res.unsqueeze(0)).contiguous()                          # [na,4,3,3] = A_a RES_z (L1921)
    ball_idx = cuda_nn.ball_query(xyz, xyz, radius, n_neighbor)
    shift = packed = None
    if permute and pose is not None:
        if FORCE_GENERAL_2D or p < KERNEL_2D_MIN_POINTS:
            shift = residual_rotation_index(pose, ball_idx)
            if not FORCE_GENERAL_2D and bool((shift == torch.arange(4, device=shift.device)).all()):
                shift = None
        else:
            rot = pose.contiguous()
            _check_pose(rot)
            packed, nontrivial = _hip.so3_residual_index(ball_idx, rot, rot, res)
            if int(nontrivial.max()) == 0:            # (one host read) unpermuted: the four fused convolutions below
                packed = None
    if packed is not None:
        rk = rotated_kernels(tot.view(na4, 3, 3), kernels)                                           # [na*4,ks,3]
        gx, _ = _hip.so3_prep(xyz, xyz, ball_idx, rot, rot, anchors.contiguous(), 0)                  # rotated offsets (L1859-1862)
        a = _InterConvArgs(ball_idx, gx, rk, None, sigma, 0, shift=packed)
        y = _InterConv.apply(feats, W, None, None, a) if contract else _Group.apply(feats, _MapGrouping(a))
        return ball_idx, InterWeights(gx, rk, sigma), y
    f5 = feats.contiguous().view(b, c, p, na, 4)
    if shift is None:
        outs = []
        for z in range(4):
            fz = f5[..., z].contiguous()
            az = tot[:, z].contiguous()
            if contract:
                outs.append(inter_so3conv_fused(xyz, pose, fz, W, n_neighbor, az, kernels, radius, sigma, False)[2])
            else:
                outs.append(_inter_group(xyz, pose, fz, n_neighbor, az, kernels, radius, sigma, False)[2])
        y = torch.stack(outs, dim=-1)
        y = y.view(*y.shape[:-2], na4)
        rk = rotated_kernels(tot.view(na4, 3, 3), kernels)
        gx, _ = _hip.so3_prep(xyz, xyz, ball_idx, None if pose is None else pose.contiguous(), None if pose is None else pose.contiguous(),
                              anchors.contiguous(), 0)
        return ball_idx, InterWeights(gx, rk, sigma), y
    # the tensor form of the really permuted case (small clouds, FORCE_GENERAL_2D)
    rk = rotated_kernels(tot.view(na4, 3, 3), kernels)                                               # [na*4,ks,3]
    rot = pose.contiguous()
    gx, _ = _hip.so3_prep(xyz, xyz, ball_idx, rot, rot, anchors.contiguous(), 0)                      # rotated offsets (L1859-1862)
    ks = kernels.shape[0]
    fs = torch.cat([f5, torch.zeros(b, c, 1, na, 4, dtype=feats.dtype, device=feats.device)], dim=2)  # shadow row (L1944)
    trans = fs.permute(0, 2, 3, 4, 1)                                                                # [b,p+1,na,4,c]
    outs = []
    for s0 in range(0, p, SLOW_2D_CHUNK):
        s1 = min(p, s0 + SLOW_2D_CHUNK)
        w = _hip.so3_inter_weights(gx[:, s0:s1].contiguous(), rk, float(sigma)).view(b, s1 - s0, na, 4, ks, -1)     # [b,pc,na,4,ks,nn]
        idx = ball_idx[:, s0:s1].long()
        g = batched_index_select_other(trans, idx, dim=1)                                            # [b,pc,nn,na,4,c]
        sel = shift[:, s0:s1, :, None, :, None].expand(-1, -1, -1, na, -1, c)
        g = torch.gather(g, 4, sel)                                                                  # feature residual index per (entry, z) (L1954-1957)
        x = torch.einsum('bpnazc,bpazkn->bckpaz', g, w).reshape(b, c, ks, s1 - s0, na4)              # (L2124)
        outs.append(so3_contract(W, x.reshape(b, c * ks, (s1 - s0) * na4).contiguous()).view(b, W.shape[0], s1 - s0, na4) if contract else x)
    return ball_idx, InterWeights(gx, rk, sigma), torch.cat(outs, dim=2 if contract else 3)


def inter_so3conv_fused_2d(xyz, pose, feats, W, n_neighbor, anchors, kernels, radius, sigma, permute):
    """What InterSO3PoseConv(use_2d=True).forward runs for stride 1 -> (InterWeights, y [b,o,p,na*4])."""
    if W.dtype != torch.float32 or not W.is_cuda:
        raise RuntimeError('use_2d: W must be a float32 device tensor (float32 only: the float64 regime does not cover this variant)')
    _, w, y = _conv_2d(xyz, pose, feats, W, n_neighbor, anchors, kernels, radius, sigma, permute, contract=True)
    return _inter_w(w), y


def inter_so3poseconv_grouping_strided_2D(xyz, pose, feats, stride, n_neighbor, anchors, kernels, radius, sigma, inter_idx=None,
                                          inter_w=None, lazy_sample=True, radius_expansion=1.0, pooling=None, permute_modes=0):
    """Grouping of the `use_2d` variant (functional.py:L1718-2130), stride-1 branch (L1812-2128: the neighbourhood is recomputed,
    inter_idx handed back unchanged).  -> inter_idx, inter_w, new_xyz, new_feats [b,c,ks,p,na*4], sample_idx, sampled_pose.
    The strided branch of the reference (L1754-1810) applies the 60-anchor expressions to the 240-anchor features and cannot run
    as written; the shipped configuration forces stride 1 (...pn_38_multi_stage.py:L2191)."""
    if pooling is not None and stride > 1 and feats.shape[1] > 1:
        raise ValueError('xyz_pooling is not None?!!')                 # functional.py:L1737
    if inter_idx is None and stride > 1:
        raise NotImplementedError('use_2d with stride > 1: the reference\'s strided branch (functional.py:L1754-1810) does not match its 240-anchor features')
    _, w, new_feats = _conv_2d(xyz, pose, feats, None, n_neighbor, anchors, kernels, radius, sigma, permute_modes != 0, contract=False)
    return inter_idx, _inter_w(w), xyz, new_feats, None, pose


def inter_so3conv_grouping(xyz, feats, stride, n_neighbor, anchors, kernels, radius, sigma,
                           inter_idx=None, inter_w=None, lazy_sample=True, radius_expansion=1.0,
                           pooling=None):
    """Pose-free grouping (functional.py:L144-203), any stride.
    -> inter_idx [b,p2,nn], inter_w, new_xyz, new_feats [b,c,ks,p2,na], sample_idx."""
    if pooling is not None and stride > 1 and feats.shape[1] > 1:
        # low-pass blur before a strided conv (functional.py:L158-173)
        if pooling == 'stride':
            pool_stride, stride_nn, stride = stride, int(n_neighbor * stride ** 0.5), 1
        elif pooling == 'no-stride':
            pool_stride, stride_nn = 1, n_neighbor
        else:
            raise NotImplementedError(f"Pooling mode {pooling} is not implemented!")
        feats, xyz = inter_so3conv_blurring(xyz, feats, stride_nn, radius, pool_stride, inter_idx, lazy_sample)
        inter_idx = None
    if inter_idx is None:
        if stride > 1:
            sample_idx, new_xyz, _ = _strided_centres(xyz, None, stride, lazy_sample)
        else:
            new_xyz = xyz
            sample_idx = torch.arange(xyz.shape[2], dtype=torch.long, device=xyz.device).unsqueeze(0).repeat(xyz.shape[0], 1)
        inter_idx, inter_w, new_feats = _inter_group(xyz, None, feats, n_neighbor, anchors, kernels,
                                                     radius * radius_expansion, sigma, False, q_xyz=new_xyz)
        return inter_idx, inter_w, new_xyz, new_feats, sample_idx
    # cached neighbourhood from an earlier layer (functional.py:L195-201)
    if isinstance(inter_w, InterWeights) and _call_dtype('inter_so3conv_grouping', feats=feats, inter_w=inter_w.gx) == torch.float64:
        new_feats = _Group.apply(feats, _F64Args(inter_idx, inter_w.gx, inter_w.r, inter_w.rk, None, None, inter_w.sigma))
    elif isinstance(inter_w, InterWeights):
        new_feats = _Group.apply(feats, _ListGrouping(_InterConvArgs(inter_idx, inter_w.gx, inter_w.rk, None, inter_w.sigma, 0)))
    else:
        new_feats = inter_so3conv_feat_grouping(inter_idx, inter_w, zpconv.add_shadow_feature(feats))
    return inter_idx, inter_w, xyz, new_feats, None


def inter_so3poseconv_grouping_strided(xyz, pose, feats, stride, n_neighbor, anchors, kernels, radius,
                                       sigma, inter_idx=None, inter_w=None, lazy_sample=True,
                                       radius_expansion=1.0, pooling=None, permute_modes=0):
    """Pose-aware grouping (functional.py:L896-1286).  stride > 1 with no cached index: centres are
    furthest-point sampled, poses gathered, the ball query runs centres -> all points with the expanded
    radius (L931-1013) and the returned inter_idx is None (L1013); otherwise the stride-1 branch (L1025-1261:
    the neighbourhood is recomputed on every call, passed-in inter_idx / inter_w are ignored and inter_idx is
    handed back unchanged).
    -> inter_idx, inter_w, new_xyz, new_feats [b,c,ks,p2,na], sample_idx, sampled_pose."""
    if pooling is not None and stride > 1 and feats.shape[1] > 1:
        raise ValueError('xyz_pooling is not None?!!')                 # functional.py:L913
    if inter_idx is None and stride > 1:
        sample_idx, new_xyz, sampled_pose = _strided_centres(xyz, pose, stride, lazy_sample)
        _, w, new_feats = _inter_group(xyz, pose, feats, n_neighbor, anchors, kernels, radius * radius_expansion, sigma,
                                       permute_modes != 0, q_xyz=new_xyz, q_pose=sampled_pose)
        return None, w, new_xyz, new_feats, sample_idx.long(), sampled_pose          # spconv/functional.py:L476 `idx.long()`
    _, w, new_feats = _inter_group(xyz, pose, feats, n_neighbor, anchors, kernels, radius, sigma,
                                   permute_modes != 0)
    return inter_idx, w, xyz, new_feats, None, pose


def intra_so3conv_grouping(intra_idx, feature):
    """intra_idx [na,pnn], feature [nb,c,np,na] -> [nb,c,pnn,np,na] (functional.py:L2553-2602)."""
    if not feature.is_cuda:
        raise RuntimeError('intra_so3conv_grouping: device tensors only')
    f64 = _call_dtype('intra_so3conv_grouping', feature=feature) == torch.float64
    return _Group.apply(feature, _IntraGrouping(intra_idx, 'f64' if f64 else 'f32'))


def intra_so3conv_grouping_2D(intra_idx, feature):
    """The 2-D variant (functional.py:L2606-2628): the anchor axis is (na, 4); the 12-tap gather acts on na.
    feature [nb,c,np,na*4] -> [nb,c,pnn,np,na*4].  float32 device tensors: one kernel each way (_IntraGrouping '2d'); anything else: the
    reference's tensor expression (a view + one gather)."""
    nb, c_in, nq, tot_na = feature.shape
    if feature.is_cuda and feature.dtype == torch.float32:
        return _Group.apply(feature, _IntraGrouping(intra_idx, '2d'))
    f = feature.contiguous().view(nb, c_in, nq, -1, 4)
    na = f.size(-2)
    _, pnn = intra_idx.shape
    f1 = f.index_select(3, intra_idx.view(-1)).view(nb, c_in, nq, na, pnn, 4)
    return f1.permute([0, 1, 4, 2, 3, 5]).contiguous().view(nb, c_in, pnn, nq, tot_na).contiguous()


def anchor_permutation_index(xyz, pose, n_neighbor, anchors, radius):
    """The reference's rotated_anchor_idx int64 [b,p,nn,na] (functional.py:L1199-1204); test hook."""
    ball_idx = cuda_nn.ball_query(xyz, xyz, radius, n_neighbor)
    mult, ident = _group_tables(anchors)
    if mult is None:          # not a group: the per-entry search (csrc/so3_anchor_map.hip)
        return _hip.so3_anchor_map(ball_idx, pose.contiguous(), pose.contiguous(), anchors.contiguous())[0].long()
    gx, _ = _hip.so3_prep(xyz, xyz, ball_idx, pose.contiguous(), pose.contiguous(), anchors.contiguous(), ident)
    return _hip.so3_anchor_perm(gx, mult)


# ------------------------------------------------------------------------------------------------
# PointnetSO3Conv: the 1x1 embed fused with the max over the points (csrc/pointnet_max.hip)
# ------------------------------------------------------------------------------------------------
# modules.py:L393-413: embed([feats ; A_a^T (xyz - centre)]).max over the points.  The coordinate channels are a rank-3 term
# (v[o,a,:] = A_a W_x[o,:], a [O,na,3] table), the max is taken inside the product: neither the (c+3)-channel concatenation nor the
# [b,o,n,na] map exists in either direction; the one dense tensor is the gradient to the features, which autograd requires.

POINTNET_MAX_CHANNELS = 2048           # output channels the backward kernel's tables hold (include/eap_hip.h)


def pointnet_max_takes(feats, dim_out):
    """Do the kernels take these features?  float32 device [b,c,n,na], na a multiple of 4 and at most 64 (the rule of the head kernels,
    heads._anchor_rows_vectorise), at most POINTNET_MAX_CHANNELS output channels, no empty dimension."""
    return (feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 4 and min(feats.shape) > 0 and feats.shape[3] % 4 == 0
            and feats.shape[3] <= 64 and 0 < dim_out <= POINTNET_MAX_CHANNELS)


def _pointnet_centre(xyz, member):
    """[b,3]: the mean of every cloud's points, of its members under a mask (what the batch-1 call on the gathered subset subtracts)"""
    if member is None:
        return xyz.mean(2)
    return (xyz * member.unsqueeze(1)).sum(2) / member.sum(1, keepdim=True).clamp(min=1.0)


class _PointnetMax(torch.autograd.Function):
    """feats [b,c,n,na], xyz [b,3,n], weight [o,c+3(,1,1)], bias [o] or None, anchors [na,3,3], member [b,n] float 0/1 or None -> [b,o,na].
    Saved: feats, xyz, weight, arg (and the two small data tensors, anchors and member)."""

    @staticmethod
    def forward(ctx, feats, xyz, weight, bias, anchors, member):
        feats, xyz, anchors = feats.contiguous(), xyz.contiguous(), anchors.contiguous()
        b, c, n, na = feats.shape
        o = weight.shape[0]
        W = weight.contiguous().view(o, c + 3)
        centre = _pointnet_centre(xyz, member).contiguous()
        v = torch.einsum('aji,oi->oaj', anchors, W[:, c:]).contiguous()                      # [o, na, 3]: A_a W_x[o, :]
        wt = W[:, :c].t().contiguous()                                                       # [c, o]: W_f, output channels contiguous
        parts = int(_hip.abi.eap_pointnet_max_parts(n))
        pval = torch.empty(b, parts, o, na, dtype=torch.float32, device=feats.device)
        parg = torch.empty(b, parts, o, na, dtype=torch.int32, device=feats.device)
        out = torch.empty(b, o, na, dtype=torch.float32, device=feats.device)
        arg = torch.empty(b, o, na, dtype=torch.int32, device=feats.device)
        bias_c = None if bias is None else bias.contiguous()
        _hip.call('eap_pointnet_max_fwd_f32', feats, b, c, o, n, na, feats, xyz, centre, member, wt, v, bias_c, pval, parg, out, arg,
                  tag={'flops': 2.0 * b * o * c * n * na, 'shape': ('pointnet_max', b, c, o, n, na)})
        ctx.save_for_backward(feats, xyz, weight, anchors, member, arg)
        ctx.has_bias = bias is not None
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g, _):
        feats, xyz, weight, anchors, member, arg = ctx.saved_tensors
        b, c, n, na = feats.shape
        o = weight.shape[0]
        W = weight.contiguous().view(o, c + 3)
        g = g.contiguous()
        d_feats = d_xyz = d_weight = d_bias = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            d_feats = torch.zeros_like(feats) if ctx.needs_input_grad[0] else None
            d_coords = torch.zeros(b, 3, n, na, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[1] else None
            _hip.call('eap_pointnet_max_bwd_data_f32', g, b, c, o, n, na, g, arg, W, c + 3, d_feats, d_coords)
            if d_coords is not None:
                d_xc = torch.einsum('aji,bina->bjn', anchors, d_coords)                      # gradient of xyz - centre
                total = d_xc.sum(2, keepdim=True)
                d_xyz = d_xc - total / n if member is None else d_xc - member.unsqueeze(1) * (total / member.sum(1).clamp(min=1.0).view(b, 1, 1))
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            centre = _pointnet_centre(xyz, member).contiguous()
            dwp = torch.empty(b, o, c + 4, dtype=torch.float32, device=g.device)
            _hip.call('eap_pointnet_max_bwd_weight_f32', g, b, c, o, n, na, g, arg, feats, xyz, centre, anchors, dwp)
            total = dwp.sum(0, dtype=torch.float64)                                          # the clouds, in float64
            if ctx.needs_input_grad[2]:
                d_weight = total[:, :c + 3].float().reshape(weight.shape)
            if ctx.has_bias and ctx.needs_input_grad[3]:
                d_bias = total[:, c + 3].float()
        return d_feats, d_xyz, d_weight, d_bias, None, None


def _pointnet_max_torch(feats, xyz, weight, bias, anchors, member):
    """the same expression as device tensor ops, for anchor counts the kernels do not take (kanchor = 1, 3)"""
    b, c, n, na = feats.shape
    W = weight.reshape(weight.shape[0], c + 3)
    xc = xyz - _pointnet_centre(xyz, member).unsqueeze(2)
    coords = xc.unsqueeze(-1) if na == 1 else torch.einsum('aji,bjn->bina', anchors, xc)
    y = torch.einsum('oc,bcna->bona', W[:, :c], feats) + torch.einsum('oi,bina->bona', W[:, c:], coords)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if member is not None:
        y = y.masked_fill(member.view(b, 1, n, 1) == 0, float('-inf'))
    return y.max(2)[0]


def pointnet_max(feats, xyz, weight, bias, anchors, member=None, return_arg=False):
    """PointnetSO3Conv's embed + max over the points (modules.py:L393-413) without the concatenation and without the [b,o,n,na] map:
    feats [b,c,n,na], xyz [b,3,n], weight = embed.weight [o,c+3] (or [o,c+3,1,1]), bias [o] or None, anchors [na,3,3] -> [b,o,na].
    member [b,n] (0/1, treated as data; None: every point): the max runs over the members, and the coordinates are centred on the members'
    mean -- what a batch-1 call on the gathered subset computes; non-members receive no gradient.  Gradients reach feats, xyz, weight
    and bias.  return_arg: also the int32 [b,o,na] point that attains every maximum (the lowest of equals)."""
    tensors = [t for t in (feats, xyz, weight, bias, anchors, member) if t is not None]
    if any(not t.is_cuda for t in tensors):
        raise RuntimeError('pointnet_max: device tensors only (no CPU fallback)')
    if any(t.dtype != torch.float32 for t in (feats, xyz, weight, anchors)) or (bias is not None and bias.dtype != torch.float32):
        raise RuntimeError('pointnet_max: float32 only')
    b, c, n, na = feats.shape
    if tuple(xyz.shape) != (b, 3, n) or weight.numel() != weight.shape[0] * (c + 3) or tuple(anchors.shape) != (na, 3, 3) or \
            (member is not None and tuple(member.shape) != (b, n)) or (bias is not None and bias.numel() != weight.shape[0]):
        raise RuntimeError(f'pointnet_max: feats {tuple(feats.shape)}, xyz {tuple(xyz.shape)}, weight {tuple(weight.shape)}, anchors '
                           f'{tuple(anchors.shape)} do not agree ([b,c,n,na], [b,3,n], [o,c+3], [na,3,3], member [b,n])')
    if member is not None:
        member = (member != 0).to(torch.float32).contiguous()
    if not pointnet_max_takes(feats, weight.shape[0]):
        if return_arg:
            raise RuntimeError('pointnet_max: return_arg needs an anchor count the kernels take (a multiple of 4, at most 64)')
        return _pointnet_max_torch(feats, xyz, weight, bias, anchors, member)
    out, arg = _PointnetMax.apply(feats, xyz, weight, bias, anchors, member)
    return (out, arg) if return_arg else out
