"""vgtk.cuda.zpconv -- replaces the pybind module of vgtk/vgtk/cuda/zpconv_cuda.cpp."""
import torch

from .. import _hip


# upper bound of the backward's scratch buffer (the batch is processed in slices that fit).  The reference op needs no
# scratch at all, so the bound is modest (two 4096-point clouds at 64 channels) and a cloud that does not fit (or an allocation that fails) takes the
# scratch-free scatter kernel instead of raising
BWD_WORKSPACE_BYTES = 8 << 30


def _check(idx, w, x):
    _hip.check_input(idx, w, x)
    if idx.dtype != torch.int32:
        raise RuntimeError('zpconv: neighbour index must be int32')
    if w.dtype != x.dtype:
        raise RuntimeError('zpconv: weights and features must have the same dtype')


def inter_zpconv_forward(idx, w, feats):
    """(idx int32 [B,P,A,K,ANN], w T [B,P,A,K,ANN], feats T [B,C,Q,A]) -> T [B,C,K,P,A];
    zpconv_cuda.cpp:L41-56."""
    _check(idx, w, feats)
    b, np_, na, ks, ann = idx.shape
    c, nq = feats.shape[1], feats.shape[2]
    out = torch.empty(b, c, ks, np_, na, dtype=feats.dtype, device=feats.device)
    if feats.dtype == torch.float32:
        # scratch for the device-side index check + the per-point neighbour lists (csrc/zpconv_mfma.hip)
        nbytes = int(_hip.abi.eap_inter_zpconv_fwd_workspace(b, np_, ann))
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=feats.device)
        _hip.call('eap_inter_zpconv_fwd_ws_f32', out, b, np_, nq, na, ks, ann, c, idx, w, feats, out, ws)
        return out
    _hip.call('eap_inter_zpconv_fwd_' + _hip.suffix(feats), out, b, np_, nq, na, ks, ann, c, idx, w, feats, out)
    return out


def inter_zpconv_backward(idx, w, grad, npoint, ordered=None):
    """(idx, w, grad T [B,C,K,P,A], int npoint) -> T [B,C,npoint,A]; zpconv_cuda.cpp:L58-75.
    ordered: no float atomicAdd anywhere.  The float32 on-chip kernel and product pipeline keep the clouds they take (they sum in a
    fixed order already); the clouds they leave, every call that gets no scratch for them and every float64 call go to
    eap_inter_zpconv_bwd_ordered_* instead of the scatter kernel.  None: torch.are_deterministic_algorithms_enabled()."""
    _check(idx, w, grad)
    b, np_, na, ks, ann = idx.shape
    c = grad.shape[1]
    out = torch.empty(b, c, int(npoint), na, dtype=grad.dtype, device=grad.device)
    if _hip.use_ordered(ordered) and b > 0:
        return _backward_ordered_any(idx, w, grad, int(npoint), out, ordered is True)
    if grad.dtype == torch.float32 and b > 0:
        # 1. scatter target on chip (csrc/zpconv_bwd_hot.hip): clouds whose lists reference few support rows, whole batch
        #    in one launch, nothing but the operands moves; the per-cloud status comes back in one small read
        todo = _backward_on_chip(idx, w, grad, out)
        if not todo:
            return out
        if len(todo) < b:
            # the clouds it left, in runs of consecutive clouds (slices, no copies of the 1.5 GB-per-cloud operands): one call per run
            run = [todo[0]]
            for i in todo[1:] + [None]:
                if i is not None and i == run[-1] + 1:
                    run.append(i)
                    continue
                b0, b1 = run[0], run[-1] + 1
                _backward_with_products(idx[b0:b1], w[b0:b1], grad[b0:b1], int(npoint), out[b0:b1])
                run = [i]
            return out
        return _backward_with_products(idx, w, grad, int(npoint), out)
    _hip.call('eap_inter_zpconv_bwd_' + _hip.suffix(grad), out, b, np_, int(npoint), na, ks, ann, c, idx, w, grad, out)
    return out


ORDERED_TABLE_BYTES = 64 << 10      # LDS the ordered intra backward inverts its table in (csrc/native_ordered.hip)
ON_CHIP_BACKWARD = True     # False: always the product pipeline of csrc/zpconv_bwd.hip (A/B runs, tests)


_HOT_VERDICTS = {}          # (storage pointer, version, shape) of an index tensor -> (weakref, clouds the on-chip kernel left)
_HOT_PENDING = []           # [event, pinned status copy, expected clouds, key]: verdict re-checks whose device result has not been looked at yet
VERIFY_REMEMBERED = True    # False: trust the remembered verdict without the asynchronous re-check (A/B timing only)


def _verdict_key(idx):
    return (idx.data_ptr(), idx._version, tuple(idx.shape))


def _check_pending_verdicts(block=False):
    """The remembered verdict of an index tensor is trusted WITHOUT a host read (no stall in a training loop), but every later call
    still gets the kernel's status back asynchronously and it is compared here, at the next call into this module (block=True:
    now).  A mismatch means the index CONTENTS changed under an unchanged version counter (`idx.data.copy_`, memory shared with
    numpy / dlpack, a raw-pointer kernel writing into the buffer): the clouds the on-chip kernel then rejected were not redone, so the
    previous result is wrong -- raise, and forget the verdict.  Contract: an index tensor handed to inter_zpconv_backward is either
    left alone or modified through torch in-place ops (which bump `_version`)."""
    for item in list(_HOT_PENDING):
        ev, host, known, key = item
        if not (block or ev.query()):
            continue
        if block:
            ev.synchronize()
        _HOT_PENDING.remove(item)
        seen = tuple(i for i, s_ in enumerate(host.tolist()) if s_ != 0)
        if seen != tuple(known):
            _HOT_VERDICTS.pop(key, None)
            raise RuntimeError('inter_zpconv_backward: the index tensor\'s contents changed without a version bump (clouds left by the on-chip kernel '
                               f'were {list(known)}, now {list(seen)}); the result of the previous call with it is invalid -- modify index tensors '
                               'through torch in-place ops or pass a new tensor')


def _backward_on_chip(idx, w, grad, out, remember=True):
    """-> clouds still to do (all of them when the shape is not taken).  The verdict depends on the INDEX alone (which clouds
    name a row twice / reference too many rows), so it is remembered per index tensor: a training loop that keeps its
    neighbourhood pays the status read once, and a batch the kernel cannot take at all (padded lists: small radii, sparse or
    partial input) skips its prelude from the second call on.  Re-checked on the device every call: _check_pending_verdicts.
    remember=False: the verdict is read back and neither looked up nor stored (the table of remembered verdicts stays the default path's)."""
    _check_pending_verdicts()
    b, np_, na, ks, ann = idx.shape
    c, nq = grad.shape[1], out.shape[2]
    nbytes = int(_hip.abi.eap_inter_zpconv_bwd_hot_workspace(b, np_, nq, na, ks, ann, c)) if ON_CHIP_BACKWARD else 0
    # (the kernel moves idx, grad and out as 16-byte words; w streams 4 bytes per lane and may start at any element)
    if nbytes <= 0 or any(t.data_ptr() % 16 for t in (idx, grad, out)):
        return list(range(b))
    key = (_verdict_key(idx), c, nq)
    hit = _HOT_VERDICTS.get(key) if remember else None
    known = hit[1] if (hit is not None and hit[0]() is idx) else None
    if known is not None and len(known) == b:
        return list(known)                                   # nothing for the on-chip kernel here (every cloud goes to the product pipeline: correct whatever the index holds)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=grad.device)
    status = torch.empty(b, dtype=torch.int32, device=grad.device)
    _hip.call('eap_inter_zpconv_bwd_hot_f32', out, b, np_, nq, na, ks, ann, c, idx, w, grad, out, ws, status)
    if known is not None:
        # same index, same shapes: the same clouds as last time, no host read now -- the status travels to pinned memory behind the
        # kernel and is compared at the next call
        if VERIFY_REMEMBERED and len(_HOT_PENDING) < 8:
            host = torch.empty(b, dtype=torch.int32, pin_memory=True)
            host.copy_(status, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            _HOT_PENDING.append([ev, host, tuple(known), key])
        return list(known)
    todo = [i for i, s in enumerate(status.tolist()) if s != 0]
    if not remember:
        return todo
    if len(_HOT_VERDICTS) > 64:
        _HOT_VERDICTS.clear()
    import weakref
    _HOT_VERDICTS[key] = (weakref.ref(idx), tuple(todo))
    return todo


def _runs(items):
    """sorted cloud numbers -> [(first, past the last)] of every run of consecutive ones"""
    runs = []
    for i in items:
        if runs and runs[-1][1] == i:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    return [tuple(r) for r in runs]


def _backward_ordered(idx, w, grad, npoint, out, requested):
    """csrc/native_ordered.hip: any 5-D index, either width; the clouds in slices whose scratch (twice the index) stays under
    BWD_WORKSPACE_BYTES.  Where the lists cannot be built or the scratch cannot be had: torch's policy (_hip.no_deterministic), then
    the scatter kernel."""
    b, np_, na, ks, ann = idx.shape
    c = grad.shape[1]
    sfx = _hip.suffix(grad)
    why = None
    if npoint > _hip.INV_LISTS_MAX_ROWS:
        why = f'{npoint} target rows, the inverse lists take {_hip.INV_LISTS_MAX_ROWS}'
    elif na > _hip.GRID_YZ_MAX or c > 16 * _hip.GRID_YZ_MAX:
        why = f'{na} anchors, {c} channels: the ordered kernel takes {_hip.GRID_YZ_MAX} anchors and {16 * _hip.GRID_YZ_MAX} channels'
    ws = None
    if why is None:
        per_cloud = int(_hip.abi.eap_inter_zpconv_bwd_ordered_workspace(1, np_, npoint, na, ks, ann))
        step = min(b, BWD_WORKSPACE_BYTES // max(per_cloud, 1), _hip.GRID_YZ_MAX // max(na, 1))
        if step >= 1:
            try:
                ws = torch.empty((int(_hip.abi.eap_inter_zpconv_bwd_ordered_workspace(step, np_, npoint, na, ks, ann)) + 3) // 4,
                                 dtype=torch.int32, device=grad.device)
            except torch.cuda.OutOfMemoryError:
                ws = None
        if ws is None:
            why = f'{per_cloud} bytes of scratch per cloud cannot be had (BWD_WORKSPACE_BYTES = {BWD_WORKSPACE_BYTES})'
    if why is not None:
        _hip.no_deterministic('inter_zpconv_backward', why, requested=requested)
        _hip.call('eap_inter_zpconv_bwd_' + sfx, out, b, np_, npoint, na, ks, ann, c, idx, w, grad, out)
        return out
    for b0 in range(0, b, step):
        nb = min(step, b - b0)
        _hip.call('eap_inter_zpconv_bwd_ordered_' + sfx, out, nb, np_, npoint, na, ks, ann, c, idx[b0:b0 + nb], w[b0:b0 + nb], grad[b0:b0 + nb],
                  out[b0:b0 + nb], ws)
    return out


def _backward_ordered_any(idx, w, grad, npoint, out, requested):
    """ordered=True.  float64: the ordered kernel.  float32: per run of clouds, the atomics-free paths of the default route where
    they serve a cloud WITHOUT their scatter fall-back -- which they do for a cloud whose index is one list per point (compared here,
    one host read per cloud: this is the deterministic mode, not the fast one), the product pipeline on top of that only for the
    sizes and alignments it takes and with its scratch in hand -- and the ordered kernel for the rest."""
    b, np_, na, ks, ann = idx.shape
    c = grad.shape[1]
    if grad.dtype != torch.float32:
        return _backward_ordered(idx, w, grad, npoint, out, requested)
    shared = [bool((idx[i] == idx[i, :, :1, :1, :]).all()) for i in range(b)] if np_ * na * ks * ann > 0 else [False] * b
    rest = [i for i in range(b) if not shared[i]]
    for b0, b1 in _runs([i for i in range(b) if shared[i]]):
        sl = idx[b0:b1], w[b0:b1], grad[b0:b1], out[b0:b1]
        left = _backward_on_chip(*sl, remember=False)          # (slices are temporaries: nothing to remember a verdict by)
        pipeline = bool(_hip.abi.eap_inter_zpconv_bwd_ws_takes(np_, npoint, na, ks, ann, c))
        for r0, r1 in _runs(left):
            part = [t[r0:r1] for t in sl]
            aligned = all(t.data_ptr() % 16 == 0 for t in (part[0], part[2], part[3]))
            if not (pipeline and aligned and _backward_with_products(part[0], part[1], part[2], npoint, part[3], scatter=False) is not None):
                rest += range(b0 + r0, b0 + r1)
    for b0, b1 in _runs(sorted(rest)):
        _backward_ordered(idx[b0:b1], w[b0:b1], grad[b0:b1], npoint, out[b0:b1], requested)
    return out


def _backward_with_products(idx, w, grad, npoint, out=None, scatter=True):
    """csrc/zpconv_bwd.hip: products in forward order + sorted sums (any number of referenced rows), scratch-free scatter
    kernel when no scratch can be had (scatter=False: None then, nothing launched)."""
    b, np_, na, ks, ann = idx.shape
    c = grad.shape[1]
    if out is None:
        out = torch.empty(b, c, npoint, na, dtype=grad.dtype, device=grad.device)
    # atomics-free path (csrc/zpconv_bwd.hip): scratch for the per-(point, neighbour) products, a few clouds at a time
    per_cloud = int(_hip.abi.eap_inter_zpconv_bwd_workspace(1, np_, int(npoint), na, ann, c))
    step = min(b, BWD_WORKSPACE_BYTES // max(per_cloud, 1))
    ws = None
    if step >= 1:
        try:
            ws = torch.empty((int(_hip.abi.eap_inter_zpconv_bwd_workspace(step, np_, int(npoint), na, ann, c)) + 3) // 4,
                             dtype=torch.int32, device=grad.device)
        except torch.cuda.OutOfMemoryError:
            ws = None
    if ws is None:
        if not scatter:
            return None
        _hip.call('eap_inter_zpconv_bwd_f32', out, b, np_, int(npoint), na, ks, ann, c, idx, w, grad, out)
        return out
    for b0 in range(0, b, step):
        nb = min(step, b - b0)
        _hip.call('eap_inter_zpconv_bwd_ws_f32', out, nb, np_, int(npoint), na, ks, ann, c, idx[b0:b0 + nb], w[b0:b0 + nb], grad[b0:b0 + nb],
                  out[b0:b0 + nb], ws)
    return out


def intra_zpconv_forward(idx, w, feats):
    """(idx int32 [A_out,ANN], w T [A_out,K,ANN], feats T [B,C,P,A_in]) -> T [B,C,K,P,A_out];
    zpconv_cuda.cpp:L77-92."""
    _check(idx, w, feats)
    na_out, ann = idx.shape
    ks = w.shape[1]
    b, c, np_, na_in = feats.shape
    out = torch.empty(b, c, ks, np_, na_out, dtype=feats.dtype, device=feats.device)
    _hip.call('eap_intra_zpconv_fwd_' + _hip.suffix(feats), out, b, np_, na_in, na_out, ks, ann, c, idx, w, feats, out)
    return out


def intra_zpconv_backward(idx, w, grad, anchor_in, ordered=None):
    """(idx, w, grad T [B,C,K,P,A_out], int anchor_in) -> T [B,C,P,anchor_in]; zpconv_cuda.cpp:L94-110.
    ordered: the sum over a, then k, then n ascending with idx[a,n] == a' (eap_intra_zpconv_bwd_ordered_*: no float atomics, the same
    bits every run) instead of the reference's atomicAdd scatter.  None: torch.are_deterministic_algorithms_enabled()."""
    _check(idx, w, grad)
    na_out, ann = idx.shape
    ks = w.shape[1]
    b, c, _, np_, _ = grad.shape
    out = torch.empty(b, c, np_, int(anchor_in), dtype=grad.dtype, device=grad.device)
    if _hip.use_ordered(ordered):
        # (the conditions of intra_ordered in csrc/native_ordered.hip: target rows, lanes, the LDS table, the grid)
        if (int(anchor_in) <= _hip.INV_LISTS_MAX_ROWS and na_out <= 64 and 4 * (int(anchor_in) + 1 + 2 * na_out * ann) <= ORDERED_TABLE_BYTES
                and b <= _hip.GRID_YZ_MAX and c <= _hip.GRID_YZ_MAX):
            _hip.call('eap_intra_zpconv_bwd_ordered_' + _hip.suffix(grad), out, b, np_, int(anchor_in), na_out, ks, ann, c, idx, w, grad, out)
            return out
        _hip.no_deterministic('intra_zpconv_backward', f'{anchor_in} input anchors, a table of {na_out} x {ann}, {b} clouds, {c} channels: the ordered kernel '
                              f'takes {_hip.INV_LISTS_MAX_ROWS} input and 64 output anchors, {ORDERED_TABLE_BYTES} bytes of inverted table in LDS, and '
                              f'{_hip.GRID_YZ_MAX} clouds and channels', requested=ordered is True)
    _hip.call('eap_intra_zpconv_bwd_' + _hip.suffix(grad), out, b, np_, int(anchor_in), na_out, ks, ann, c, idx, w, grad, out)
    return out
