"""numpy restatements of what the front end of a training step computes on the device before its big kernels run: the row list of
the inverse neighbour lists (csrc/inv_lists.hip, eap_inv_lists_rows) and the five words the list head hands to the host
(csrc/list_probe.hip, eap_so3_dense_probe).  The ball query's reference is the oracle's (oracle.native.ball_query)."""
import numpy as np

from oracle import native  # noqa: F401  (ball_query: re-exported for the tests)


def row_list(idx, n):
    """idx int [b,p,nn] -> rows, off, cnt int32 [b,n], n_rows int32 [b]: a cloud's referenced rows sorted by count descending, ties by the
    lower index, -1 past the last referenced row; cnt in that order; off the exclusive prefix sum of cnt (slots past the end hold the
    total).  Indices outside [0, n) are not counted."""
    idx = np.asarray(idx)
    b = idx.shape[0]
    rows = np.full((b, n), -1, np.int32)
    cnt = np.zeros((b, n), np.int32)
    off = np.zeros((b, n), np.int32)
    n_rows = np.zeros(b, np.int32)
    for bi in range(b):
        flat = idx[bi].reshape(-1)
        flat = flat[(flat >= 0) & (flat < n)]
        counts = np.bincount(flat, minlength=n)
        order = np.lexsort((np.arange(n), -counts))           # count descending, then index ascending
        k = int((counts != 0).sum())
        rows[bi, :k] = order[:k]
        cnt[bi, :k] = counts[order[:k]]
        off[bi] = np.concatenate([[0], np.cumsum(cnt[bi])[:-1]])
        n_rows[bi] = k
    return rows, off, cnt, n_rows


def probe_words(p, n_rows, nonident=None, dflags=None, memb=None, poses=(), rot_cloud=None, norm_w=None, norm_b=None, ratio=128.0):
    """-> the five int32 words of eap_so3_dense_probe (include/eap_hip.h)."""
    out = np.zeros(5, np.int32)
    out[0] = np.asarray(n_rows).max()
    out[1] = 1 if nonident is None else np.asarray(nonident).max()
    bad = 1 if dflags is None else int(np.asarray(dflags).max())
    eye = np.eye(3, dtype=np.float32)
    for rot in poses:
        bad += int((np.asarray(rot)[..., :3, :3] != eye).any())
    if rot_cloud is not None:
        r = np.asarray(rot_cloud, np.float64)
        d = np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max()      # (a NaN maximum is not above the bar)
        bad += int(d > 1e-6)
    out[2] = bad
    if memb is not None:
        m = np.asarray(memb).view(np.uint32)
        touched = ((m & 0xffff) != 0).sum((1, 2)) + ((m >> 16) != 0).sum((1, 2))
        out[3] = np.int32(np.float32(touched.max()) * np.float32(16.0 / max(p, 1)))
    if norm_w is not None:
        w, bb = np.asarray(norm_w, np.float32), np.asarray(norm_b, np.float32)
        out[4] = int(((np.abs(bb) > np.float32(ratio) * np.abs(w)) & (w != 0)).any())
    return out


def offset_copy(t):
    """a contiguous copy of the device tensor `t` that starts one element (4 bytes in float32 and int32) into its storage"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view
