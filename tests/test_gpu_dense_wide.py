"""GPU: the dense product (csrc/so3_dense.hip) for clouds that reference MORE THAN 512 support rows -- the wide tables: 32 membership
words per point, a 64-bit group key, up to 1024 row slots, up to 768 k-steps on the forward's contraction axis.

Clouds (synth_clouds.laptop_batch, radii of the 512-point plan on larger clouds; row counts from the reference's first-nsample-by-index
ball query):   (91, 2, 2048) r = 0.16, nsample 64: 684-711 rows, no padded list      (80, 2, 4096) r = 0.13: 983-998 rows (62-63 of 64 groups)
               (80, 2, 4096) r = 0.12: 1115-1120 rows (over the cap)                 (7, 2, 1024) r = 0.12, nsample 32: 535-543 rows, ~14.5 groups
Oracles: numpy restatements of the table definitions (integer-exact), float64 torch sums of the reference's formulas
(so3conv/functional.py:L2508-2549, L1261), and for whole layers the list kernels the golden fixtures pin (DENSE_MODE 'off').
Bars: those of tests/test_gpu_dense.py, unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_dense import NA, KS, dev, _quat_rot  # noqa: E402,F401

NN = 64


def _cloud(dev, seed, B, P, radius, sigma, nn=NN):
    import synth_clouds
    import vgtk.so3conv.functional as L
    import vgtk.cuda.grouping as cuda_nn
    xyz_np, lab_np, _ = synth_clouds.laptop_batch(seed, B, P)
    xyz = torch.from_numpy(xyz_np).to(dev).contiguous()
    anchors = torch.from_numpy(np.asarray(L.get_anchors(NA), dtype=np.float32)).to(dev)
    kernels = torch.from_numpy(L.get_sphereical_kernel_points_from_ply(0.7 * radius, 1)).to(dev)
    return dict(xyz=xyz, idx=cuda_nn.ball_query(xyz, xyz, radius, nn), rk=L.rotated_kernels(anchors, kernels), sigma=float(sigma), radius=radius,
                labels=lab_np, nn=nn)


def _head(s):
    """-> head, largest row count, rp; the lists must be unpadded (every list names nn distinct rows)"""
    import vgtk.so3conv.functional as L
    idx = s['idx']
    srt = idx.sort(dim=2).values
    assert bool((srt[:, :, 1:] != srt[:, :, :-1]).all()), 'a padded list'
    head = L._ListHead(idx, s['xyz'].shape[2], None, None, dense_probe=(None, None))
    rcap, _ = head.decide()
    head.wait()
    torch.cuda.synchronize()
    return head, rcap, L._dense_rows(rcap, s['xyz'].shape[2])


def _numpy_member(s, head, rp):
    """[B, P, rp] bool: row slot r (the r-th entry of the cloud's referenced rows) is named by p's list"""
    idx = s['idx'].cpu().numpy()
    rows, n_rows = head.rows.cpu().numpy(), head.n_rows.cpu().numpy()
    B, P, _ = idx.shape
    n = s['xyz'].shape[2]
    out = np.zeros((B, P, rp), bool)
    for b in range(B):
        slot_of = np.full(n, -1, np.int64)
        slot_of[rows[b, :n_rows[b]]] = np.arange(n_rows[b])
        sl = slot_of[idx[b]]
        assert sl.min() >= 0 and sl.max() < rp
        out[b][np.arange(P)[:, None], sl] = True
    return out


def _pack_words(bits, words):
    """[.., r] bool -> [.., words] uint32, bit i of word w = row slot 32 w + i"""
    full = np.zeros(bits.shape[:-1] + (32 * words,), np.uint64)
    full[..., :bits.shape[-1]] = bits
    return (full.reshape(bits.shape[:-1] + (words, 32)) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def _numpy_mask_words(member, ks, rp, direction):
    """The definition above dense_mask_kernel for one cloud: bit 16 t + 8 j + e of the dword of (wave tile wt, k-step, lane)  <->  column
    n = 64 wt + 32 j + (lane & 31), contraction index kk = 32 step + 16 t + 8 (lane >> 5) + e; dir 0: kk = point, n = dense index;
    dir 1: kk = dense index, n = point; dense index d = (r / 16) 16 ks + 16 k + r % 16.  member [P, rp] bool (the product's point order)
    -> uint32 [wave tiles, k-steps, 64]"""
    P = member.shape[0]
    nkr = ks * rp
    d = np.arange(nkr)
    g, rem = d // (16 * ks), d % (16 * ks)
    r_of = 16 * g + (rem & 15)
    n_cols, kd = (P, (nkr + 31) // 32 * 32) if direction else (nkr, P)
    wtiles, steps = 4 * ((n_cols + 255) // 256), kd // 32
    # [point (+ padding), dense index (+ padding)]
    big = np.zeros((max(P, 32 * steps if not direction else 64 * wtiles), max(nkr, 64 * wtiles if not direction else 32 * steps)), bool)
    big[:P, :nkr] = member[:, r_of]
    wt = np.arange(wtiles).reshape(-1, 1, 1, 1, 1, 1)
    st = np.arange(steps).reshape(1, -1, 1, 1, 1, 1)
    ln = np.arange(64).reshape(1, 1, -1, 1, 1, 1)
    t = np.arange(2).reshape(1, 1, 1, -1, 1, 1)
    j = np.arange(2).reshape(1, 1, 1, 1, -1, 1)
    e = np.arange(8).reshape(1, 1, 1, 1, 1, -1)
    n = 64 * wt + 32 * j + (ln & 31)
    kk = 32 * st + 16 * t + 8 * (ln >> 5) + e
    vals = big[n, kk] if direction else big[kk, n]
    return (vals.astype(np.uint32) << (16 * t + 8 * j + e).astype(np.uint32)).sum((3, 4, 5), dtype=np.uint64).astype(np.uint32)


def test_wide_tables_against_numpy(dev):
    """member, keys, point order, masks and step lists of both directions at 684-711 referenced rows: integer-exact against numpy."""
    import synth_clouds
    from vgtk import _hip
    _, _, radius, sigma = synth_clouds.backbone_layers(512)[1]
    s = _cloud(dev, 91, 2, 2048, radius, sigma)
    head, rcap, rp = _head(s)
    B, P = 2, 2048
    assert head.dense_possible() and 512 < int(head.n_rows.min()) and rcap <= 1024, head.n_rows
    assert tuple(head.memb.shape) == (B, P, 32)
    member = _numpy_member(s, head, rp)                                        # [B,P,rp]
    assert (member.sum(-1) == NN).all() and member[:, :, 512:].any()
    memb = head.memb.cpu().numpy().view(np.uint32)
    assert np.array_equal(memb, _pack_words(member, 32))
    # keys: bit g = some row of 16 g .. 16 g + 15
    grp = member.reshape(B, P, rp // 16, 16).any(-1)                           # [B,P,G]
    G = grp.shape[2]
    assert G > 32
    want_keys = (grp.astype(np.uint64) << np.arange(G, dtype=np.uint64)).sum(-1, dtype=np.uint64).view(np.int64)
    keys = torch.empty(B, P, dtype=torch.int64, device=dev)
    _hip.call('eap_so3_dense_point_keys_wide', head.memb, B, P, _hip._ptr(head.memb), _hip._ptr(keys))
    assert np.array_equal(keys.cpu().numpy(), want_keys)
    geo = _hip.DenseGeometry(s['xyz'], s['xyz'], head.memb, head.rows, rp, s['rk'], s['sigma'], NN, head.n_rows)
    assert geo.wide and geo.order is not None
    order = np.stack([np.argsort(want_keys[b], kind='stable') for b in range(B)])
    assert np.array_equal(geo.order.cpu().numpy(), order)
    n_rows = head.n_rows.cpu().numpy()
    for direction in (0, 1):
        n_cols = P if direction else KS * rp
        wtiles, steps = 4 * ((n_cols + 255) // 256), ((KS * rp + 31) // 32 * 32 if direction else P) // 32
        words = geo.mask(direction).view(torch.int32)[:B * wtiles * steps * 64].view(B, wtiles, steps, 64).cpu().numpy().view(np.uint32)
        st = geo.steps(direction).cpu().numpy()
        assert st.shape == (B, wtiles // 4, steps + 1)
        short = 0
        for b in range(B):
            want = _numpy_mask_words(member[b][order[b]], KS, rp, direction)
            assert np.array_equal(words[b], want), (direction, b)
            nz = (want.reshape(wtiles // 4, 4, steps, 64) != 0).any((1, 3))     # [column block, k-step]
            for bn in range(wtiles // 4):
                w = np.nonzero(nz[bn])[0]
                w = w if len(w) else np.array([0])
                assert st[b, bn, 0] == len(w) and np.array_equal(st[b, bn, 1:1 + len(w)], w), (direction, b, bn)
                short += len(w) < steps
            if direction:                                                       # nothing is listed past the cloud's own prefix
                assert st[b, :, 1:][np.arange(steps)[None, :] < st[b, :, :1]].max() < ((n_rows[b] + 15) // 16 * 16) * KS // 32
        assert short > 0


def _weights64(s, pts, rows, rp):
    """Wd[b, point of pts, r, a, k] in float64 from the reference's formula x the membership of row r in the point's list"""
    xyz, idx, rk = s['xyz'].double(), s['idx'].long(), s['rk'].double()
    out, mem = [], []
    for b in range(xyz.shape[0]):
        rw = rows[b, :rp].long()
        ok = rw >= 0
        xr = xyz[b][:, rw.clamp(min=0)]                                       # [3, rp]
        g = xr[:, None, :] - xyz[b][:, pts][:, :, None]                       # [3, pq, rp]  x_r - x_p
        d = g.permute(1, 2, 0)[:, :, None, None, :] - rk[None, None]          # [pq, rp, A, K, 3]
        w = torch.relu(1.0 - (d * d).sum(-1) / s['sigma'])
        del d
        member = (idx[b][pts][:, :, None] == rw[None, None, :]).any(1) & ok[None, :]      # [pq, rp]
        out.append(w * member[:, :, None, None].double())
        mem.append(member.double())
    return torch.stack(out), torch.stack(mem)


@pytest.mark.parametrize('o', [128, 256])
def test_products_against_float64_beyond_512_rows(dev, o):
    """Both products over every 8th point of 2048-point clouds (256 query points, 684-711 referenced rows, row slots >= 512 in use) against
    the float64 sums: the bound of tests/test_gpu_dense.py, 1e-6 sum |a||w| + 5e-7 sum |a| over the list members -- masked terms are exact
    zeros, so it does not depend on the row count."""
    import synth_clouds
    from vgtk import _hip
    _, _, radius, sigma = synth_clouds.backbone_layers(512)[1]
    s = _cloud(dev, 91, 2, 2048, radius, sigma)
    head, rcap, rp = _head(s)
    assert rcap > 512
    pts = torch.arange(0, 2048, 8, device=dev)
    pq, B = pts.numel(), 2
    geo = _hip.DenseGeometry(s['xyz'][:, :, pts].contiguous(), s['xyz'], head.memb[:, pts].contiguous(), head.rows, rp, s['rk'], s['sigma'], NN, head.n_rows)
    assert geo.wide
    wd, memb = _weights64(s, pts, head.rows, rp)                              # [B,pq,rp,A,K], [B,pq,rp]
    assert float(memb[:, :, 512:].sum()) > 0 and float(wd[:, :, 512:].max()) > 0.0 and float(wd.max()) > 0.5
    gen = torch.Generator(device=dev).manual_seed(59)
    g = torch.randn(B, o, KS, rp, NA, device=dev, generator=gen) * torch.exp(2 * torch.randn(B, o, 1, 1, NA, device=dev, generator=gen))
    y = _hip.so3_dense_fwd(g.view(B, o, KS, rp * NA), geo, pq)
    ref = torch.einsum('bokra,bprak->bopa', g.double(), wd)
    mag = torch.einsum('bokra,bprak->bopa', g.double().abs(), wd)
    magm = torch.einsum('bokra,bpr->bopa', g.double().abs(), memb)
    assert float(((y.double() - ref).abs() / (1e-6 * mag + 5e-7 * magm).clamp(min=1e-30)).max()) < 1.0
    del g, ref, mag, magm
    gy = torch.randn(B, o, pq, NA, device=dev, generator=gen) * torch.exp(2 * torch.randn(B, o, 1, NA, device=dev, generator=gen))
    z = _hip.so3_dense_bwd(gy, geo).view(B, o, KS, NA, rp)
    ref = torch.einsum('bopa,bprak->bokar', gy.double(), wd)
    mag = torch.einsum('bopa,bprak->bokar', gy.double().abs(), wd)
    magm = torch.einsum('bopa,bpr->boar', gy.double().abs(), memb)[:, :, None]
    assert float(((z.double() - ref).abs() / (1e-6 * mag + 5e-7 * magm).clamp(min=1e-30)).max()) < 1.0


def _run(dev, monkeypatch, mode, s, pose, feats0, W0, c, o):
    """tests/test_gpu_dense.py _layer_run with the cloud's own nsample"""
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    monkeypatch.setattr(L, 'DENSE_MODE', mode)
    torch.manual_seed(2913)
    conv = sptk.InterSO3PoseConv(c, o, 1, 1, s['radius'], s['sigma'], s['nn'], kanchor=NA, permute_modes=1).to(dev)
    with torch.no_grad():
        conv.basic_conv.W.copy_(W0)
    feats = feats0.clone().requires_grad_(True)
    L.BACKWARD_LOG = []
    y = conv(zptk.SphericalPointCloudPose(s['xyz'], feats, None, pose))[3].feats
    gen = torch.Generator(device=dev).manual_seed(21)
    gy = torch.randn(y.shape, device=dev, generator=gen)
    gF, gW = torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)
    log, L.BACKWARD_LOG = L.BACKWARD_LOG, None
    with torch.no_grad():
        y_ng = conv(zptk.SphericalPointCloudPose(s['xyz'], feats0, None, pose))[3].feats
    return y.detach(), gF, gW, log, y_ng


def _inputs(dev, seed, B, P, c, o):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(B, c, P, NA, device=dev, generator=gen), torch.randn(o, c * KS, device=dev, generator=gen) * 0.05


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _check_against_lists(r1, r0, name):
    e = (_rel(r1[0], r0[0]), _rel(r1[1], r0[1]), _rel(r1[2], r0[2]))
    print('%s: rel y %.3g dF %.3g dW %.3g' % ((name,) + e))
    assert e[0] < 2e-5 and e[1] < 2e-5 and e[2] < 5e-5, e


@pytest.mark.parametrize('seed,P,radius,o,rows', [(91, 2048, 0.16, 128, (600, 800)), (91, 2048, 0.16, 256, (600, 800)), (80, 4096, 0.13, 128, (960, 1024))])
def test_whole_layer_forced_against_lists_beyond_512_rows(dev, monkeypatch, seed, P, radius, o, rows):
    """InterSO3PoseConv 64 -> 128 / 256 with the dense product forced / switched off at 684-711 referenced rows, and once close to the cap
    (983-998 rows: 62-63 of the 64 groups, the top key bits and the last membership word): the project's bars; the no-grad forward equals
    the grad-mode one."""
    B, c = 2, 64
    s = _cloud(dev, seed, B, P, radius, 0.5 * radius * radius if radius != 0.16 else 0.0128)
    feats0, W0 = _inputs(dev, 61, B, P, c, o)
    r0 = _run(dev, monkeypatch, 'off', s, None, feats0, W0, c, o)
    r1 = _run(dev, monkeypatch, 'force', s, None, feats0, W0, c, o)
    assert [r['regime'] for r in r1[3]] == ['dense rows'] and r1[3][0]['referenced_rows_max'] > 512, r1[3]
    assert rows[0] < r1[3][0]['referenced_rows_max'] <= rows[1], r1[3]
    assert r0[3][0]['regime'] != 'dense rows'
    _check_against_lists(r1, r0, 'forced %d x %d, o = %d, rows %d' % (B, P, o, r1[3][0]['referenced_rows_max']))
    assert torch.equal(r1[4], r1[0])


def test_skipping_is_exact_beyond_512_rows(dev, monkeypatch):
    """The whole layer with the k-step lists and with every k-step: y, dF, dW bit-equal; the forward's lists (540-576 k-steps on the
    contraction axis: more than the 512 a list once held) are shorter than the axis, and the product RUNS them: a list cut down to its
    first entry changes the result."""
    import synth_clouds
    from vgtk import _hip
    B, P, c, o = 2, 2048, 64, 128
    _, _, radius, sigma = synth_clouds.backbone_layers(512)[1]
    s = _cloud(dev, 91, B, P, radius, sigma)
    feats0, W0 = _inputs(dev, 67, B, P, c, o)
    r1 = _run(dev, monkeypatch, 'force', s, None, feats0, W0, c, o)
    monkeypatch.setattr(_hip, 'SKIP_DENSE_STEPS', False)
    r0 = _run(dev, monkeypatch, 'force', s, None, feats0, W0, c, o)
    monkeypatch.setattr(_hip, 'SKIP_DENSE_STEPS', True)
    assert r1[3][0]['regime'] == r0[3][0]['regime'] == 'dense rows' and r1[3][0]['referenced_rows_max'] > 512
    assert torch.equal(r1[0], r0[0]) and torch.equal(r1[1], r0[1]) and torch.equal(r1[2], r0[2])
    head, rcap, rp = _head(s)
    geo = _hip.DenseGeometry(s['xyz'], s['xyz'], head.memb, head.rows, rp, s['rk'], s['sigma'], NN, head.n_rows)
    st = geo.steps(1)
    k_steps = KS * rp // 32
    assert st.shape[2] - 1 == k_steps and k_steps > 512
    assert int(st[:, :, 0].min()) < k_steps and int(st[:, :, 0].min()) > 1
    g = torch.randn(B, o, KS, rp * NA, device=dev, generator=torch.Generator(device=dev).manual_seed(71))
    y_all = _hip.so3_dense_fwd(g, geo, P)
    cut = st.clone()
    cut[:, :, 0] = 1
    geo._steps[1] = cut
    y_cut = _hip.so3_dense_fwd(g, geo, P)
    assert not torch.equal(y_cut, y_all) and float(y_cut.abs().max()) < float(y_all.abs().max())


def test_rigid_parts_beyond_512_rows(dev, monkeypatch):
    """Two rotations per cloud (the clouds' own two rigid parts), forced: one product per part, the bars against the list kernels."""
    import synth_clouds
    B, P, c, o = 2, 2048, 64, 128
    _, _, radius, sigma = synth_clouds.backbone_layers(512)[1]
    s = _cloud(dev, 91, B, P, radius, sigma)
    R = _quat_rot(np.random.default_rng(7), 4)
    pose_np = np.tile(np.eye(4, dtype=np.float32), (B, P, 1, 1))
    for b in range(B):
        pose_np[b, :, :3, :3] = R[2 * b:2 * b + 2][s['labels'][b] % 2]
        assert 0 < int((s['labels'][b] % 2).sum()) < P
    pose = torch.from_numpy(pose_np).to(dev)
    feats0, W0 = _inputs(dev, 73, B, P, c, o)
    r0 = _run(dev, monkeypatch, 'off', s, pose, feats0, W0, c, o)
    r1 = _run(dev, monkeypatch, 'force', s, pose, feats0, W0, c, o)
    assert r1[3][0]['regime'] == 'dense rows' and r1[3][0].get('parts') == 2 and r1[3][0]['referenced_rows_max'] > 512, r1[3]
    assert r0[3][0]['regime'] != 'dense rows'
    _check_against_lists(r1, r0, 'parts')
    assert torch.equal(r1[4], r1[0])


def test_conv_norm_node_beyond_512_rows(dev, monkeypatch):
    """conv_norm_act with a training-mode BatchNormLeakyReLU inside the conv's node at 684-711 referenced rows against conv + separate
    modules: the bars of tests/test_gpu_dense.py::test_conv_norm_node_against_separate_modules."""
    import synth_clouds
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    B, P, c, o = 2, 2048, 64, 128
    _, _, radius, sigma = synth_clouds.backbone_layers(512)[1]
    s = _cloud(dev, 91, B, P, radius, sigma)
    xyz = s['xyz']
    monkeypatch.setattr(L, 'DENSE_MODE', 'force')
    pose = torch.eye(4, device=dev).repeat(B, P, 1, 1)
    gen = torch.Generator(device=dev).manual_seed(79)
    feats0 = torch.randn(B, c, P, NA, device=dev, generator=gen)
    W0 = torch.randn(o, c * KS, device=dev, generator=gen) * 0.05
    gamma0 = torch.rand(o, device=dev, generator=gen) + 0.5
    gamma0[3] = -0.7
    beta0 = torch.randn(o, device=dev, generator=gen) * 0.3
    gy = torch.randn(B, o, P, NA, device=dev, generator=gen)
    out = {}
    for fused in (False, True):
        monkeypatch.setattr(L, 'FUSE_CONV_NORM', fused)
        torch.manual_seed(2913)
        conv = sptk.InterSO3PoseConv(c, o, 1, 1, radius, sigma, NN, kanchor=NA, permute_modes=1).to(dev)
        norm = sptk.BatchNormLeakyReLU(o, negative_slope=0.01).to(dev)
        with torch.no_grad():
            conv.basic_conv.W.copy_(W0); norm.weight.copy_(gamma0); norm.bias.copy_(beta0)
        feats = feats0.clone().requires_grad_(True)
        L.BACKWARD_LOG = []
        y = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
        grads = torch.autograd.grad(y, [feats, conv.basic_conv.W, norm.weight, norm.bias], gy)
        log, L.BACKWARD_LOG = L.BACKWARD_LOG, None
        assert log[0]['regime'] == 'dense rows' and log[0]['referenced_rows_max'] > 512 and (log[0].get('norm') == 'in the node') == fused, log
        out[fused] = (y.detach(),) + grads + (norm.running_mean.clone(), norm.running_var.clone(), int(norm.num_batches_tracked))
    a, b_ = out[True], out[False]
    e = [_rel(a[i], b_[i]) for i in range(7)]
    print('node: y %.3g dF %.3g dW %.3g dgamma %.3g dbeta %.3g mean %.3g var %.3g' % tuple(e))
    assert e[0] < 1e-5
    assert e[1] < 2e-5 and e[2] < 5e-5
    assert e[3] < 2e-5 and e[4] < 2e-5
    assert e[5] < 1e-5 and e[6] < 1e-5 and a[7] == b_[7] == 1


def test_clouds_over_the_cap_fall_back(dev, monkeypatch):
    """More than 1024 referenced rows (4096 points, r = 0.12: 1115-1120, no padded list), and padded lists at the wide probe width
    (2048 points, r = 0.05): the list kernels even with the product forced, results bit-equal to DENSE_MODE 'off'."""
    import vgtk.so3conv.functional as L
    B, c, o = 2, 16, 128
    s = _cloud(dev, 80, B, 4096, 0.12, 0.5 * 0.12 * 0.12)
    head, rcap, rp = _head(s)                                                  # (asserts that no list is padded)
    assert int(head.n_rows.min()) > 1024 and not head.dense_possible(), head.n_rows
    feats0, W0 = _inputs(dev, 83, B, 4096, c, o)
    r0 = _run(dev, monkeypatch, 'off', s, None, feats0, W0, c, o)
    r1 = _run(dev, monkeypatch, 'force', s, None, feats0, W0, c, o)
    assert r1[3][0]['regime'] != 'dense rows' and all(torch.equal(a, b) for a, b in zip(r0[:3], r1[:3]))
    assert torch.equal(r1[4], r0[4])
    s = _cloud(dev, 91, B, 2048, 0.05, 0.002)
    srt = s['idx'].sort(dim=2).values
    assert bool((srt[:, :, 1:] == srt[:, :, :-1]).any())                       # padded lists
    head = L._ListHead(s['idx'], 2048, None, None, dense_probe=(None, None))
    assert not head.dense_possible()
    feats0, W0 = _inputs(dev, 89, B, 2048, c, o)
    r0 = _run(dev, monkeypatch, 'off', s, None, feats0, W0, c, o)
    r1 = _run(dev, monkeypatch, 'force', s, None, feats0, W0, c, o)
    assert r1[3][0]['regime'] != 'dense rows' and all(torch.equal(a, b) for a, b in zip(r0[:3], r1[:3]))


def test_default_decision_takes_many_rows_in_few_groups(dev, monkeypatch):
    """1024-point clouds, nsample 32, r = 0.12: 535-543 referenced rows, a list touches ~14.5 of their 34 groups -- under the bound of 16 that
    governs every row count: 'auto' runs the product, same results as the list kernels; with the wide bound lowered, back to the lists."""
    import vgtk.so3conv.functional as L
    B, P, c, o = 2, 1024, 64, 128
    s = _cloud(dev, 7, B, P, 0.12, 0.5 * 0.12 * 0.12, nn=32)
    head, rcap, rp = _head(s)
    assert int(head.n_rows.min()) > 512 and rcap <= 1024 and head.dense_possible(), head.n_rows
    assert 8.0 < head.groups_touched() <= 16.0 and L.DENSE_MAX_GROUPS_WIDE >= 16.0, head.groups_touched()
    feats0, W0 = _inputs(dev, 97, B, P, c, o)
    r0 = _run(dev, monkeypatch, 'off', s, None, feats0, W0, c, o)
    r1 = _run(dev, monkeypatch, 'auto', s, None, feats0, W0, c, o)
    assert r1[3][0]['regime'] == 'dense rows' and r1[3][0]['referenced_rows_max'] > 512, r1[3]
    assert r0[3][0]['regime'] != 'dense rows'
    _check_against_lists(r1, r0, 'auto')
    assert torch.equal(r1[4], r1[0])
    monkeypatch.setattr(L, 'DENSE_MAX_GROUPS_WIDE', 4.0)
    r2 = _run(dev, monkeypatch, 'auto', s, None, feats0, W0, c, o)
    assert r2[3][0]['regime'] != 'dense rows'
