"""GPU: the dense layers' gradient tail on PACKED Z (eap_so3_dense_product_packed_f32, eap_so3_dense_zbound_packed_f32,
eap_gemm_f16x2_splitk_tail_f32, eap_gemm_bf16x3_reduce_tail_f32, eap_rows_gather_packed_f32, eap_rows_scatter_packed_f32) against the
zero-filled layout it replaces and against float64.

Shapes: the smallest eap_so3_dense_supported takes -- three clouds, na = 60, ks = 24, o = 128 (128-row blocks) and o = 256, p = 288 (one 256-point
block plus a ragged 32-point wave).  The clouds' referenced rows are cut (_targets) to rp, to a multiple of 16 below rp whose live columns
end inside a 128-column tile, and to a count that is not a multiple of 16 (its live columns end inside a tile as well).  With na = 60 a cloud has
960 m live columns, always whole 16-element k-tiles of the reduce kernel, so a live end inside a k-tile cannot come from the layer; the
reduce entry's zero fill of a partial k-tile is exercised by calling it with such counts (test_reduce_tail_ends_inside_a_k_tile).

Every buffer the packed path allocates is handed out full of NaN (torch.empty patched as tools/gpu/uninit_check.py does).

Bars: live columns of Z, the feature-gradient GEMM's output and the scattered dF bit-equal to the zero-filled path; dF <= 2e-5 and dW <= 5e-5
of their largest magnitude against float64 from the zero-filled Z (tests/test_gpu_dense.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NN, NA, KS, C = 64, 60, 24, 128
P = 288


def _targets(fewest):
    """referenced rows per cloud from the smallest natural count: g whole groups of 16 (= rp), the largest odd number of groups below g (a
    multiple of 16 below rp; 960 x odd live columns end inside a 128-column tile), and 11 rows short of an odd number of groups below that"""
    g = fewest // 16
    assert g >= 4, fewest
    g1 = g - 1 if (g - 1) % 2 else g - 2
    return 16 * g, 16 * g1, 16 * (g1 - 2) - 11


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture
def poisoned_empty(monkeypatch):
    """torch.empty / empty_like hand out float device buffers full of NaN while the returned switch is on"""
    on = [False]
    plain, plain_like = torch.empty, torch.empty_like

    def empty(*a, **k):
        t = plain(*a, **k)
        if on[0] and t.is_floating_point() and t.is_cuda:
            t.fill_(float('nan'))
        return t

    def empty_like(*a, **k):
        t = plain_like(*a, **k)
        if on[0] and t.is_floating_point() and t.is_cuda:
            t.fill_(float('nan'))
        return t

    monkeypatch.setattr(torch, 'empty', empty)
    monkeypatch.setattr(torch, 'empty_like', empty_like)
    return on


@pytest.fixture(scope='module')
def case(dev):
    """three clouds whose lists name exactly _targets(..) support rows (the other entries become shadow entries: index n), their list head
    and geometry, random operands -- shared by the tests below, never modified"""
    import numpy as np
    import synth_clouds
    import vgtk.so3conv.functional as L
    import vgtk.cuda.grouping as cuda_nn
    from vgtk import _hip
    _, _, radius, sigma = synth_clouds.backbone_layers(4096)[2]
    B = 3
    xyz = torch.from_numpy(synth_clouds.laptop_batch(11, B, P)[0]).to(dev).contiguous()
    anchors = torch.from_numpy(np.asarray(L.get_anchors(NA), dtype=np.float32)).to(dev)
    kernels = torch.from_numpy(L.get_sphereical_kernel_points_from_ply(0.7 * radius, 1)).to(dev)
    rk = L.rotated_kernels(anchors, kernels)
    idx = cuda_nn.ball_query(xyz, xyz, radius, NN)
    head = L._ListHead(idx, P, None, None, dense_probe=(None, None))
    head.decide(); head.wait()
    targets = _targets(int(head.n_rows.min()))
    keep = torch.zeros(B, P + 1, dtype=torch.bool, device=dev)
    for b, t in enumerate(targets):
        keep[b, head.rows[b, :t].long()] = True
    idx = torch.where(keep.gather(1, idx.long().view(B, -1)).view_as(idx), idx, torch.full_like(idx, P)).contiguous()
    head = L._ListHead(idx, P, None, None, dense_probe=(None, None))
    rcap, _ = head.decide()
    assert head.dense_possible()
    head.wait()
    assert head.n_rows.tolist() == list(targets)
    rp = L._dense_rows(rcap, P)
    assert rp == targets[0]
    geo = _hip.DenseGeometry(xyz, xyz, head.memb, head.rows, rp, rk, float(sigma), NN, head.n_rows)
    gen = torch.Generator(device=dev).manual_seed(5)
    feats = torch.randn(B, C, P, NA, device=dev, generator=gen)
    live = [_hip.dense_live16(t, rp) for t in targets]
    # one cloud at rp, one a multiple of 16 below it, one not a multiple of 16; the two short ones end inside a 128-column tile
    assert live[0] == rp and targets[1] % 16 == 0 and targets[1] < rp and targets[2] % 16 != 0 and live[2] < live[1], (targets, live)
    assert (NA * live[1]) % 128 != 0 and (NA * live[2]) % 128 != 0
    return dict(head=head, geo=geo, rp=rp, feats=feats, ldz=_hip.dense_pitch(NA * rp), live=live, targets=targets)


def _live(x_unpacked, x_packed, case):
    """the live columns of both layouts as lists of [.., na, live16] blocks per cloud"""
    rp, out = case['rp'], []
    for b, lv in enumerate(case['live']):
        u = x_unpacked[b][..., :NA * rp].reshape(*x_unpacked.shape[1:-1], NA, rp)[..., :lv]
        k = x_packed[b][..., :NA * lv].reshape(*x_packed.shape[1:-1], NA, lv)
        out.append((u, k))
    return out


@pytest.mark.parametrize('o', [128, 256])
def test_packed_tail_against_the_zero_filled_layout(dev, case, poisoned_empty, o):
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    head, geo, rp, feats, ldz = case['head'], case['geo'], case['rp'], case['feats'], case['ldz']
    B, ra = 3, NA * rp
    assert _hip.dense_tail_packed_takes(C, o * KS, ra, ldz)
    gen = torch.Generator(device=dev).manual_seed(17 + o)
    gy = torch.rand(B, o, P, NA, device=dev, generator=gen) * 2 - 1
    W = torch.randn(o, C * KS, device=dev, generator=gen) * 0.05
    colmax = gy.abs().amax((1, 2)).contiguous()                       # |Z[o,k,(a,r)]| <= colmax[b,a] x (points that list row r): weights <= 1
    W2 = L._weight_operand(W, C, KS)

    # ---- the zero-filled path, as _backward_dense runs it
    zu = _hip.so3_dense_bwd(gy, geo, ldz)
    words_u = _hip.so3_dense_zbound(colmax, head.cnt, head.n_rows, rp, P, ldz)
    gFr_u = L._rows_grad_from_z(zu, W2, C, rp, NA, ldz, True, (words_u.view(torch.int32), 4, 1.0))
    gF_u = _hip.rows_scatter(gFr_u.contiguous(), head.rows, P)

    # ---- the packed path on poisoned buffers
    poisoned_empty[0] = True
    zp = _hip.so3_dense_bwd(gy, geo, ldz, packed=True)
    words_p, ncols = _hip.so3_dense_zbound_packed(colmax, head.cnt, head.n_rows, rp, P, ldz)
    gFc = torch.empty(B, C, ldz, dtype=torch.float32, device=dev)
    _hip.matmul_tail(W2, zp.view(B, o * KS, ldz), gFc, ncols, (words_p.view(torch.int32), 4, 1.0))
    gF_p = _hip.rows_scatter_packed(gFc, C, head.rows, head.n_rows, rp, P, NA)
    fc = _hip.rows_gather_packed(feats, head.rows, head.n_rows, rp, ldz)
    dt = torch.empty(C, o * KS, dtype=torch.float32, device=dev)
    _hip.matmul_reduce_tail(fc[..., :ra], zp.view(B, o * KS, ldz)[..., :ra].transpose(1, 2), dt, ncols)
    poisoned_empty[0] = False
    gW_p = dt.view(C, o, KS).permute(1, 0, 2).reshape(o, C * KS)

    assert ncols.tolist() == [NA * lv for lv in case['live']]
    # Z, the bound words, the packed feature rows: the zero-filled layout's numbers at the packed positions, NaN (= never written) behind them
    for b, (u, k) in enumerate(_live(zu.view(B, o * KS, ldz), zp.view(B, o * KS, ldz), case)):
        assert torch.equal(u, k), b
        assert bool(torch.isnan(zp.view(B, o * KS, ldz)[b, :, NA * case['live'][b]:]).all()) or NA * case['live'][b] == ldz, b
    for b, lv in enumerate(case['live']):
        assert torch.equal(words_u[b, :ra // 4].view(NA, rp // 4)[:, :lv // 4], words_p[b, :NA * lv // 4].view(NA, lv // 4)), b
        assert float(words_p[b, NA * lv // 4:].abs().sum()) == 0.0
    fc_u = _hip.rows_gather(feats, head.rows, rp).transpose(2, 3).reshape(B, C, ra)
    for b, (u, k) in enumerate(_live(fc_u, fc, case)):
        assert torch.equal(u, k), b
    # dF: the GEMM's live columns and the scattered gradient bit for bit
    gFc_u = gFr_u.transpose(2, 3).reshape(B, C, ra)
    for b, (u, k) in enumerate(_live(gFc_u, gFc, case)):
        assert torch.equal(u, k), b
    assert torch.equal(gF_u, gF_p)
    # float64 from the zero-filled Z
    z64 = zu.view(B, o * KS, ldz)[..., :ra].double()
    gF64 = torch.matmul(W2.double(), z64).view(B, C, NA, rp).transpose(2, 3)
    rows = head.rows[:, :rp].long()
    ref = torch.zeros(B, C, P + 1, NA, dtype=torch.float64, device=dev)
    ref.scatter_(2, torch.where(rows >= 0, rows, torch.full_like(rows, P))[:, None, :, None].expand(B, C, rp, NA), gF64)
    ref = ref[:, :, :P]
    e_f = float((gF_p.double() - ref).abs().max() / ref.abs().max())
    gW64 = torch.einsum('bnr,bcr->nc', z64, fc_u.double()).view(o, KS, C).permute(0, 2, 1).reshape(o, C * KS)
    e_w = float((gW_p.double() - gW64).abs().max() / gW64.abs().max())
    print(f'o = {o}: dF {e_f:.2e} (bar 2e-5), dW {e_w:.2e} (bar 5e-5)')
    assert bool(torch.isfinite(gF_p).all()) and bool(torch.isfinite(gW_p).all())
    assert e_f <= 2e-5 and e_w <= 5e-5, (e_f, e_w)
    assert float(ref.abs().max()) > 0 and float(gW64.abs().max()) > 0


def test_reduce_tail_ends_inside_a_k_tile(dev):
    """eap_gemm_bf16x3_reduce_tail_f32 with live ends inside a 16-element k-tile (and inside a 32-element pair of them), at whole k-tiles per slab,
    at 0 and past K: the operands are NaN behind every item's end; against float64 over the live elements, 5e-5 of the largest magnitude
    (the bar of the weight gradient)."""
    from vgtk import _hip
    gen = torch.Generator(device=dev).manual_seed(3)
    M, N, K = 128, 256, 8192               # eight slabs per item, over the item's own live prefix
    ends = [K, 1029, 1024, 40, 0, K + 77, 3000]
    B = len(ends)
    A = torch.randn(B, M, K, device=dev, generator=gen)
    Bm = torch.randn(B, N, K, device=dev, generator=gen)
    ref = torch.zeros(M, N, dtype=torch.float64, device=dev)
    for b, e in enumerate(ends):
        e = min(e, K)
        ref += A[b, :, :e].double() @ Bm[b, :, :e].double().t()
        A[b, :, e:] = float('nan'); Bm[b, :, e:] = float('nan')
    out = torch.full((M, N), float('nan'), device=dev)
    ncols = torch.tensor(ends, dtype=torch.int32, device=dev)
    assert _hip.matmul_reduce_tail_takes(A, Bm.transpose(1, 2), out)
    _hip.matmul_reduce_tail(A, Bm.transpose(1, 2), out, ncols)
    assert bool(torch.isfinite(out).all())
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    assert err <= 5e-5, err


def test_conv_norm_node_packed_against_zero_filled(dev, monkeypatch):
    """vgtk.so3conv.conv_norm_act forward + backward at 2 x 512 points, forced onto the dense regime, with the packed tail and with the
    zero-filled one: the same regime, dF bit-equal, dW within the layer bar, everything else bit-equal."""
    import synth_clouds
    import vgtk.so3conv as sptk
    import vgtk.spconv as zptk
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    monkeypatch.setattr(L, 'DENSE_MODE', 'force')
    monkeypatch.setattr(L, 'FUSE_CONV_NORM', True)
    B, Pn, o = 2, 512, 256
    _, _, radius, sigma = synth_clouds.backbone_layers(4096)[2]
    xyz = torch.from_numpy(synth_clouds.laptop_batch(71, B, Pn)[0]).to(dev)
    pose = torch.eye(4, device=dev).repeat(B, Pn, 1, 1)
    gen = torch.Generator(device=dev).manual_seed(41)
    feats0 = torch.randn(B, C, Pn, NA, device=dev, generator=gen)
    W0 = torch.randn(o, C * KS, device=dev, generator=gen) * 0.05
    gy = torch.randn(B, o, Pn, NA, device=dev, generator=gen)
    seen, plain_call = [], _hip.call

    def call(name, *a, **k):
        seen.append(name)
        return plain_call(name, *a, **k)

    monkeypatch.setattr(_hip, 'call', call)
    out, logs, names = {}, {}, {}
    for packed in (False, True):
        monkeypatch.setattr(L, 'DENSE_TAIL_PACKED', packed)
        torch.manual_seed(2913)
        conv = sptk.InterSO3PoseConv(C, o, 1, 1, radius, sigma, NN, kanchor=NA, permute_modes=1).to(dev)
        norm = sptk.BatchNormLeakyReLU(o, negative_slope=0.01).to(dev)
        with torch.no_grad():
            conv.basic_conv.W.copy_(W0)
        feats = feats0.clone().requires_grad_(True)
        del seen[:]
        L.BACKWARD_LOG = []
        y = sptk.conv_norm_act(conv, norm, zptk.SphericalPointCloudPose(xyz, feats, None, pose))[3].feats
        grads = torch.autograd.grad(y, [feats, conv.basic_conv.W, norm.weight, norm.bias], gy)
        logs[packed], L.BACKWARD_LOG = L.BACKWARD_LOG, None
        names[packed] = set(seen)
        out[packed] = (y.detach(),) + grads
    assert logs[True] == logs[False] and logs[True][0]['regime'] == 'dense rows' and logs[True][0].get('norm') == 'in the node', logs
    new = {'eap_so3_dense_product_packed_f32', 'eap_so3_dense_zbound_packed_f32', 'eap_gemm_f16x2_splitk_tail_f32', 'eap_gemm_bf16x3_reduce_tail_f32',
           'eap_rows_gather_packed_f32', 'eap_rows_scatter_packed_f32'}
    assert new <= names[True] and not (new & names[False]), (names[True] & new, names[False] & new)
    assert 'eap_so3_dense_zbound_f32' in names[False] and 'eap_so3_dense_zbound_f32' not in names[True]
    a, u = out[True], out[False]
    assert torch.equal(a[0], u[0]) and torch.equal(a[1], u[1]) and torch.equal(a[3], u[3]) and torch.equal(a[4], u[4])
    e_w = float((a[2] - u[2]).abs().max() / u[2].abs().max())
    print(f'dW packed against zero-filled: {e_w:.2e}')
    assert bool(torch.isfinite(a[2]).all()) and e_w <= 5e-5, e_w
