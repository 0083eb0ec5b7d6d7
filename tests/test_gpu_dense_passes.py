"""GPU: the two memory passes around the dense product (csrc/so3_dense.hip), through the C ABI.

The re-ordering pass Yt [b,na,o,p] -> Y [b,o,p,na] (dense_untranspose_tile_kernel; the two forms that return partial moments run
dense_untranspose_kernel) only moves numbers, so its outputs are compared BIT FOR BIT; its BatchNorm + activation form against
leaky(fma(y, scale, shift)) with the multiply-add formed in float64 and rounded to float32 -- two roundings where the kernel's fmaf
has one -- so at most 1 ulp apart.  Tiles are 128 columns (64 for the moment forms): p = 64 and 96 are one ragged tile, 160 two with a
ragged last one, 70 (not a multiple of 4) takes the dword loads; the channel counts are no multiple of anything.

The split (dense_split_kernel<BN>) writes the product's stored operand as two fp16 planes in fragment order: (h + l) / scale must
give the operand back to 2^-21 of the row's bound (the bar of tests/test_gpu_dense.py test_split_planes_reconstruct_the_operand),
columns that do not exist must be exact zeros in both planes, and -- the order of the pieces inside a 1 KB run -- the planes
contracted by the product kernel must give the float64 product at the forward product's bar."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOPE = 0.25


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _ordered(x):
    """float32 -> int64 that orders like the floats (adjacent floats differ by 1, -0 = +0)"""
    i = x.contiguous().view(torch.int32).long()
    return torch.where(i < 0, -(i & 0x7fffffff), i)


def _a_map(dev, gen, b, p, p_dst):
    """column -> point: distinct points of range(p_dst), about one column in eight dropped (-1)"""
    m = torch.stack([torch.randperm(p_dst, device=dev, generator=gen)[:p] for _ in range(b)]).int()
    drop = torch.rand(b, p, device=dev, generator=gen) < 0.125
    drop[:, 0] = False                                  # (column 0 stays: the pivot of the moment form)
    m[drop] = -1
    return m.contiguous()


def _scatter_reference(yt, m, p_dst, sentinel):
    """what the mapped forms must leave: row m[b, pp] of cloud b = column pp, every other row the sentinel"""
    b, na, o, p = yt.shape
    ref = torch.full((b, o, p_dst, na), sentinel, device=yt.device)
    src = yt.permute(0, 2, 3, 1)
    for i in range(b):
        keep = m[i] >= 0
        ref[i][:, m[i][keep].long()] = src[i][:, keep]
    return ref


@pytest.mark.parametrize('p', [64, 96, 160, 70])
@pytest.mark.parametrize('na', [60, 20, 4])
def test_reordering_moves_every_number_to_its_place(dev, na, p):
    from vgtk import _hip
    from vgtk._hip import _ptr, _F32
    b, gen = 2, _gen(dev, 100 * na + p)
    for o in (1, 3, 5, 8):
        yt = torch.randn(b, na, o, p, device=dev, generator=gen)
        want = yt.permute(0, 2, 3, 1).contiguous()
        y = torch.full((b, o, p, na), 7.5, device=dev)
        _hip.call('eap_so3_dense_untranspose_f32', yt, b, o, p, na, _ptr(yt), _ptr(y), _ptr(None), _ptr(None))
        assert torch.equal(y, want), (o, 'plain')
        # through a map into a wider Y: rows no column names keep what was there
        p_dst = p + 16
        m = _a_map(dev, gen, b, p, p_dst)
        want_m = _scatter_reference(yt, m, p_dst, -3.25)
        ym = torch.full((b, o, p_dst, na), -3.25, device=dev)
        _hip.call('eap_so3_dense_untranspose_map_f32', yt, b, o, p, na, p_dst, _ptr(m), _ptr(yt), _ptr(ym))
        assert torch.equal(ym, want_m), (o, 'mapped')
        assert int((want_m[:, 0, :, 0] == -3.25).sum()) >= b * 16           # (not vacuous: untouched rows exist)
        # BatchNorm + leaky_relu on the way out, without and with the map
        sc = (torch.rand(o, device=dev, generator=gen) + 0.5) * torch.where(torch.rand(o, device=dev, generator=gen) < 0.3, -1.0, 1.0)
        sh = 0.3 * torch.randn(o, device=dev, generator=gen)                  # (small against y: both branches of the activation occur)
        u = (yt.double() * sc.double()[None, None, :, None] + sh.double()[None, None, :, None]).float()      # fma in float64, rounded
        act = torch.where(u > 0, u, (u.double() * SLOPE).float())            # (the product of two float32 in float64, rounded: float32's own multiply)
        assert bool((act > 0).any()) and bool((act < 0).any())
        yb = torch.full((b, o, p, na), 7.5, device=dev)
        _hip.call('eap_so3_dense_untranspose_bnact_f32', yt, b, o, p, na, p, _ptr(None), _ptr(yt), _ptr(sc), _ptr(sh), _F32(SLOPE), _ptr(yb))
        ulps = int((_ordered(yb) - _ordered(act.permute(0, 2, 3, 1))).abs().max())
        print(f'na={na} p={p} o={o}: BatchNorm form, largest difference {ulps} ulp')
        assert ulps <= 1, (o, ulps)
        ybm = torch.full((b, o, p_dst, na), -3.25, device=dev)
        _hip.call('eap_so3_dense_untranspose_bnact_f32', yt, b, o, p, na, p_dst, _ptr(m), _ptr(yt), _ptr(sc), _ptr(sh), _F32(SLOPE), _ptr(ybm))
        want_bm = _scatter_reference(act, m, p_dst, -3.25)
        written = _scatter_reference(torch.ones_like(yt), m, p_dst, 0.0) > 0
        assert torch.equal(ybm[~written], want_bm[~written])
        assert int((_ordered(ybm) - _ordered(want_bm)).abs().max()) <= 1, o
        assert torch.equal(ybm[written], _scatter_reference(yb.permute(0, 3, 1, 2).contiguous(), m, p_dst, -3.25)[written])     # the same numbers as unmapped


@pytest.mark.parametrize('p', [64, 96, 160, 70])
@pytest.mark.parametrize('na', [60, 20, 4])
def test_reordering_with_partial_moments(dev, na, p):
    """The moment-returning forms keep their interface: psum / psq [o][b * chunks + chunk] over chunks of 64 columns, of (y - pivot) and
    its square with pivot = Y[0][o][0][0], padding columns of a map left out.  Each partial against the float64 sum over its chunk
    (float32 summation of <= 64 na terms: 1e-5 of the chunk's sum of magnitudes is generous), and the float64 sums of the partials within
    1e-6 relative of torch's -- relative to the sum of |y - pivot| for the first moment, whose terms cancel."""
    from vgtk import _hip
    from vgtk._hip import _ptr
    b, gen = 2, _gen(dev, 7 + 100 * na + p)
    chunks = (p + 63) // 64
    for o in (1, 3, 5, 8):
        yt = torch.randn(b, na, o, p, device=dev, generator=gen) + 0.5
        m = _a_map(dev, gen, b, p, p + 16)
        pivot_pos = torch.zeros(1, dtype=torch.int32, device=dev)            # column 0 of cloud 0 is the pivot's
        for mapped in (False, True):
            p_dst = p + 16 if mapped else p
            y = torch.full((b, o, p_dst, na), -3.25, device=dev)
            ps = torch.full((o, b * chunks), float('nan'), device=dev)
            pq = torch.full((o, b * chunks), float('nan'), device=dev)
            if mapped:
                _hip.call('eap_so3_dense_untranspose_map_stats_f32', yt, b, o, p, na, p_dst, _ptr(m), _ptr(pivot_pos), _ptr(yt), _ptr(y), _ptr(ps), _ptr(pq))
                assert torch.equal(y, _scatter_reference(yt, m, p_dst, -3.25))
                keep = (m >= 0).double()
            else:
                _hip.call('eap_so3_dense_untranspose_f32', yt, b, o, p, na, _ptr(yt), _ptr(y), _ptr(ps), _ptr(pq))
                assert torch.equal(y, yt.permute(0, 2, 3, 1))
                keep = torch.ones(b, p, dtype=torch.float64, device=dev)
            d = (yt.double() - yt[0, 0, :, 0].double()[None, None, :, None]) * keep[:, None, None, :]       # [b,na,o,p]
            pad = chunks * 64 - p
            d = torch.nn.functional.pad(d, (0, pad)).view(b, na, o, chunks, 64)
            s1 = d.sum((1, 4)).permute(1, 0, 2).reshape(o, b * chunks)       # [o][b chunks + chunk]
            s2 = (d * d).sum((1, 4)).permute(1, 0, 2).reshape(o, b * chunks)
            sa = d.abs().sum((1, 4)).permute(1, 0, 2).reshape(o, b * chunks)
            assert float(((ps.double() - s1).abs() / sa.clamp(min=1e-30)).max()) < 1e-5, (o, mapped)
            assert float(((pq.double() - s2).abs() / s2.clamp(min=1e-30)).max()) < 1e-5, (o, mapped)
            e1 = float(((ps.double().sum(1) - s1.sum(1)).abs() / sa.sum(1)).max())
            e2 = float(((pq.double().sum(1) - s2.sum(1)).abs() / s2.sum(1)).max())
            print(f'na={na} p={p} o={o} mapped={mapped}: moments off by {e1:.2e}, {e2:.2e}')
            assert e1 < 1e-6 and e2 < 1e-6, (o, mapped, e1, e2)


def _planes_to_rows(planes, scale, b, m, l, na):
    """planes [b,a,kb,mt,plane,lane,8 halves] -> (h + l) [b,a,row,k] with k = 16 kb + 8 (lane >> 5) + e, row = 32 mt + (lane & 31); and
    the two planes' largest magnitude per (b, a, row, k)"""
    lp = (l + 31) // 32 * 32
    pl = planes.view(torch.float16).view(b, na, lp // 16, m // 32, 2, 2, 32, 8).double()      # [b,a,kb,mt,plane,kg,i,e]
    rows = pl.permute(0, 1, 4, 3, 6, 2, 5, 7).reshape(b, na, 2, m, lp)                         # [b,a,plane,row,k]
    return rows[:, :, 0] + rows[:, :, 1], rows.abs().amax(2)


def _dyadic(gen, dev, shape, bits=6, span=4.0):
    """random multiples of 2^-bits in (-span, span): sums and products of a few of them are exact in float32"""
    return torch.round(torch.randn(shape, device=dev, generator=gen).clamp(-span + 0.1, span - 0.1) * 2 ** bits) / 2 ** bits


@pytest.mark.parametrize('l', [8, 40, 48])
@pytest.mark.parametrize('na', [60, 20])
@pytest.mark.parametrize('m', [32, 64])
def test_split_behind_a_batchnorm(dev, m, na, l):
    """eap_so3_dense_split_bn_f32: gx = k1 g - k2 - k3 xhat formed from (dL/dy', y') on the way into the planes.  l = 8 and 40 of the 48
    source columns through a column map with -1 entries (40: the last k-block of 32 is half empty), l = 48 without a map.  gamma = 1 / ig
    with ig a power of two and dyadic inputs: the float32 evaluation is exact, what is left is the split's own error."""
    from vgtk import _hip
    from vgtk._hip import _ptr, _F32
    b, l_src, gen = 2, 48, _gen(dev, m + na + l)
    grad = _dyadic(gen, dev, (b, m, l_src, na))
    act = _dyadic(gen, dev, (b, m, l_src, na))
    act[act == 0] = 0.5
    colmap = None
    if l != l_src:
        colmap = torch.stack([torch.randperm(l_src, device=dev, generator=gen)[:l] for _ in range(b)]).int()
        colmap[:, 2::5] = -1
        colmap = colmap.contiguous()
    # a positive and a negative activation in every row: the first two columns the operand takes
    first = colmap[:, :2].long() if colmap is not None else torch.tensor([[0, 1]] * b, device=dev)
    for i in range(b):
        act[i, :, first[i, 0]] = act[i, :, first[i, 0]].abs()
        act[i, :, first[i, 1]] = -act[i, :, first[i, 1]].abs()
    ig = 2.0 ** torch.randint(-1, 3, (m,), device=dev, generator=gen).float()                  # 1 / gamma exact (gamma = 2, 1, 1/2, 1/4)
    k1 = 2.0 ** torch.randint(-1, 2, (m,), device=dev, generator=gen).float()
    k2, k3, be = _dyadic(gen, dev, (m,), 4, 1.0), _dyadic(gen, dev, (m,), 4, 1.0), _dyadic(gen, dev, (m,), 4, 2.0)
    coef = torch.stack([k1, k2, k3, be, ig]).contiguous()
    c = lambda v: v.double()[None, :, None, None]
    pos = act > 0
    gg = torch.where(pos, grad.double(), grad.double() * SLOPE)
    pre = torch.where(pos, act.double(), act.double() / SLOPE)
    gx = gg * c(k1) - c(k2) - (pre - c(be)) * c(ig) * c(k3)                                     # [b,m,l_src,na] float64
    assert torch.equal(gx.float().double(), gx)                                                # (exact in float32, as promised)
    if colmap is not None:
        take = colmap.clamp(min=0).long()
        gx = torch.stack([gx[i][:, take[i]] for i in range(b)]) * (colmap >= 0).double()[:, None, :, None]
    assert bool((pos.flatten(2).any(2) & (~pos).flatten(2).any(2)).all())
    bound = (gx.abs().amax(2) * 1.5).float().clamp(min=2.0 ** -20)                              # [b,m,na] >= max |gx| of the row
    scale = torch.empty(2, b, na, m, device=dev)
    lp = (l + 31) // 32 * 32
    planes = torch.full((b * na * m * lp,), 0x3c003c00, dtype=torch.int32, device=dev)          # (fp16 ones: nothing may stay)
    _hip.call('eap_so3_dense_split_bn_f32', grad, b, m, l, l_src, na, _ptr(bound.view(torch.int32)), _ptr(colmap), _ptr(grad), _ptr(act), _ptr(coef),
              _F32(SLOPE), _ptr(scale), _ptr(planes))
    assert torch.equal(scale[1].view(b, m, na), scale[0].permute(0, 2, 1))
    top = bound.permute(0, 2, 1) * scale[0]
    assert float(top.min()) >= 2.0 ** 14 and float(top.max()) < 2.0 ** 15                      # the row's bound lands in [2^14, 2^15)
    v, mag = _planes_to_rows(planes, scale, b, m, l, na)                                       # [b,a,row,k]
    rec = (v / scale[0].double()[:, :, :, None])[:, :, :, :l].permute(0, 2, 3, 1)              # [b,row,k,a]
    err = float(((rec - gx).abs() / bound.double()[:, :, None, :]).max())
    print(f'm={m} na={na} l={l}: reconstruction error {err * 2 ** 21:.3f} x 2^-21 of the row bound')
    assert err < 2.0 ** -21
    absent = torch.zeros(b, lp, dtype=torch.bool, device=dev)
    absent[:, l:] = True
    if colmap is not None:
        absent[:, :l] = colmap < 0
    assert int(absent.sum()) > 0 and float((mag * absent[:, None, None, :]).max()) == 0.0     # exact zeros in both planes


def _check_plain_split(x_rows, scale, planes, b, m, l, na, written=None):
    """x_rows float64 [b,row,k,a]: the operand the planes must hold; written bool [b,k] (None: everything up to l)"""
    assert torch.equal(scale[1].view(b, m, na), scale[0].permute(0, 2, 1))
    v, _ = _planes_to_rows(planes, scale, b, m, l, na)
    rec = (v / scale[0].double()[:, :, :, None])[:, :, :, :l].permute(0, 2, 3, 1)
    rowmax = x_rows.abs().amax(2, keepdim=True).clamp(min=1e-30)
    e = (rec - x_rows).abs() / rowmax
    if written is not None:
        e = e * written[:, None, :, None]
    return float(e.max())


@pytest.mark.parametrize('na', [60, 20])
@pytest.mark.parametrize('m', [32, 64])
def test_plain_split_of_three_sources(dev, m, na):
    """eap_so3_dense_split_f32 on a plain source, a column-mapped one and a dense-index one (mapped = 1 with n_rows: element d of a row is
    the (kernel point k, row slot r) pair with dense index d = (r / 16) 16 ks + 16 k + r % 16, read at segment k, position r of a padded
    pitch; k-blocks past the cloud's own rows are not written)."""
    from vgtk import _hip
    b, gen = 2, _gen(dev, 31 * m + na)
    x = torch.randn(b, m, 48, na, device=dev, generator=gen) * torch.exp(3 * torch.randn(b, m, 1, na, device=dev, generator=gen))
    scale, planes = _hip.so3_dense_split(x)
    e = _check_plain_split(x.double(), scale, planes, b, m, 48, na)
    _, mag = _planes_to_rows(planes, scale, b, m, 48, na)
    assert e < 2.0 ** -21 and float(mag[..., 48:].max()) == 0.0, e
    # columns through a map (40 of 48, some absent)
    colmap = torch.stack([torch.randperm(48, device=dev, generator=gen)[:40] for _ in range(b)]).int()
    colmap[:, 3::7] = -1
    colmap = colmap.contiguous()
    scale, planes = _hip.so3_dense_split(x, colmap=colmap)
    xm = torch.stack([x[i][:, colmap[i].clamp(min=0).long()] for i in range(b)]).double() * (colmap >= 0).double()[:, None, :, None]
    e = _check_plain_split(xm, scale, planes, b, m, 40, na)
    _, mag = _planes_to_rows(planes, scale, b, m, 40, na)
    absent = torch.ones(b, 64, dtype=torch.bool, device=dev)
    absent[:, :40] = colmap < 0
    assert e < 2.0 ** -21 and float((mag * absent[:, None, None, :]).max()) == 0.0, e
    # dense index: ks = 4 kernel points, rp = 32 row slots, rows [o][k][pitch]; cloud 0 has 10 rows (one group of 16), cloud 1 all 32
    ks, rp, pitch = 4, 32, 32 * na + 24
    g = torch.full((b, m, ks, pitch), float('nan'), device=dev)
    g[..., :rp * na] = torch.randn(b, m, ks, rp * na, device=dev, generator=gen)
    n_rows = torch.tensor([10, 32], dtype=torch.int32, device=dev)
    scale, planes = _hip.so3_dense_split(g, seg=rp, seg_pitch=pitch, shape=(b, m, ks * rp, na), mapped=True, n_rows=n_rows)
    d = torch.arange(ks * rp, device=dev)
    grp, rem = d // (16 * ks), d % (16 * ks)
    k_of, r_of = rem // 16, 16 * grp + rem % 16
    gd = g[..., :rp * na].view(b, m, ks, rp, na)[:, :, k_of, r_of].double()                      # [b,row,d,a]
    written = torch.stack([d < ((int(n) + 15) // 16 * 16) * ks for n in n_rows.tolist()])
    # (the row maximum runs over the whole source row, written or not)
    v, _ = _planes_to_rows(planes, scale, b, m, ks * rp, na)
    rec = (v / scale[0].double()[:, :, :, None]).permute(0, 2, 3, 1)
    rowmax = gd.abs().amax(2, keepdim=True)
    e = torch.where(written[:, None, :, None], (rec - gd).abs() / rowmax, torch.zeros_like(rec))
    assert float(e.max()) < 2.0 ** -21, float(e.max())                                         # (a NaN in a written place fails too)
    assert int(written.sum()) == 64 + 128


def test_fragment_order_under_the_product(dev):
    """The planes as the product kernel reads them: dY -> planes (plain, column-mapped through the geometry's point order, and behind
    a BatchNorm with identity coefficients) -> eap_so3_dense_product_f32 (backward direction) against the float64 sum at the bar of
    tests/test_gpu_dense.py: a 16-byte piece in the wrong place of its 1 KB run is another row's or another k half's numbers."""
    import test_gpu_dense as D
    from vgtk import _hip
    from vgtk._hip import _ptr, _I64, _F32
    P, B, o = 288, 2, 128
    s = D._setup(dev, B, P, layer=2)
    head, geo, rp = D._geometry(s, dev)
    wd = D._dense_weights64(s, head.rows, rp)                                                  # [B,P,rp,A,K]
    gen = _gen(dev, 5)
    gy = torch.randn(B, o, P, D.NA, device=dev, generator=gen) * torch.exp(2 * torch.randn(B, o, 1, D.NA, device=dev, generator=gen))
    ref = torch.einsum('bopa,bprak->bokar', gy.double(), wd)
    mag = torch.einsum('bopa,bprak->bokar', gy.double().abs(), wd)
    magm = torch.einsum('bopa,bpr->boar', gy.double().abs(), D._member(s, head.rows, rp))[:, :, None]
    cols = geo.columns()
    l = P if cols is None else cols.shape[1]

    def product(scale, planes):
        z = torch.empty(B, o, D.KS, D.NA * rp, device=dev)
        _hip.call('eap_so3_dense_product_f32', gy, 0, B, o, l, D.NA, D.KS, rp, _I64(D.NA * rp), _F32(geo.sigma), _ptr(geo.n_rows), _ptr(planes), _ptr(scale),
                  _ptr(geo.pt), _ptr(geo.kr), _ptr(geo.mask(0)), _ptr(z))
        return z.view(B, o, D.KS, D.NA, rp)

    z = product(*_hip.so3_dense_split(gy, colmap=cols))
    assert float(((z.double() - ref).abs() / (1e-6 * mag + 5e-7 * magm).clamp(min=1e-30)).max()) < 1.0
    # the BatchNorm form with k1 = 1, k2 = k3 = 0 and a positive activation everywhere hands the same gradient through
    coef = torch.stack([torch.ones(o, device=dev), torch.zeros(o, device=dev), torch.zeros(o, device=dev), torch.zeros(o, device=dev),
                        torch.ones(o, device=dev)]).contiguous()
    act = torch.rand(B, o, P, D.NA, device=dev, generator=gen) + 0.5
    bound = gy.abs().amax(2).contiguous()
    scale = torch.empty(2, B, D.NA, o, device=dev)
    planes = torch.empty(B * D.NA * o * ((l + 31) // 32 * 32), dtype=torch.int32, device=dev)
    _hip.call('eap_so3_dense_split_bn_f32', gy, B, o, l, P, D.NA, _ptr(bound.view(torch.int32)), _ptr(cols), _ptr(gy), _ptr(act), _ptr(coef), _F32(SLOPE),
              _ptr(scale), _ptr(planes))
    z2 = product(scale, planes)
    assert float(((z2.double() - ref).abs() / (1e-6 * mag + 5e-7 * magm).clamp(min=1e-30)).max()) < 1.0
