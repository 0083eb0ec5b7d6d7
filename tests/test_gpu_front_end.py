"""GPU: the small launches in front of a layer's big kernels -- the ball query with a lane group per query point (csrc/grouping.hip),
the row list sorted over the referenced rows only (csrc/inv_lists.hip), the list head's words from one entry (csrc/list_probe.hip):
integer results, every comparison is for equality -- and the feature gradient's product over k-slabs (csrc/gemm_bf16x3.hip,
eap_gemm_f16x2_splitk_f32) against float64."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import front_end_common as FE  # noqa: E402

T = torch.from_numpy
SIZES = [1, 15, 16, 17, 63, 64, 65, 1000]
NSAMPLES = [1, 2, 63, 64, 65]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


# ---- ball query ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_ball_query_every_size_pair(dev, dtype):
    """n, m in {1, 15, 16, 17, 63, 64, 65, 1000}, m != n, nsample in {1, 2, 63, 64, 65}, a radius that leaves most lists short and one that
    fills them: bit-equal to the oracle."""
    import vgtk.cuda.grouping as G
    rng = np.random.default_rng(5)
    for n in SIZES:
        xyz = rng.random((2, 3, n)).astype(dtype)
        xyz_d = T(xyz).to(dev)
        for m in SIZES:
            if m == n:
                continue
            q = rng.random((2, 3, m)).astype(dtype)
            q_d = T(q).to(dev)
            for ns in NSAMPLES:
                for radius in (0.25, 0.7):
                    ref = FE.native.ball_query(q, xyz, radius, ns)
                    got = G.ball_query(q_d, xyz_d, radius, ns).cpu().numpy()
                    assert np.array_equal(got, ref), (n, m, ns, radius)


def _line(n, h, skip, dtype):
    """support point k at x = k (the first `skip` far away), queries at x = skip - 0.5 and one with an empty ball: with radius h the
    hits are skip .. skip + h - 1 (as far as the cloud goes)"""
    xyz = np.zeros((1, 3, n), dtype)
    xyz[0, 0] = np.arange(n)
    xyz[0, 0, :skip] = -1.0e4 - np.arange(skip)
    q = np.zeros((1, 3, 4), dtype)
    q[0, 0] = [skip - 0.5, skip - 0.5, -3.0e4, skip - 0.5]
    return q, xyz


def _by_hand(hits, ns):
    row = np.zeros(ns, np.int32)
    cnt = min(len(hits), ns)
    row[:cnt] = hits[:cnt]
    if 0 < cnt < ns - 1:
        for t in range(cnt, ns):
            row[t] = row[t - cnt]
    return row


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_ball_query_hit_counts_at_the_padding_rules(dev, dtype):
    """0, nsample - 1, nsample and nsample + 1 hits; the last hit the cloud's last point; lists that fill exactly at the end of a group of
    16 candidates (hits 16 .. 31 with nsample 16, 0 .. 63 with nsample 64); operands one element (4 bytes in float32) into their storage:
    bit-equal to the oracle and to the answer written out by hand."""
    import vgtk.cuda.grouping as G
    for ns in NSAMPLES + [16, 32]:
        for h in sorted({0, ns - 1, ns, ns + 1}):
            for skip in (0, 7, 16):
                for n in sorted({max(skip + h, 1), skip + h + 40}):
                    q, xyz = _line(n, h, skip, dtype)
                    ref = FE.native.ball_query(q, xyz, float(h), ns)
                    hits = list(range(skip, min(skip + h, n)))
                    want = np.stack([_by_hand(hits, ns), _by_hand(hits, ns), np.zeros(ns, np.int32), _by_hand(hits, ns)])
                    assert np.array_equal(ref[0], want), (ns, h, skip, n)
                    for shift in (False, True):
                        q_d, xyz_d = T(q).to(dev), T(xyz).to(dev)
                        if shift:
                            q_d, xyz_d = FE.offset_copy(q_d), FE.offset_copy(xyz_d)
                            assert q_d.data_ptr() % 16 != 0 or xyz_d.data_ptr() % 16 != 0
                        got = G.ball_query(q_d, xyz_d, float(h), ns).cpu().numpy()
                        assert np.array_equal(got, ref), (ns, h, skip, n, shift)


# ---- row list -----------------------------------------------------------------------------------------------------------
def _check_rows(dev, idx, n):
    from vgtk import _hip
    want = FE.row_list(idx, n)
    got = _hip.inv_lists_rows(T(idx.astype(np.int32)).to(dev), n)
    for name, g, w in zip(('rows', 'off', 'cnt', 'n_rows'), got, want):
        assert np.array_equal(g.cpu().numpy(), w), (name, n)
    return want[3]


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000, 1024, 1025, 4096, 16384])
def test_row_list_sizes(dev, n):
    """some rows referenced (uneven counts), none (every index >= n or negative), equal counts throughout"""
    rng = np.random.default_rng(n)
    some = rng.permutation(n)[:n // 8 + 1]
    idx = some[rng.integers(0, some.size, (2, 64, 16))]
    idx[1, :5] = n + 3                                     # (entries outside the support are not counted)
    n_rows = _check_rows(dev, idx, n)
    assert 0 < n_rows.max() <= some.size
    assert (_check_rows(dev, np.stack([np.full((64, 16), n), np.full((64, 16), -1)]), n) == 0).all()
    rep = 1024 // min(n, 1024)
    equal = np.resize(np.repeat(rng.permutation(n)[:1024 // rep], rep), (1, 64, 16))
    assert (_check_rows(dev, equal, n) == min(n, 1024 // rep)).all()


@pytest.mark.parametrize('referenced', [2048, 2049, 4096])
def test_row_list_at_the_whole_range_threshold(dev, referenced):
    """2048 referenced rows sort compacted, 2049 and all 4096 over the whole range; one cloud with uneven and one with equal counts"""
    n = 4096
    rng = np.random.default_rng(referenced)
    rows = rng.permutation(n)[:referenced]
    uneven = np.concatenate([rows, rows[rng.integers(0, referenced, 3 * n - referenced)]])
    equal = np.resize(rows, 3 * n) if referenced != 2049 else np.concatenate([np.tile(rows, 5), np.full(3 * n - 5 * 2049, n)])
    n_rows = _check_rows(dev, np.stack([uneven, equal]).reshape(2, 3 * n // 32, 32), n)
    assert (n_rows == referenced).all()


# ---- the list head's words ----------------------------------------------------------------------------------------------
def _head_words(monkeypatch, native, *args, **kw):
    import vgtk.so3conv.functional as L
    from vgtk import _hip
    monkeypatch.setattr(_hip, 'NATIVE_LIST_PROBE', native)
    calls = []
    real = _hip.so3_dense_probe
    monkeypatch.setattr(_hip, 'so3_dense_probe', lambda *a: (calls.append(1), real(*a))[1])
    head = L._ListHead(*args, **kw)
    head.event.synchronize()
    assert len(calls) == (1 if native else 0)
    return head, head.host.tolist()


def _rot_z(a):
    return [[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]]


@pytest.mark.parametrize('p,radius', [(96, 0.3), (600, 0.12)])
def test_list_head_words_match_the_tensor_expressions(dev, monkeypatch, p, radius):
    """the entry against the tensor expressions it replaces and against the numpy restatement, word for word: 16-word (p = 96) and 32-word
    (p = 600) membership tables, p no multiple of 64, with and without norm, nonident, poses, one non-identity block, a per-cloud rotation
    with an orthonormality defect of 5e-7 (passes) and of 2e-6 (does not)"""
    import synth_clouds
    import vgtk.cuda.grouping as G
    b, nn = 2, 16
    xyz = T(synth_clouds.laptop_batch(3, b, p)[0]).to(dev)
    idx = G.ball_query(xyz, xyz, radius, nn)
    eye = torch.eye(4, device=dev).repeat(b, p, 1, 1)
    turned = eye.clone()
    turned[1, p - 1, :3, :3] = torch.tensor(_rot_z(0.3), device=dev)
    nan = eye.clone()
    nan[0, 0, 1, 1] = float('nan')

    def cloud_rot(defect):
        r = torch.eye(3, device=dev).repeat(b, 1, 1)
        r[1, 0, 1] = defect
        return r

    def norm(ill):
        w = torch.linspace(-1.0, 1.0, 37, device=dev)
        w[5] = 0.0
        bias = w * 100.0
        bias[5] = 7.0                                        # (gamma == 0: not counted)
        if ill:
            bias[36] = 128.5
        return types.SimpleNamespace(weight=torch.nn.Parameter(w), bias=torch.nn.Parameter(bias))

    nonident = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    cases = [dict(), dict(nonident=nonident), dict(dense_probe=(None, None)), dict(dense_probe=(eye, eye), norm=norm(False)),
             dict(dense_probe=(eye, turned), norm=norm(True)), dict(dense_probe=(turned, turned)), dict(dense_probe=(nan, None)),
             dict(dense_probe=()), dict(dense_probe=(('orthonormal', cloud_rot(5e-7)),)),
             dict(dense_probe=(('orthonormal', cloud_rot(2e-6)),), norm=norm(False), nonident=nonident)]
    for kw in cases:
        kw = dict(kw)
        ni = kw.pop('nonident', None)
        h0, w0 = _head_words(monkeypatch, False, idx, p, ni, **kw)
        h1, w1 = _head_words(monkeypatch, True, idx, p, ni, **kw)
        assert w1 == w0, (kw.keys(), w1, w0)
        probe = kw.get('dense_probe')
        if probe is not None:
            assert h1.memb.shape[2] == (32 if p > 512 else 16) and torch.equal(h1.memb, h0.memb)
        from vgtk import _hip
        memb = dflags = None
        if probe is not None:
            memb, dflags = _hip.so3_dense_member(idx, h1.rows, h1.n_rows, p)
        nm = kw.get('norm')
        want = FE.probe_words(p, h1.n_rows.cpu().numpy(), None if ni is None else ni.cpu().numpy(),
                              None if dflags is None else dflags.cpu().numpy(), None if memb is None else memb.cpu().numpy(),
                              [r.cpu().numpy() for r in (probe or ()) if r is not None and not isinstance(r, tuple)],
                              next((r[1].cpu().numpy() for r in (probe or ()) if isinstance(r, tuple)), None),
                              None if nm is None else nm.weight.detach().cpu().numpy(), None if nm is None else nm.bias.detach().cpu().numpy())
        assert w1 == want[:len(w1)].tolist(), (kw.keys(), w1, want)
        assert len(w1) == (5 if nm is not None else 4)


# ---- the feature gradient's product over k-slabs ---------------------------------------------------------------------------
def _slab_counts(K):
    """every count the launcher can choose: a divisor of the K / 16 k-tiles that leaves slabs of at least 16 (include/eap_hip.h)"""
    tiles = K // 16
    return [s for s in range(1, 65) if tiles % s == 0 and (s == 1 or tiles // s >= 16)]


def _launched(fn):
    from vgtk import _hip
    rec = []
    _hip.KERNEL_TIMES = rec
    try:
        fn()
    finally:
        _hip.KERNEL_TIMES = None
    return [n for n, *_ in rec]


@pytest.mark.parametrize('K', [16 * 64, 16 * 65 * 4])
def test_split_k_feature_gradient_product(dev, K):
    """M = 128 (and 64 rows zero-padded to 128), N = 256 and 260 columns in a pitch of 384, batch 1 and 3, every slab count: within
    2^-21 sum |a||b| of float64 per element (the two-plane bound of tests/test_gpu_split_planes.py), one slab bit-equal to
    eap_gemm_f16x2_f32, two runs of every count bit-equal, and _hip.matmul takes the entry with the launcher's count."""
    from vgtk import _hip
    M = 128
    assert _slab_counts(K) == ([1, 2, 4] if K == 1024 else [1, 2, 4, 5, 10, 13])
    gen = torch.Generator().manual_seed(K)
    worst = 0.0
    for rows in (64, 128):
        A = torch.randn(M, K, generator=gen) * 0.05
        A[rows:] = 0.0
        A = A.to(dev)
        abs_a = _hip.absmax_rows(A, 1, M, K, K, 0)
        for N, cols in ((256, 256), (384, 260)):
            for batch in (1, 3):
                B = torch.randn(batch, K, N, generator=gen).abs() * torch.exp(torch.randn(batch, 1, N, generator=gen) * 2.0)
                B[:, :, cols:] = 0.0
                B = B.to(dev)
                abs_b = _hip.absmax_colgroups(B, batch, K, N, N, K * N, 4)
                ref = torch.matmul(A.double().cpu(), B.double().cpu())
                bound = torch.matmul(A.abs().double().cpu(), B.abs().double().cpu())
                base = torch.full((batch, M, N), float('nan'), device=dev)
                _hip.call('eap_gemm_f16x2_f32', base, 0, M, N, K, A, K, B, N, K * N, base, N, M * N, batch, abs_a, abs_b, 4, 1.0, None, None, 0.0,
                          None, 0)
                for slabs in _slab_counts(K):
                    floats = int(_hip.abi.eap_gemm_f16x2_splitk_workspace(M, N, batch, slabs))
                    assert floats == (0 if slabs == 1 else slabs * batch * M * N)
                    runs = []
                    for _ in range(2):
                        C = torch.full((batch, M, N), float('nan'), device=dev)
                        work = torch.full((max(floats, 4),), float('nan'), device=dev)
                        _hip.call('eap_gemm_f16x2_splitk_f32', C, M, N, K, A, K, B, N, K * N, C, N, M * N, batch, abs_a, abs_b, 4, 1.0, slabs,
                                  work if floats else None, floats)
                        runs.append(C)
                    assert torch.equal(runs[0], runs[1]), (rows, N, batch, slabs)
                    if slabs == 1:
                        assert torch.equal(runs[0], base), (rows, N, batch)
                    err = (runs[0].double().cpu() - ref).abs()
                    ratio = (err / bound.clamp_min(1e-300)).max().item()
                    worst = max(worst, ratio)
                    assert (err <= 2.0 ** -21 * bound).all(), (rows, N, batch, slabs, ratio)
                    assert (runs[0][:, rows:] == 0).all() and (runs[0][:, :, cols:] == 0).all()
                # the route: the launcher's own count, the same bits as that count asked for by hand; switched off, the one-slab entry
                chosen = _hip.abi.eap_gemm_f16x2_splitk_slabs(M, N, K, batch, 0)
                assert chosen in _slab_counts(K) and chosen > 1
                out = torch.full((batch, M, N), float('nan'), device=dev)
                names = _launched(lambda: _hip.matmul(A, B, out, b_bound=(abs_b, 4, 1.0)))
                assert names[-1] == 'eap_gemm_f16x2_splitk_f32', names
                C = torch.empty_like(out)
                work = torch.empty(chosen * batch * M * N, device=dev)
                _hip.call('eap_gemm_f16x2_splitk_f32', C, M, N, K, A, K, B, N, K * N, C, N, M * N, batch, abs_a, abs_b, 4, 1.0, chosen, work, work.numel())
                assert torch.equal(out, C)
                was, _hip.SPLIT_K_ONE_ROW_TILE = _hip.SPLIT_K_ONE_ROW_TILE, False
                try:
                    names = _launched(lambda: _hip.matmul(A, B, out, b_bound=(abs_b, 4, 1.0)))
                finally:
                    _hip.SPLIT_K_ONE_ROW_TILE = was
                assert names[-1] == 'eap_gemm_f16x2_f32' and torch.equal(out, base), names
    print(f'\nK = {K}: largest error / sum |a||b| = {worst:.3e} (bar 2^-21 = {2.0 ** -21:.3e})')
