"""GPU: every dispatch regime of vgtk.cuda.zpconv -- matrix-core forward (csrc/zpconv_mfma.hip), rows kernel (csrc/zpconv_rows.hip), scalar
kernels (csrc/zpconv.hip), on-chip backward (csrc/zpconv_bwd_hot.hip), product pipeline (csrc/zpconv_bwd.hip), atomic scatter, intra --
placed at the edges of its shape range by the case table of tests/zpconv_common.py.  Every case asserts WHICH regime served it (the name the
entry reports through eap_last_kernel, the on-chip entry's status vector, the verdict vgtk.cuda.zpconv remembers) and compares in two
modes: exact (small-integer operands: bit-equal to the int64 reference) and float (every element within 2 T u sum|products| of the float64
reference).  tests/test_zpconv_common_host.py shows on the CPU that both modes reject one wrong term on every case here.  Each case prints
`ZPCONV <regime> <case> <mode> <figure>`; profiles/zpconv_regimes.txt holds the worst ratios measured."""
import numpy as np
import pytest
import torch

import zpconv_common as ZC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _no_verdict_leaks():
    import vgtk.cuda.zpconv as Z
    Z._HOT_VERDICTS.clear()
    del Z._HOT_PENDING[:]
    yield
    Z._check_pending_verdicts(block=True)
    Z._HOT_VERDICTS.clear()


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _last_kernel():
    from vgtk import _hip
    return _hip.abi.eap_last_kernel().decode()


def _run(case, d_idx, d_w, d_x):
    """the Python entry -> (result, regime name)"""
    import vgtk.cuda.zpconv as Z
    _last_kernel()                                                         # (clear)
    if case.kind == 'fwd':
        out = Z.inter_zpconv_forward(d_idx, d_w, d_x)
    else:
        out = Z.inter_zpconv_backward(d_idx, d_w, d_x, case.dims[2])
    return out, _last_kernel()


def _report(regime, case, mode, figure):
    print(f'ZPCONV {regime} {case} {mode} {figure:.4g}')


def _hot_workspace_bytes(b, np_, nq, na, c, S, rcap):
    """HotWorkspace of csrc/zpconv_bwd_hot.hip, restated: the partial buffer is the only chunk that depends on the point ranges S"""
    r = lambda n: (n + 255) // 256 * 256
    fl, ent, rq = 4 * 64 * ((b + 63) // 64), 4 * b * np_ * 64, 4 * b * nq
    partial = 4 * b * S * (na // 4) * (c // 32) * rcap * 4 * 32 if S > 1 else 0
    return 2 * r(fl) + 2 * r(ent) + 2 * r(rq) + r(partial)


@pytest.mark.parametrize('case', ZC.CASES, ids=repr)
def test_inter_regime(dev, case, monkeypatch):
    import vgtk.cuda.zpconv as Z
    from vgtk import _hip
    b, np_, nq, na, ks, nn, c = case.dims
    monkeypatch.setattr(Z, 'ON_CHIP_BACKWARD', case.on_chip)
    for mode in ZC.modes_of(case):
        Z._HOT_VERDICTS.clear()
        d_idx, d_w, d_x = _dev(dev, *ZC.operands(case, mode))
        if case.raises:
            with pytest.raises(RuntimeError, match=case.raises):
                _run(case, d_idx, d_w, d_x)
            continue
        calls, whole = [], None
        if case.workspace:
            whole, name = _run(case, d_idx, d_w, d_x)                      # every cloud in one call
            assert name == ZC.PRODUCTS
            per_cloud = int(_hip.abi.eap_inter_zpconv_bwd_workspace(1, np_, nq, na, nn, c))
            monkeypatch.setattr(Z, 'BWD_WORKSPACE_BYTES', 2 * per_cloud if case.workspace == 'slices' else per_cloud - 1)
        entry = _hip.call                                                  # which entries the call goes through, with their batch sizes
        monkeypatch.setattr(_hip, 'call', lambda name, ref, *args, **kw: (calls.append((name, args[0])), entry(name, ref, *args, **kw))[1])
        out, name = _run(case, d_idx, d_w, d_x)
        monkeypatch.setattr(_hip, 'call', entry)
        if case.workspace:
            monkeypatch.setattr(Z, 'BWD_WORKSPACE_BYTES', 8 << 30)
            if case.workspace == 'slices':
                assert calls == [('eap_inter_zpconv_bwd_ws_f32', 2), ('eap_inter_zpconv_bwd_ws_f32', 2), ('eap_inter_zpconv_bwd_ws_f32', 1)]
                assert torch.equal(out, whole)                             # bit-equal to the unsliced call, in both modes
            else:
                assert calls == [('eap_inter_zpconv_bwd_f32', b)]
        if case.status is not None:                                        # the clouds the on-chip kernel left, as runs of consecutive clouds
            runs = [len(r) for r in ''.join('x' if s_ else ' ' for s_ in case.status).split()]
            assert calls == [('eap_inter_zpconv_bwd_hot_f32', b)] + [('eap_inter_zpconv_bwd_ws_f32', n) for n in runs]
        assert tuple(out.shape) == ((b, c, ks, np_, na) if case.kind == 'fwd' else (b, c, nq, na))
        if b == 0:
            continue
        assert name == case.expect, (mode, name)
        if case.status is not None:
            left = tuple(i for i, s in enumerate(case.status) if s)
            assert [v[1] for v in Z._HOT_VERDICTS.values()] == [left]
            rcap = int(_hip.abi.eap_inter_zpconv_bwd_hot_rows())
            assert rcap == ZC.HOT_RCAP
            assert int(_hip.abi.eap_inter_zpconv_bwd_hot_workspace(b, np_, nq, na, ks, nn, c)) == _hot_workspace_bytes(b, np_, nq, na, c, case.S, rcap)
        elif case.kind == 'bwd' and case.width == 'f32':
            assert not Z._HOT_VERDICTS                                     # the on-chip entry was not asked
        ok, figure = ZC.check(out.cpu().numpy(), case.name, mode)
        _report(name, case.name, mode, figure)
        assert ok, (mode, figure)
        if case.status is not None:
            again, name = _run(case, d_idx, d_w, d_x)                      # the remembered verdict: no host read, re-checked at teardown
            assert name == case.expect and torch.equal(again, out)
            Z._check_pending_verdicts(block=True)


@pytest.mark.parametrize('case', [c for c in ZC.CASES if c.kind == 'bwd' and c.dims[4:6] == (24, 64) and c.on_chip], ids=repr)
def test_on_chip_entry_at_the_abi(dev, case):
    """eap_inter_zpconv_bwd_hot_f32 itself: the status vector per cloud, and the clouds it reports done complete in an output pre-filled with
    NaN -- a support row nobody references comes back as an exact zero"""
    from vgtk import _hip
    b, np_, nq, na, ks, nn, c = case.dims
    nbytes = int(_hip.abi.eap_inter_zpconv_bwd_hot_workspace(b, np_, nq, na, ks, nn, c))
    if case.status is None:
        assert nbytes == 0 and nq > 16384                                  # past the row bitmap: the shape is not taken
        return
    for mode in ZC.MODES:
        idx, w, g = ZC.operands(case, mode)
        d_idx, d_w, d_g = _dev(dev, idx, w, g)
        out = torch.full((b, c, nq, na), float('nan'), dtype=torch.float32, device=dev)
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        status = torch.full((b,), -1, dtype=torch.int32, device=dev)
        _last_kernel()
        _hip.call('eap_inter_zpconv_bwd_hot_f32', out, b, np_, nq, na, ks, nn, c, d_idx, d_w, d_g, out, ws, status)
        assert _last_kernel() == ZC.HOT
        assert status.tolist() == case.status, mode
        done = [i for i, s in enumerate(case.status) if s == 0]
        got = out.cpu().numpy()[done]
        T = ZC.inter_backward_T(idx, nq)
        if mode == 'exact':
            ref = ZC.reference(case.name, mode)[0][done]
            assert ZC.exact_equal(got, ref), int((got != ref).sum())
            figure = 0
        else:
            if case.float_ok:
                ref, _, A = (t[done] for t in ZC.reference(case.name, mode))
            else:                                                          # (the clouds it leaves exceed the k u cap; the ones it takes do not)
                ref, A = ZC.inter_backward(idx[done], w[done], g[done], nq), ZC.inter_backward(idx[done], w[done], g[done], nq, absolute=True)
                assert 2.0 * T[done].max() * ZC.U['f32'] <= ZC.KU_CAP
            figure = ZC.worst_ratio(got, ref, ZC.float_bound(T[done], A))
            assert figure <= 1.0, figure
        unreferenced = np.broadcast_to(T[done] == 0, got.shape)
        assert (unreferenced.any() or not done) and (got[unreferenced] == 0).all()
        _report(ZC.HOT + '(abi)', case.name, mode, figure)


def _four_bytes_in(t):
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = store[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize('on_chip', [True, False])
@pytest.mark.parametrize('which', ['idx', 'w', 'x'])
@pytest.mark.parametrize('kind', ['fwd', 'bwd'])
def test_operands_four_bytes_into_their_storage(dev, kind, which, on_chip, monkeypatch):
    """idx, w, feats / grad, one at a time, as contiguous views with data_ptr() % 16 == 4.  A kernel that moves 16-byte words is selected only
    when every operand it moves that way is aligned: the forward falls to the scalar kernel for each of the three; the backward to the
    scatter kernel for idx and grad, while w -- read 4 bytes per lane by the on-chip kernel and by the product pipeline -- keeps its regime."""
    import vgtk.cuda.zpconv as Z
    if kind == 'fwd' and not on_chip:
        return                                                             # (the switch concerns the backward only)
    monkeypatch.setattr(Z, 'ON_CHIP_BACKWARD', on_chip)
    case = ZC.MISALIGNED_FWD if kind == 'fwd' else ZC.MISALIGNED_BWD
    aligned_regime = case.expect if on_chip else ZC.PRODUCTS
    expect = ZC.SCALAR if kind == 'fwd' else (aligned_regime if which == 'w' else ZC.SCATTER)
    for mode in ZC.MODES:
        Z._HOT_VERDICTS.clear()
        d = dict(zip(('idx', 'w', 'x'), _dev(dev, *ZC.operands(case, mode))))
        _, name = _run(case, d['idx'], d['w'], d['x'])
        assert name == aligned_regime                                       # the aligned call: the regime the misaligned one must leave
        d[which] = _four_bytes_in(d[which])
        out, name = _run(case, d['idx'], d['w'], d['x'])
        assert name == expect, (mode, name)
        ok, figure = ZC.check(out.cpu().numpy(), case.name, mode)
        _report(name + f'(misaligned {which})', case.name, mode, figure)
        assert ok, (mode, figure)


@pytest.mark.parametrize('shape', ZC.INTRA_CASES, ids=str)
def test_intra(dev, shape):
    import vgtk.cuda.zpconv as Z
    b, c, np_, a_in, a_out, ks, nn = shape
    for width in ('f32', 'f64'):
        for mode in ZC.MODES:
            idx, w, feats, grad = ZC.intra_operands(shape, mode, width)
            d_idx, d_w, d_f, d_g = _dev(dev, idx, w, feats, grad)
            refs = ZC.intra_reference(shape, mode, width)
            for direction in ('fwd', 'bwd'):
                _last_kernel()
                got = Z.intra_zpconv_forward(d_idx, d_w, d_f) if direction == 'fwd' else Z.intra_zpconv_backward(d_idx, d_w, d_g, a_in)
                assert _last_kernel() == ZC.INTRA
                ref, T, A = refs[direction]
                if mode == 'exact':
                    assert ZC.exact_equal(got.cpu().numpy(), ref), (width, direction)
                else:
                    figure = ZC.worst_ratio(got.cpu().numpy(), ref, ZC.float_bound(T, A, width))
                    _report(ZC.INTRA, f'{direction}_{width}_{shape}'.replace(' ', ''), mode, figure)
                    assert figure <= 1.0, (width, direction, figure)
