"""CPU: the view-based GEMM calls of vgtk/_hip.py (matmul, matmul_reduce, matmul_epilogue, matmul_reduce_takes_split) derive the
positional numbers of gemm / gemm_reduce / gemm_epilogue from the views' shapes and strides, check them, and forward.  The three
positional functions are replaced by recorders here (nothing is launched); tensors are CPU float32.

  * SITES: one row per call site of vgtk/so3conv/functional.py that states its product as views, the views built the way the site
    builds them, at toy sizes; the recorded call must equal the numbers the site stated by hand before, written out literally;
  * DERIVATIONS: the rules of `_hip.operand` against hand-written tuples (pitch, item stride, storage offset, transposition, a
    shared A, dimensions of size 1);
  * every refusal raises RuntimeError before the recorder sees a call.

The SITES rows restate the sites' view expressions: an edit to a site does not fail its row.  Where the function of functional.py runs on
host tensors (_contract_into, _weight_grad_from_z, _rows_grad_from_z) test_the_functions_of_the_operator_layer_make_these_calls calls it
against the same rows.  _backward_textbook and _group_contract are functions of a grouping pair: with a stub pair (zero tensors, counted
calls) they run on host tensors too -- the float32 products against the `_backward_textbook` rows, the float64 ones through a recorder in
place of _hip.call (the `_backward_map` rows are the same function on the same views).  The other sites are held by the GPU suite.

A recorded call is the full parameter list of the positional function, in its order (defaults filled in); a tensor is compared by
its data pointer, anything else by equality (a b_bound tuple by identity)."""
import inspect

import pytest
import torch

b, c, o, ks, p, na = 2, 3, 5, 2, 4, 4
ck, pa, oks = c * ks, p * na, o * ks            # 6, 16, 10
rp = 2
ra = rp * na                                     # 8: the (row, anchor) axis of the dense product's Z and G ...
ldz = ld = ra + 4                                # ... padded by 4
pad_c = 4                                        # the feature-gradient GEMM's shared operand zero-extended by a row
nt = 2                                           # taps of the intra conv; one slice holds all c channels


class Recorder:
    def __init__(self, monkeypatch):
        from vgtk import _hip
        self._hip, self.calls = _hip, []
        for name in ('gemm', 'gemm_reduce', 'gemm_epilogue'):
            monkeypatch.setattr(_hip, name, self._recorder(name, inspect.signature(getattr(_hip, name))))
        # (the predicate behind matmul_reduce_takes_split: a host function of the library, looked up in the typed prototypes; recorded with any
        # ctypes arguments unwrapped)
        monkeypatch.setattr(_hip.abi, 'eap_gemm_bf16x3_reduce_f32_supported', self._predicate)
        self.predicate_answer = 1

    def _recorder(self, name, sig):
        def record(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            self.calls.append((name,) + tuple(bound.arguments.values()))
            return True
        return record

    def _predicate(self, *args):
        self.calls.append(('reduce_takes_split',) + tuple(a.value if hasattr(a, 'value') else a for a in args))
        return self.predicate_answer


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


def same(got, want, bufs):
    """a recorded call against the literal one: names in `want` stand for the buffers of the row"""
    assert len(got) == len(want), (got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        w = bufs[w] if isinstance(w, str) and i > 0 else w
        if torch.is_tensor(w):
            g = g.data_ptr() if torch.is_tensor(g) else g           # (the predicate is handed pointers)
            assert g == w.data_ptr(), f'argument {i}: another tensor or another first element'
        elif isinstance(w, tuple):
            assert g is w, f'argument {i}: the bound was not passed through'
        else:
            assert type(g) is type(w) and g == w, f'argument {i}: got {g!r}, stated {w!r}\n  got    {got}\n  stated {want}'


def f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


# ---- the call sites -----------------------------------------------------------------------------------------------------------------
# Each row: site, build(_hip) -> (bufs, call), the positional call of the site as it stood before (numbers from its text at the sizes
# above: o=5, pa=16, ck=6, oks=10, ra=8, ldz=ld=12, pad_c=4, b=2).

def _contract_fwd(epilogue):
    def build(_hip):
        W, x, y = f32(o, ck), f32(b, ck, pa), f32(b, o, pa)
        bufs = dict(W=W, x=x, y=y, scale=f32(o), shift=f32(o), res=f32(b, o, p, na).view(b, o, pa))
        if epilogue:
            return bufs, lambda: _hip.matmul_epilogue(W, x, y, bufs['scale'], bufs['shift'], 0.25, bufs['res'])
        return bufs, lambda: _hip.matmul(W, x, y)
    return build


def _contract_bwd_dx(split):
    def build(_hip):
        W, gy, gx = f32(o, ck), f32(b, o, pa), f32(b, ck, pa)
        Wt = W.t().contiguous()
        return dict(W=W, Wt=Wt, gy=gy, gx=gx), (lambda: _hip.matmul(Wt, gy, gx)) if split else (lambda: _hip.matmul(W.t(), gy, gx))
    return build


def _contract_bwd_dw(_hip):
    gy, x, gW = f32(b, o, pa), f32(b, ck, pa), f32(o, ck)
    return dict(gy=gy, x=x, gW=gW), lambda: _hip.matmul_reduce(gy, x.transpose(1, 2), gW)


def _contract_into(layout, epilogue=False):
    def build(_hip):
        W, x = f32(o, ck), f32(b, c, ks, p, na)                 # x: the nominal shape; layout 2 holds X^T [b, pa, ck]
        y = f32(b + 1, o, p, na)[1:].view(b, o, pa)             # a slab of the output: a view that starts inside its storage
        bound = (torch.zeros(b, p, dtype=torch.int32), na, 1.0)
        bufs = dict(W=W, x=x, y=y, bound=bound, scale=f32(o), shift=f32(o), res=f32(b + 1, o, p, na)[1:])
        xt = x.view(b, p * na, c * ks).transpose(1, 2)
        if epilogue:
            return bufs, lambda: _hip.matmul_epilogue(W, xt, y, bufs['scale'], bufs['shift'], 0.25, bufs['res'], b_bound=bound)
        if layout == 2:
            return bufs, lambda: _hip.matmul(W, xt, y, b_bound=bound)
        return bufs, lambda: _hip.matmul(W, x.view(b, c * ks, p * na), y)
    return build


def _weight_grad_from_z(which):
    def build(_hip):
        z4, fc = f32(b, o, ks, ldz), f32(b, c, rp, na).view(b, c, ra)
        z = z4.view(b, o * ks, ldz)[..., :ra]
        d = f32(o * ks * c)
        dt = d.view(c, o * ks)
        bufs = dict(z=z4, fc=fc, d=d, dt=d)
        if which == 'takes':
            return bufs, lambda: _hip.matmul_reduce_takes_split(fc, z.transpose(1, 2), dt)
        if which == 'dt':
            return bufs, lambda: _hip.matmul_reduce(fc, z.transpose(1, 2), dt)
        return bufs, lambda: _hip.matmul_reduce(z, fc.transpose(1, 2), d.view(o * ks, c))
    return build


def _dense_g(_hip):
    W3, fc, g = f32(o * ks, c), f32(b, c, ld), f32(b, o * ks, ld)       # (the product runs over the padded columns too)
    return dict(W3=W3, fc=fc, g=g), lambda: _hip.matmul(W3, fc, g)


def _rows_grad_from_z(_hip):
    W2, z, gFc = f32(pad_c, oks), f32(b, o, ks, ldz), f32(b, pad_c, ldz)
    bound = (torch.zeros(b, ldz // 4, dtype=torch.int32), 4, 1.0)
    return dict(W2=W2, z=z, gFc=gFc, bound=bound), lambda: _hip.matmul(W2, z.view(b, oks, ldz), gFc, b_bound=bound)


def _textbook_dw(layout):
    def build(_hip):
        gy, x, gW = f32(b, o, p, na), f32(b, c, ks, p, na), f32(o, ck)
        if layout == 2:
            return dict(gy=gy, x=x, gW=gW), lambda: _hip.matmul_reduce(gy.view(b, o, pa), x.view(b, pa, ck), gW)
        return dict(gy=gy, x=x, gW=gW), lambda: _hip.matmul_reduce(gy.view(b, o, pa), x.view(b, ck, pa).transpose(1, 2), gW)
    return build


def _textbook_dx(_hip):
    W, gy, x = f32(o, ck), f32(b, o, p, na), f32(b, c, ks, p, na)
    Wt, gx = W.t().contiguous(), torch.empty_like(x.view(b, ck, pa))
    return dict(Wt=Wt, gy=gy, gx=gx), lambda: _hip.matmul(Wt, gy.view(b, o, pa), gx)


def _intra_dw(_hip):
    gy, g, d = f32(b, o, p, na), f32(b, c, nt, p, na), f32(o, c * nt)
    return dict(gy=gy, g=g, d=d), lambda: _hip.matmul_reduce(gy.view(b, o, pa), g.view(b, c * nt, pa).transpose(1, 2), d)


SITES = [
    ('_Contract.forward, folded epilogue', _contract_fwd(True),
     ('gemm_epilogue', 0, 5, 16, 6, 'W', 6, 'x', 16, 96, 'y', 16, 80, 2, 'scale', 'shift', 0.25, 'res', None)),
    ('_Contract.forward', _contract_fwd(False),
     ('gemm', 0, 0, 5, 16, 6, 'W', 6, 0, 'x', 16, 96, 'y', 16, 80, 2, False, None)),
    ('_Contract.backward, dX from W^T written out', _contract_bwd_dx(True),
     ('gemm', 0, 0, 6, 16, 5, 'Wt', 5, 0, 'gy', 16, 80, 'gx', 16, 96, 2, False, None)),
    ('_Contract.backward, dX with the transposition left to the GEMM', _contract_bwd_dx(False),
     ('gemm', 1, 0, 6, 16, 5, 'W', 6, 0, 'gy', 16, 80, 'gx', 16, 96, 2, False, None)),
    ('_Contract.backward, dW', _contract_bwd_dw,
     ('gemm_reduce', 0, 1, 5, 6, 16, 'gy', 16, 80, 'x', 16, 96, 'gW', 6, 2, False)),
    ('_contract_into, transposed intermediate, folded epilogue', _contract_into(2, True),
     ('gemm_epilogue', 1, 5, 16, 6, 'W', 6, 'x', 6, 96, 'y', 16, 80, 2, 'scale', 'shift', 0.25, 'res', 'bound')),
    ('_contract_into, transposed intermediate', _contract_into(2),
     ('gemm', 0, 1, 5, 16, 6, 'W', 6, 0, 'x', 6, 96, 'y', 16, 80, 2, False, 'bound')),
    ('_contract_into, row-major intermediate', _contract_into(0),
     ('gemm', 0, 0, 5, 16, 6, 'W', 6, 0, 'x', 16, 96, 'y', 16, 80, 2, False, None)),
    ('_weight_grad_from_z, the question', _weight_grad_from_z('takes'),
     ('reduce_takes_split', 3, 10, 8, 'fc', 8, 24, 'z', 12, 120, 10)),
    ('_weight_grad_from_z, Fc Z^T', _weight_grad_from_z('dt'),
     ('gemm_reduce', 0, 1, 3, 10, 8, 'fc', 8, 24, 'z', 12, 120, 'dt', 10, 2, False)),
    ('_weight_grad_from_z, Z Fc^T', _weight_grad_from_z('d'),
     ('gemm_reduce', 0, 1, 10, 3, 8, 'z', 12, 120, 'fc', 8, 24, 'd', 3, 2, False)),
    ('_dense_g', _dense_g,
     ('gemm', 0, 0, 10, 12, 3, 'W3', 3, 0, 'fc', 12, 36, 'g', 12, 120, 2, False, None)),
    ('_rows_grad_from_z', _rows_grad_from_z,
     ('gemm', 0, 0, 4, 12, 10, 'W2', 10, 0, 'z', 12, 120, 'gFc', 12, 48, 2, False, 'bound')),
    ('_backward_textbook, dW from the transposed intermediate', _textbook_dw(2),
     ('gemm_reduce', 0, 0, 5, 6, 16, 'gy', 16, 80, 'x', 6, 96, 'gW', 6, 2, False)),
    ('_backward_textbook, dW from the row-major intermediate', _textbook_dw(0),
     ('gemm_reduce', 0, 1, 5, 6, 16, 'gy', 16, 80, 'x', 16, 96, 'gW', 6, 2, False)),
    ('_backward_textbook, dX', _textbook_dx,
     ('gemm', 0, 0, 6, 16, 5, 'Wt', 5, 0, 'gy', 16, 80, 'gx', 16, 96, 2, False, None)),
    ('_backward_map, dW', _textbook_dw(0),
     ('gemm_reduce', 0, 1, 5, 6, 16, 'gy', 16, 80, 'x', 16, 96, 'gW', 6, 2, False)),
    ('_backward_map, dX', _textbook_dx,
     ('gemm', 0, 0, 6, 16, 5, 'Wt', 5, 0, 'gy', 16, 80, 'gx', 16, 96, 2, False, None)),
    ('_IntraConv.backward, dW of one channel slice', _intra_dw,
     ('gemm_reduce', 0, 1, 5, 6, 16, 'gy', 16, 80, 'g', 16, 96, 'd', 6, 2, False)),
]


def test_one_row_per_converted_site():
    assert len(SITES) == 19


@pytest.mark.parametrize('site,build,stated', SITES, ids=[s[0] for s in SITES])
def test_site_states_the_numbers_it_stated_by_hand(rec, site, build, stated):
    bufs, call = build(rec._hip)
    call()
    assert len(rec.calls) == 1, rec.calls
    same(rec.calls[0], stated, bufs)


def test_the_functions_of_the_operator_layer_make_these_calls(rec, monkeypatch):
    """the helpers of vgtk/so3conv/functional.py that run on host tensors once the GEMMs are recorders, against the same rows"""
    from vgtk.so3conv import functional as F
    _hip, rows = rec._hip, {s[0]: s[2] for s in SITES}

    W, x = f32(o, ck), f32(b, c, ks, p, na)
    y = f32(b + 1, o, p, na)[1:].view(b, o, pa)
    bound = (torch.zeros(b, p, dtype=torch.int32), na, 1.0)
    with torch.no_grad():
        ep = F.FoldedEpilogue(f32(o), f32(o), 0.25, f32(b + 1, o, p, na))
    F._contract_into(W, x, y, 2, ep, b0=1, x_bound=bound)
    F._contract_into(W, x, y, 2, x_bound=bound)
    F._contract_into(W, x, y, 0)
    bufs = dict(W=W, x=x, y=y, bound=bound, scale=ep.scale, shift=ep.shift, res=ep.residual[1:])
    for got, row in zip(rec.calls, ('_contract_into, transposed intermediate, folded epilogue', '_contract_into, transposed intermediate',
                                    '_contract_into, row-major intermediate')):
        same(got, rows[row], bufs)
    assert len(rec.calls) == 3 and ep.applied

    z, fc = f32(b, o, ks, ldz), f32(b, c, rp, na).view(b, c, ra)
    for answer, row in ((1, '_weight_grad_from_z, Fc Z^T'), (0, '_weight_grad_from_z, Z Fc^T')):
        del rec.calls[:]
        rec.predicate_answer = answer
        assert F._weight_grad_from_z(z, fc, b, c, o, ks, ra, ldz).shape == (o, c * ks)
        assert len(rec.calls) == 2
        out = rec.calls[1][12]
        same(rec.calls[0], rows['_weight_grad_from_z, the question'], dict(z=z, fc=fc))
        same(rec.calls[1], rows[row], dict(z=z, fc=fc, d=out, dt=out))

    del rec.calls[:]
    W2, zb = f32(pad_c, oks), (torch.zeros(b, ldz // 4, dtype=torch.int32), 4, 1.0)
    g = F._rows_grad_from_z(z, W2, c, rp, na, ldz, True, zb)
    assert g.shape == (b, c, rp, na) and len(rec.calls) == 1
    same(rec.calls[0], rows['_rows_grad_from_z'], dict(W2=W2, z=z, gFc=rec.calls[0][12], bound=zb))


# ---- the skeleton around a grouping pair ----------------------------------------------------------------------------------------------

n_sup = 5                                        # support rows per cloud


class StubGrouping:
    """a grouping pair whose two methods return zero tensors of the right shape and record their calls"""

    def __init__(self, layout=0, dtype=torch.float32):
        self.layout, self.mid, self.dtype = layout, ks, dtype
        self.grouped, self.transposed, self.made = [], [], []

    def group(self, feats, b0, b1):
        self.grouped.append((b0, b1))
        self.made.append(torch.zeros(b1 - b0, feats.shape[1], self.mid, p, na, dtype=self.dtype))
        return self.made[-1]

    def group_transposed(self, gx, n, b0, b1):
        assert tuple(gx.shape) == (b1 - b0, c, self.mid, p, na) and gx.is_contiguous() and n == n_sup
        self.transposed.append((b0, b1, gx.data_ptr()))
        return torch.zeros(b1 - b0, c, n, na, dtype=self.dtype)


def test_the_textbook_backward_of_a_pair_makes_these_calls(rec):
    """float32, the whole batch in one slab: dW in the view expression of the layout, then dX from W^T written out; X regrouped only for dW"""
    from vgtk.so3conv import functional as F
    rows = {s[0]: s[2] for s in SITES}
    gy, W, feats, x = f32(b, o, p, na), f32(o, ck), f32(b, c, n_sup, na), f32(b, c, ks, p, na)
    for layout, row in ((2, '_backward_textbook, dW from the transposed intermediate'), (0, '_backward_textbook, dW from the row-major intermediate')):
        del rec.calls[:]
        stub = StubGrouping(layout)
        gF, gW = F._backward_textbook(stub, gy, W, feats, x, True, True, [(0, b)])
        assert [call[0] for call in rec.calls] == ['gemm_reduce', 'gemm']                 # X kept: dW first, then dX
        same(rec.calls[0], rows[row], dict(gy=gy, x=x, gW=gW))
        Wt, gx = rec.calls[1][6], rec.calls[1][12]
        same(rec.calls[1], rows['_backward_textbook, dX'], dict(Wt=Wt, gy=gy, gx=gx))
        assert Wt.data_ptr() != W.data_ptr() and tuple(Wt.shape) == (ck, o) and Wt.is_contiguous()      # W^T written out
        assert stub.grouped == [] and stub.transposed == [(0, b, gx.data_ptr())]
        assert tuple(gF.shape) == tuple(feats.shape) and tuple(gW.shape) == tuple(W.shape)
    # X not kept
    for need_f, need_w, groups, calls in ((False, True, 1, ['gemm_reduce']), (True, False, 0, ['gemm']), (True, True, 1, ['gemm_reduce', 'gemm'])):
        del rec.calls[:]
        stub = StubGrouping(0)
        gF, gW = F._backward_textbook(stub, gy, W, feats, None, need_f, need_w, [(0, b)])
        assert len(stub.grouped) == groups and len(stub.transposed) == int(need_f), (need_f, need_w, stub.grouped)
        assert [call[0] for call in rec.calls] == calls
        assert (gF is not None) == need_f and (gW is not None) == need_w
        if need_w:
            same(rec.calls[0], rows['_backward_textbook, dW from the row-major intermediate'], dict(gy=gy, x=stub.made[0], gW=gW))


def test_the_textbook_backward_in_float64_runs_slab_by_slab(monkeypatch):
    """float64: X regrouped per slab, dW accumulated onto the slabs before, dX from the VIEW W^T (no copy), every product over its slab's clouds"""
    from vgtk import _hip
    from vgtk.so3conv import functional as F
    calls = []
    monkeypatch.setattr(_hip, 'call', lambda name, ref, *args, tag=None: calls.append((name,) + args))
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    nb = 3
    gy, W, feats = f64(nb, o, p, na), f64(o, ck), f64(nb, c, n_sup, na)
    one_cloud = 8 * ck * pa
    for limit, want in ((one_cloud, [(0, 1), (1, 2), (2, 3)]), (1 << 62, [(0, 3)])):
        del calls[:]
        monkeypatch.setattr(F, 'F64_X_BYTES_MAX', limit)
        slabs = F._f64_slabs(nb, one_cloud)
        assert slabs == want
        stub = StubGrouping(0, torch.float64)
        gF, gW = F._backward_textbook(stub, gy, W, feats, None, True, True, slabs)
        assert [call[0] for call in calls] == ['eap_gemm_f64_reduce', 'eap_gemm_f64'] * len(slabs)      # per slab: dW, then dX
        reduces, products = calls[0::2], calls[1::2]
        # (ta, tb, M, N, K, A, lda, sa, B, ldb, sb, out, ldc, batch, accumulate) / (..., out, ldc, sc, batch)
        assert [r[15] for r in reduces] == [int(b0 > 0) for b0, _ in slabs]
        assert [r[14] for r in reduces] == [b1 - b0 for b0, b1 in slabs] and [g[15] for g in products] == [b1 - b0 for b0, b1 in slabs]
        for (b0, b1), r, g, x in zip(slabs, reduces, products, stub.made):
            assert r[6].data_ptr() == gy[b0:b1].data_ptr() and r[9].data_ptr() == x.data_ptr() and r[12].data_ptr() == gW.data_ptr()
            assert g[1] == 1 and g[6].data_ptr() == W.data_ptr() and g[9].data_ptr() == gy[b0:b1].data_ptr()      # A = W^T as a view of W
        assert stub.grouped == slabs and [t[:2] for t in stub.transposed] == slabs
        assert tuple(gF.shape) == tuple(feats.shape) and gF.dtype == torch.float64


def test_the_forward_loop_of_a_pair_groups_and_contracts_slab_by_slab(rec, monkeypatch):
    from vgtk.so3conv import functional as F
    monkeypatch.setattr(F, 'X_CHUNK_CLOUDS', 2)
    nb = 3
    W, feats, y = f32(o, ck), f32(nb, c, n_sup, na), f32(nb, o, p, na)
    contract = lambda W, x, ys, b0: F._contract_into(W, x, ys, 0)
    stub = StubGrouping(0)
    assert F._group_contract(stub, feats, W, y, F._f32_slabs(nb, False), False, contract) is None       # X is scratch
    assert stub.grouped == [(0, 2), (2, 3)] and len(rec.calls) == 2
    for (b0, b1), x, got in zip(stub.grouped, stub.made, rec.calls):
        same(got, ('gemm', 0, 0, o, pa, ck, 'W', ck, 0, 'x', pa, ck * pa, 'y', pa, o * pa, b1 - b0, False, None), dict(W=W, x=x, y=y[b0:b1]))
    del rec.calls[:]
    stub = StubGrouping(0)
    kept = F._group_contract(stub, feats, W, y, F._f32_slabs(nb, True), True, contract)                  # a kept X: one slab of all clouds
    assert stub.grouped == [(0, 3)] and kept is stub.made[0] and len(rec.calls) == 1
    same(rec.calls[0], ('gemm', 0, 0, o, pa, ck, 'W', ck, 0, 'x', pa, ck * pa, 'y', pa, o * pa, nb, False, None), dict(W=W, x=kept, y=y))


# ---- the derivation -----------------------------------------------------------------------------------------------------------------

M, N, K, Z = 3, 5, 4, 2


def _derivations():
    A, B, C = f32(Z, M, K), f32(Z, K, N), f32(Z, M, N)
    At, Bt = f32(Z, K, M), f32(Z, N, K)
    wide, flat = f32(Z, K, 8), f32(7 + Z * M * K)
    yield 'contiguous', (A, B, C), (0, 0, 3, 5, 4, A, 4, 12, B, 5, 20, C, 5, 15, 2)
    yield 'A transposed', (At.transpose(1, 2), B, C), (1, 0, 3, 5, 4, At, 3, 12, B, 5, 20, C, 5, 15, 2)
    yield 'B transposed', (A, Bt.transpose(1, 2), C), (0, 1, 3, 5, 4, A, 4, 12, Bt, 4, 20, C, 5, 15, 2)
    yield 'B a column slice', (A, wide[:, :, 2:7], C), (0, 0, 3, 5, 4, A, 4, 12, wide[0, 0, 2:], 8, 32, C, 5, 15, 2)
    yield 'A shared by the batch', (A[0], B, C), (0, 0, 3, 5, 4, A, 4, 0, B, 5, 20, C, 5, 15, 2)
    Cp = f32(Z, M, 8)
    yield 'out with a padded pitch', (A, B, Cp[:, :, :N]), (0, 0, 3, 5, 4, A, 4, 12, B, 5, 20, Cp, 8, 24, 2)
    Bs = f32(Z, 30)
    yield 'an item stride larger than the item', (A, Bs[:, :K * N].view(Z, K, N), C), (0, 0, 3, 5, 4, A, 4, 12, Bs, 5, 30, C, 5, 15, 2)
    yield 'a storage offset', (flat[7:].view(Z, M, K), B, C), (0, 0, 3, 5, 4, flat[7:], 4, 12, B, 5, 20, C, 5, 15, 2)
    A1, C1 = f32(Z, 1, K), f32(Z, 1, N)
    yield 'M = 1', (A1, B, C1), (0, 0, 1, 5, 4, A1, 4, 4, B, 5, 20, C1, 5, 5, 2)
    B1, C1 = f32(Z, K, 1), f32(Z, M, 1)
    yield 'N = 1', (A, B1, C1), (0, 0, 3, 1, 4, A, 4, 12, B1, 1, 4, C1, 1, 3, 2)
    A1, B1 = f32(Z, M, 1), f32(Z, 1, N)
    yield 'K = 1', (A1, B1, C), (0, 0, 3, 5, 1, A1, 1, 3, B1, 5, 5, C, 5, 15, 2)
    Bt1, C1 = f32(Z, 1, K), f32(Z, M, 1)                            # N = 1 as the transpose of a [1, K] row: one reading only
    yield 'N = 1, B transposed', (A, Bt1.transpose(1, 2), C1), (0, 1, 3, 1, 4, A, 4, 12, Bt1, 4, 4, C1, 1, 3, 2)


DERIVATIONS = list(_derivations())


@pytest.mark.parametrize('name,views,stated', DERIVATIONS, ids=[d[0] for d in DERIVATIONS])
def test_derivation(rec, name, views, stated):
    rec._hip.matmul(*views)
    assert len(rec.calls) == 1
    same(rec.calls[0], ('gemm',) + stated + (False, None), {})


def test_derivation_of_the_reduce_and_epilogue_forms(rec):
    _hip = rec._hip
    A, Bt, C, Cp = f32(Z, M, K), f32(Z, N, K), f32(M, 8), f32(Z, M, 8)
    _hip.matmul_reduce(A, Bt.transpose(1, 2), C[:, :N])
    same(rec.calls[0], ('gemm_reduce', 0, 1, 3, 5, 4, A, 4, 12, Bt, 4, 20, C, 8, 2, False), {})
    _hip.matmul_reduce(A[1], Bt.transpose(1, 2), C[:, :N])
    same(rec.calls[1], ('gemm_reduce', 0, 1, 3, 5, 4, A[1], 4, 0, Bt, 4, 20, C, 8, 2, False), {})
    scale, shift, res = f32(M), f32(M), f32(Z, M, 8)[:, :, :N]           # laid out like out
    assert _hip.matmul_epilogue(A[0], Bt.transpose(1, 2), Cp[:, :, :N], scale, shift, 0.5, res) is True
    same(rec.calls[2], ('gemm_epilogue', 1, 3, 5, 4, A, 4, Bt, 4, 20, Cp, 8, 24, 2, scale, shift, 0.5, res, None), {})
    rec.predicate_answer = 0
    assert _hip.matmul_reduce_takes_split(A, Bt.transpose(1, 2), C[:, :N]) is False
    same(rec.calls[3], ('reduce_takes_split', 3, 5, 4, A, 4, 12, Bt, 4, 20, 8), {})
    assert len(rec.calls) == 4


def test_sizes_of_one_make_two_readings_possible_and_the_untransposed_one_wins():
    """the rule of _hip.operand: ld of an untransposed view is stride(-2) as torch reports it"""
    from vgtk._hip import operand
    assert operand(f32(Z, K, 1)) == (0, 1, K, Z, K, 1)                           # strides (4, 1, 1): both readings, trans = 0
    assert operand(f32(Z, 1, K).transpose(1, 2)) == (1, K, K, Z, K, 1)           # strides (4, 1, 4): the rows are contiguous only
    assert operand(f32(Z, 1, K)) == (0, K, K, Z, 1, K)
    assert operand(f32(K, N)) == (0, N, 0, 1, K, N)
    assert operand(f32(K, N).t()) == (1, N, 0, 1, N, K)
    assert operand(f32(Z, K, 8)[:, 1:, 2:7]) == (0, 8, 32, Z, K - 1, N)


# ---- the refusals -------------------------------------------------------------------------------------------------------------------

def overclaiming(view, *shape):
    """view(t) of a tensor t of this shape whose storage then lost its last element: the view claims more than the storage holds"""
    t = f32(*shape)
    v = view(t)
    t.untyped_storage().resize_(t.untyped_storage().nbytes() - 4)
    return v


def _refusals():
    A, B, C = f32(Z, M, K), f32(Z, K, N), f32(Z, M, N)
    yield 'neither stride is 1', lambda: (f32(Z, M, 2 * K)[:, :, ::2], B, C)
    yield 'the inner sizes disagree', lambda: (f32(Z, M, K + 1), B, C)
    yield 'M of out disagrees', lambda: (A, B, f32(Z, M + 1, N))
    yield 'N of out disagrees', lambda: (A, B, f32(Z, M, N + 1))
    yield 'the batch of A disagrees', lambda: (f32(Z + 1, M, K), B, C)
    yield 'the batch of out disagrees', lambda: (A, B, f32(Z + 1, M, N))
    yield 'A is float64', lambda: (A.double(), B, C)
    yield 'B is float16', lambda: (A, B.half(), C)
    yield 'out is float64', lambda: (A, B, C.double())
    yield 'out is transposed', lambda: (A, B, f32(Z, N, M).transpose(1, 2))
    yield 'A claims more than its storage holds', lambda: (overclaiming(lambda t: t, Z, M, K), B, C)
    yield 'a transposed B claims more than its storage holds', lambda: (A, overclaiming(lambda t: t.transpose(1, 2), Z, N, K), C)
    yield 'a slice of B claims more than its storage holds', lambda: (A, overclaiming(lambda t: t[:, :, 8 - N:], Z, K, 8), C)
    yield 'out claims more than its storage holds', lambda: (A, B, overclaiming(lambda t: t, Z, M, N))
    yield 'the items of out overlap', lambda: (A, B, torch.as_strided(f32(Z * M * N), (Z, M, N), (M * N - 1, N, 1)))
    yield 'the rows of out overlap', lambda: (A, B, torch.as_strided(f32(Z * M * N), (Z, M, N), (M * N, N - 1, 1)))
    yield 'B is one matrix', lambda: (A, B[0], C)
    yield 'a 4-D operand', lambda: (A[None], B, C)


REFUSALS = list(_refusals())


@pytest.mark.parametrize('name,views', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(rec, name, views):
    with pytest.raises(RuntimeError):
        rec._hip.matmul(*views())
    assert rec.calls == []


def test_every_form_refuses(rec):
    """the other three forms go through the same checks (one case of each kind), and have some of their own"""
    _hip = rec._hip
    A, B, C = f32(Z, M, K), f32(Z, K, N), f32(Z, M, N)
    scale = shift = f32(M)
    forms = (lambda a, b, c: _hip.matmul_reduce(a, b, c[0]), lambda a, b, c: _hip.matmul_reduce_takes_split(a, b, c[0]),
             lambda a, b, c: _hip.matmul_epilogue(a[0], b, c, scale, shift, 0.5))
    for form in forms:
        form(A, B, C)                                                # (taken as they are)
        for a, b, c in ((A, f32(Z, K + 1, N), C), (A, B, f32(Z, M, N + 1)), (A, B.double(), C), (A, B, f32(Z, N, M).transpose(1, 2)),
                        (A, f32(Z, K, 2 * N)[:, :, ::2], C), (A, overclaiming(lambda t: t[:, :, 8 - N:], Z, K, 8), C)):
            del rec.calls[:]
            with pytest.raises(RuntimeError):
                form(a, b, c)
            assert rec.calls == []
    for form in (_hip.matmul_reduce, _hip.matmul_reduce_takes_split):
        with pytest.raises(RuntimeError):
            form(A, B, overclaiming(lambda t: t, M, N))
        with pytest.raises(RuntimeError):
            form(f32(Z + 1, M, K), B, C[0])                          # the batch of A disagrees
    with pytest.raises(RuntimeError):
        _hip.matmul_epilogue(A[0], B, overclaiming(lambda t: t, Z, M, N), scale, shift, 0.5)
    with pytest.raises(RuntimeError):
        _hip.matmul_reduce(A, B, C)                                  # out of the reduce form is one matrix
    with pytest.raises(RuntimeError):
        _hip.matmul(A, B, C[0])                                      # ... of the others a stack
    with pytest.raises(RuntimeError):
        _hip.matmul_epilogue(A, B, C, scale, shift, 0.5)             # the epilogue kernel's A is shared by the batch
    with pytest.raises(RuntimeError):
        _hip.matmul_epilogue(f32(K, M).t(), B, C, scale, shift, 0.5)                         # ... and row-major
    with pytest.raises(RuntimeError):
        _hip.matmul_epilogue(A[0], B, C, scale, shift, 0.5, residual=f32(Z, M, N - 1))       # a residual smaller than out
    with pytest.raises(RuntimeError):
        _hip.matmul_epilogue(A[0], B, C, scale, shift, 0.5, residual=f32(Z, M, N).double())
    with pytest.raises(RuntimeError):
        _hip.matmul_epilogue(A[0], B, C, scale, shift, 0.5, residual=f32(Z, M, 2 * N)[:, :, :N])     # storage enough, another pitch
    with pytest.raises(RuntimeError):
        _hip.matmul_epilogue(A[0], B, f32(Z, M, 2 * N)[:, :, :N], scale, shift, 0.5, residual=f32(Z, M, N))   # contiguous, out is not
    assert rec.calls == []
