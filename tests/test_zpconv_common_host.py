"""CPU: what tests/test_gpu_zpconv_regimes.py relies on, checked without a device (tests/zpconv_common.py) --
  * the float64 and int64 numpy references agree with the C oracle (oracle/native_ops.c) on the shapes of tests/test_gpu_parity.py's
    test_inter_zpconv / test_intra_zpconv and on the hand-derived cases of tests/test_oracle_native.py;
  * the builders keep their promises over the whole case table: rows per cloud, no repeats inside a list, A < 2^24 in exact mode,
    k u <= 2^-14 in float mode, and the host-side predicates (point ranges, stage count, LDS limits) the table's expectations are read from;
  * the comparator is sensitive: a correct result with ONE term dropped, doubled, moved to the neighbouring row, given the next kernel point's
    weight, or with one unreferenced row left non-zero is rejected in both modes on every case that has such a term;
  * float mode sees precision loss: weights rounded to 11 significant bits are rejected on every float case, the correctly rounded result
    stays at a ratio <= 0.5."""
import numpy as np
import pytest

import zpconv_common as ZC
from oracle import native
from test_oracle_native import known_zpconv

f32, f64, i64 = np.float32, np.float64, np.int64


@pytest.mark.parametrize('shape', [(2, 9, 11, 12, 5, 8, 3), (1, 17, 20, 60, 24, 64, 10), (2, 4, 4, 1, 3, 7, 2)])
def test_inter_references_agree_with_the_oracle(shape):
    b, p, q, a, k, ann, c = shape
    rng = np.random.default_rng(1)
    idx = rng.integers(0, q, (b, p, a, k, ann)).astype(np.int32)
    w, feats = rng.random((b, p, a, k, ann)), rng.standard_normal((b, c, q, a))
    g = rng.standard_normal((b, c, k, p, a))
    np.testing.assert_allclose(ZC.inter_forward(idx, w, feats), native.inter_zpconv_forward(idx, w, feats), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ZC.inter_backward(idx, w, g, q), native.inter_zpconv_backward(idx, w, g, q), rtol=1e-12, atol=1e-12)
    # integer operands: the int64 reference, the float64 reference and the oracle (float32 and float64) agree exactly
    wi, fi, gi = (rng.choice([-3, -2, -1, 1, 2, 3], t.shape).astype(f32) for t in (w, feats, g))
    want = ZC.inter_forward(idx, wi, fi, i64)
    assert ZC.exact_equal(ZC.inter_forward(idx, wi, fi, f64), want) and ZC.exact_equal(native.inter_zpconv_forward(idx, wi, fi), want)
    want = ZC.inter_backward(idx, wi, gi, q, i64)
    assert ZC.exact_equal(ZC.inter_backward(idx, wi, gi, q, f64), want) and ZC.exact_equal(native.inter_zpconv_backward(idx, wi, gi, q), want)
    # T and A are what they say: ones as operands count the products
    ones_w, ones_g = np.ones_like(wi), np.ones_like(gi)
    assert ZC.exact_equal(ZC.inter_backward(idx, ones_w, ones_g, q, i64), np.broadcast_to(ZC.inter_backward_T(idx, q), (b, c, q, a)).astype(i64))
    assert ZC.exact_equal(ZC.inter_forward(idx, ones_w, np.ones_like(fi), i64), np.full((b, c, k, p, a), ZC.inter_forward_T(idx), i64))


def test_intra_references_agree_with_the_oracle():
    rng = np.random.default_rng(2)
    b, c, p, a_in, a_out, k, ann = 2, 5, 33, 60, 60, 4, 12
    idx = rng.integers(0, a_in, (a_out, ann)).astype(np.int32)
    w, feats, g = rng.random((a_out, k, ann)), rng.standard_normal((b, c, p, a_in)), rng.standard_normal((b, c, k, p, a_out))
    np.testing.assert_allclose(ZC.intra_forward(idx, w, feats), native.intra_zpconv_forward(idx, w, feats), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ZC.intra_backward(idx, w, g, a_in), native.intra_zpconv_backward(idx, w, g, a_in), rtol=1e-12, atol=1e-12)
    wi, fi, gi = (rng.choice([-3, -2, -1, 1, 2, 3], t.shape).astype(f32) for t in (w, feats, g))
    assert ZC.exact_equal(native.intra_zpconv_forward(idx, wi, fi), ZC.intra_forward(idx, wi, fi, i64))
    assert ZC.exact_equal(native.intra_zpconv_backward(idx, wi, gi, a_in), ZC.intra_backward(idx, wi, gi, a_in, i64))
    assert ZC.exact_equal(ZC.intra_backward(idx, np.ones_like(wi), np.ones_like(gi), a_in, i64),
                          np.broadcast_to(ZC.intra_backward_T(idx, k, a_in), (b, c, p, a_in)).astype(i64))


@pytest.mark.parametrize('acc', [f64, i64])
def test_references_give_the_hand_derived_answers(acc):
    known_zpconv(lambda i, w, f: ZC.inter_forward(i, w * 2, f, acc) / 2, lambda i, w, g, n: ZC.inter_backward(i, w * 2, g, n, acc) / 2,
                 lambda i, w, f: ZC.intra_forward(i, w, f, acc), lambda i, w, g, n: ZC.intra_backward(i, w, g, n, acc))


def test_index_builders_keep_their_promises():
    lists = ZC.lists_with_rows(3, 11, 300, 291, 5)                         # (asserts inside: R rows, no repeats, rows 0 and nq - 1, rank != row)
    assert lists.shape == (3, 11, 64) and all(np.unique(lists[i]).size == 291 for i in range(3))
    assert not np.array_equal(lists[0], lists[1])
    with pytest.raises(AssertionError):
        ZC.lists_with_rows(1, 4, 300, 290, 5)                              # 4 lists of 64 cannot name 290 rows
    with pytest.raises(AssertionError):
        ZC.lists_with_rows(1, 11, 291, 291, 5)                             # no unreferenced row left
    idx = ZC.broadcast5d(lists, 4, 24)
    assert idx.shape == (3, 11, 4, 24, 64) and idx.flags.c_contiguous and (idx[:, :, 3, 23] == lists).all()
    dev = ZC.deviate(idx, (2, -1, -1, -1, -1), 300)
    assert (dev != idx).sum() == 1 and dev[2, 10, 3, 23, 63] != idx[2, 10, 3, 23, 63] and 0 <= dev.min() and dev.max() < 300
    pad = ZC.padded(lists)
    assert (pad[..., 32:] == lists[..., :1]).all() and (pad[..., :32] == lists[..., :32]).all()
    arb = ZC.arbitrary5d(2, 3, 4, 5, 6, 7, 1)
    assert arb.shape == (2, 3, 4, 5, 6) and arb.dtype == np.int32 and arb.max() < 7 and not (arb == arb[:, :, :1, :1]).all()


def _hot_ranges(b, np_):
    S = 1 if b >= 8 else (8 + b - 1) // b
    return min(S, np_)


@pytest.mark.parametrize('case', ZC.ALL_CASES, ids=repr)
def test_case_table_conditions(case):
    """Every case: the index is what its descriptor says, the expectations follow from the selection code's own formulas, and the two
    conditions of the modes hold (asserted inside ZC.reference: A < 2^24; k u <= 2^-14 where the case runs in float mode -- and a case that
    does not run in float mode really exceeds the cap)."""
    b, np_, nq, na, ks, nn, c = case.dims
    idx = ZC.make_index(case)
    assert idx.shape == (b, np_, na, ks, nn) and idx.dtype == np.int32 and idx.flags.c_contiguous
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < nq)
    per = case.index if isinstance(case.index, list) else [case.index] * b
    for bi, d in enumerate(per):
        one_list = bool((idx[bi] == idx[bi, :, :1, :1]).all())
        lists = idx[bi, :, 0, 0]
        if isinstance(d, int):
            assert one_list and np.unique(lists).size == d and all(np.unique(r).size == nn for r in lists)
            assert np.setdiff1d(np.arange(nq), lists).size >= 1 and {0, nq - 1} <= set(lists.ravel().tolist())
        elif d == 'lists':
            assert one_list
        elif d[0] == 'pad':
            assert one_list and all(np.unique(r).size < nn for r in lists)
        elif d[0] == 'dev':
            assert not one_list and (idx[bi] != idx[bi, :, :1, :1]).sum() <= ks * na
        elif d[0] == 'one':
            assert (idx[bi] == d[1]).all()
    if case.status is not None:                                             # the on-chip backward's own rules, restated
        assert (ks, nn) == (24, 64) and na % 4 == 0 and c % 32 == 0 and nq <= 16384
        assert case.S == _hot_ranges(b, np_)
        for bi, d in enumerate(per):
            assert case.status[bi] == (0 if isinstance(d, int) and d <= ZC.HOT_RCAP else 1)
    for mode in ZC.MODES:
        if mode == 'float' and not case.float_ok:
            assert ZC.ku_max(case, ZC.products(case, idx)) > ZC.KU_CAP
            continue
        ref, T, A = ZC.reference(case.name, mode)
        assert ref.shape == ((b, c, ks, np_, na) if case.kind == 'fwd' else (b, c, nq, na))
        assert ref.dtype == (i64 if mode == 'exact' else f64)
        assert not A.size or A.max() < (ZC.EXACT_CAP if mode == 'exact' else np.inf)


def test_case_table_places_the_edges_the_kernels_have():
    """the thresholds the table is built around, from the kernels' own constants"""
    two = lambda R: (R + 1) * 512 + 2 * (4 * 24 * 32 * 4 + 64 * 4) <= 158 * 1024
    assert two(266) and not two(267) and ZC.HOT_TWO_STAGE_ROWS == 266
    assert (158 * 1024 - 4 * 24 * 32 * 4 - 64 * 4) // 512 - 1 == ZC.HOT_RCAP
    pitch = lambda na: ((na + 3) & ~3) + (0 if (((na + 3) >> 2) & 7) == 1 else 4) + 4
    rows_lds = lambda na, nn: 4 * 8 * nn * pitch(na) + 4 * nn
    assert rows_lds(60, 72) <= 160 * 1024 < rows_lds(60, 76)
    scalar_lds = lambda size, na, nn: (size + 4) * na * (2 * nn + 1)
    assert scalar_lds(4, 64, 159) <= 160 * 1024 < scalar_lds(4, 64, 160) and scalar_lds(8, 64, 106) <= 160 * 1024 < scalar_lds(8, 64, 107)
    names = {c.name for c in ZC.CASES}
    for need in ('hot_rows266', 'hot_rows267', 'hot_rows290', 'hot_rows291', 'hot_bitmap_limit', 'hot_past_bitmap_limit', 'prod_sliced_batch',
                 'prod_no_scratch', 'matrix_b65', 'rows_nn72_na60_last_in_lds', 'scalar_fwd_f32_lds_past', 'scalar_bwd_f64_lds_past'):
        assert need in names


def _cases_with_terms():
    return [c for c in ZC.ALL_CASES if c.raises is None and c.dims[0] > 0]


@pytest.mark.parametrize('case', _cases_with_terms(), ids=repr)
def test_comparator_rejects_one_wrong_term(case):
    hits = 0
    for mode in ZC.modes_of(case):
        ref, T, A = ZC.reference(case.name, mode)
        correct = ref.astype(ZC.DT[case.width])                            # the reference rounded once
        ok, figure = ZC.check(correct, case.name, mode)
        assert ok and figure <= 0.5, (mode, figure)
        for kind in ZC.PERTURBATIONS:
            wrong = ZC.perturbed(case, mode, kind)
            if wrong is None:
                continue
            hits += 1
            ok, figure = ZC.check(wrong, case.name, mode)
            assert not ok, (mode, kind, figure)
        nan = correct.copy()
        if nan.size:
            nan.flat[nan.size // 2] = np.nan
            assert not ZC.check(nan, case.name, mode)[0]
    b, np_, nq, na, ks, nn, c = case.dims
    if nn >= 2:                                                            # at least 2 entries per affected element: the perturbations exist
        assert hits >= 2 * len(ZC.modes_of(case)), hits


def test_every_perturbation_is_exercised():
    seen = {k: 0 for k in ZC.PERTURBATIONS}
    for name in ('hot_rows267', 'hot_rows290', 'prod_c20', 'matrix_np9', 'rows_ks9', 'scalar_bwd_f64_c7'):
        for kind in ZC.PERTURBATIONS:
            seen[kind] += ZC.perturbed(ZC.BY_NAME[name], 'exact', kind) is not None
    assert all(v >= 2 for v in seen.values()), seen


@pytest.mark.parametrize('case', [c for c in _cases_with_terms() if c.float_ok and c.dims[5] > 0], ids=repr)
def test_float_mode_rejects_weights_of_11_bits(case):
    idx, w, x = ZC.operands(case, 'float')
    lossy = ZC.evaluate(case, idx, ZC.round_to_bits(w, 11), x, f64).astype(ZC.DT[case.width])
    ok, ratio = ZC.check(lossy, case.name, 'float')
    assert not ok and ratio > 1.0, ratio
    ok, ratio = ZC.check(ZC.reference(case.name, 'float')[0].astype(ZC.DT[case.width]), case.name, 'float')
    assert ok and ratio <= 0.5, ratio


@pytest.mark.parametrize('shape', ZC.INTRA_CASES, ids=str)
def test_intra_table_conditions_and_sensitivity(shape):
    for width in ('f32', 'f64'):
        for mode in ZC.MODES:
            idx, w, feats, grad = ZC.intra_operands(shape, mode, width)
            for direction, (ref, T, A) in ZC.intra_reference(shape, mode, width).items():
                correct = ref.astype(ZC.DT[width])
                bound = ZC.float_bound(T, A, width)
                wrong = correct.copy()
                wrong.flat[-1] += 1 if mode == 'exact' else 4 * np.max(bound)
                if mode == 'exact':
                    assert ZC.exact_equal(correct, ref) and not ZC.exact_equal(wrong, ref)
                else:
                    assert ZC.worst_ratio(correct, ref, bound) <= 0.5 < 1.0 < ZC.worst_ratio(wrong, ref, bound)
