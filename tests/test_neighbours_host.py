"""The NumPy statement of the nearest-neighbour contract (tests/neighbours_ref.py) against a brute-force float64 cosine / dot
followed by a lexsort, and the launch plan's LDS budget (tfr_neighbours_plan is host-only).  No device."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests.neighbours_ref import neighbours_ref, neighbour_scores, row_rnorm, scores_f64, dyadic_table, pow4_table
from tests import widths as W

LDS_PER_CU = 160 * 1024                                   # the limit tests/test_lds_budget.py uses


def brute(Tab, rows, k, metric, excl=None, lo=0, hi=None, item_abs=False):
    """float64 scores, then one lexsort per row by (score descending, id ascending)"""
    S = scores_f64(Tab, rows, metric, item_abs)
    R = S.shape[1]
    hi = R if hi is None else hi
    ids = np.full((len(rows), k), -1, np.int32)
    sc = np.full((len(rows), k), -np.inf)
    for r, a in enumerate(rows):
        ok = np.zeros(R, bool)
        ok[lo:hi] = True
        ok[a] = False
        if excl is not None:
            ok[np.asarray(excl[r], np.int64)] = False
        cand = np.flatnonzero(ok)
        order = np.lexsort((cand, -S[r, cand]))[:k]
        ids[r, :order.size] = cand[order]
        sc[r, :order.size] = S[r, cand[order]]
    return ids, sc


@pytest.mark.parametrize("metric,maker", [("dot", dyadic_table), ("dot", pow4_table), ("cosine", pow4_table)])
@pytest.mark.parametrize("D", [1, 4, 5, 27, 64])
def test_exact_tables_equal_the_float64_lexsort(metric, maker, D):
    rs = np.random.RandomState(100 + D)
    R = 90
    Tab = maker(rs, R, D)
    Tab[7] = Tab[3]; Tab[50] = Tab[3]; Tab[51] = -Tab[3]           # exact ties and their mirror
    Tab[11] = 0                                                    # a zero row
    rows = np.array([3, 7, 11, 0, 89, 3], np.int64)
    for k in (1, 10, 89, 120):
        ids, sc = neighbours_ref(Tab, rows, k, metric)
        wi, ws = brute(Tab, rows, k, metric)
        assert np.array_equal(ids, wi), (metric, D, k)
        assert np.array_equal(sc.astype(np.float64), ws), (metric, D, k)


def test_random_tables_agree_with_float64_up_to_f32_rounding():
    rs = np.random.RandomState(7)
    R, D, k = 400, 33, 10
    Tab = rs.normal(0, .3, (R, D)).astype(np.float32)
    rows = np.arange(0, R, 3)
    for metric in ("dot", "cosine"):
        S64 = scores_f64(Tab, rows, metric)
        S32 = neighbour_scores(Tab, rows, metric)
        tol = np.abs(S32 - S64).max()
        assert tol <= 1e-5 * np.abs(S64).max()
        ids, sc = neighbours_ref(Tab, rows, k, metric)
        wi, ws = brute(Tab, rows, k, metric)
        for r in range(rows.size):
            assert np.all(np.abs(sc[r] - S64[r, ids[r]]) <= tol)
            assert np.all(S64[r, ids[r]] >= ws[r, -1] - 2 * tol)   # nothing returned lies below the true k-th by more than rounding
            clear = ws[r] > ws[r, -1] + 2 * tol                    # true members clear of the boundary are all returned
            assert set(wi[r][clear].tolist()) <= set(ids[r].tolist())


def test_self_exclusions_zero_rows_padding_range_and_ties():
    rs = np.random.RandomState(9)
    R, D = 40, 8
    Tab = dyadic_table(rs, R, D)
    Tab[5] = 0
    Tab[20] = Tab[2]; Tab[30] = Tab[2]; Tab[31] = Tab[2]
    rows = np.array([2, 5, 20, 39], np.int64)
    for metric in ("dot", "cosine"):
        ids, sc = neighbours_ref(Tab, rows, R + 5, metric)
        for r, a in enumerate(rows):
            assert a not in ids[r]                                           # self never returned
            assert np.array_equal(np.sort(ids[r, :R - 1]), np.delete(np.arange(R), a))
            assert np.all(ids[r, R - 1:] == -1) and np.all(sc[r, R - 1:] == -np.inf)   # k larger than the eligible rows
        # the copies of row 2 tie exactly: returned in id order, the query's own id left out
        i0, _ = neighbours_ref(Tab, [2], 3, "cosine")
        i1, _ = neighbours_ref(Tab, [30], 3, "cosine")
        assert i0[0].tolist() == [20, 30, 31] and i1[0].tolist() == [2, 20, 31]
        # exclusion rows
        excl = [np.array([20, 30]), np.array([], np.int64), np.arange(R), np.array([0])]
        ids, sc = neighbours_ref(Tab, rows, 6, metric, excl=excl)
        assert not set(ids[0].tolist()) & {2, 20, 30} and np.all(ids[2] == -1) and 0 not in ids[3]
        assert np.array_equal(ids, brute(Tab, rows, 6, metric, excl=excl)[0])
        # candidate range: ids stay row ids of the table; a query outside the range is legal
        ids, sc = neighbours_ref(Tab, rows, 6, metric, lo=18, hi=33)
        assert np.all((ids >= 18) & (ids < 33)) and 20 not in ids[2]
        assert np.array_equal(ids, brute(Tab, rows, 6, metric, lo=18, hi=33)[0])
    # a zero row: cosine +0 against everything (ordered by id, not NaN), and +0 as a candidate of every other row
    ids, sc = neighbours_ref(Tab, [5], 4, "cosine")
    assert ids[0].tolist() == [0, 1, 2, 3] and np.all(sc[0] == 0) and not np.any(np.signbit(sc[0]))
    assert row_rnorm(Tab)[5] == 0
    assert np.all(neighbour_scores(Tab, rows, "cosine")[:, 5] == 0)


def test_item_abs_and_nan_rows():
    rs = np.random.RandomState(10)
    Tab = dyadic_table(rs, 30, 6)
    ids, sc = neighbours_ref(Tab, [1, 2], 5, "dot", item_abs=True)
    wi, ws = neighbours_ref(np.abs(Tab), [1, 2], 5, "dot")
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws) and np.all(sc >= 0)
    Tab[4, 0] = np.nan
    ids, sc = neighbours_ref(Tab, [1, 4], 29, "cosine")
    assert 4 not in ids[0] and ids[0, -1] == -1                 # a NaN score is never returned
    assert np.all(ids[1] == -1)                                  # every score of a NaN row is NaN


@pytest.mark.parametrize("D", sorted(set(W.TOPK) | {1, 256}))
def test_plan_lds_fits_a_cu(D):
    for k in (1, 10, 128, 129, 256):
        for n, cand in ((1, 1), (31, 300), (3706, 3706), (10677, 10677), (1 << 20, 1 << 20)):
            p = T.neighbours.plan(D, k, n, cand)
            assert 0 < p["lds_bytes"] <= LDS_PER_CU, (D, k, n, cand, p)
            assert p["rows_per_block"] == (32 if k <= 128 else 16)
            assert 1 <= p["slices"] <= 256 and p["slices"] * k <= 8192
            assert p["row_chunk"] % p["rows_per_block"] == 0 and p["row_chunk"] * p["slices"] * k * 8 <= 128 << 20


def test_plan_refuses_bad_arguments():
    for bad in ((64, 0, 10, 10), (64, 257, 10, 10), (64, 10, 10, 0), (64, 10, -1, 10), (65, 10, 10, 10)):
        with pytest.raises(T.TfrError) as e:
            T.neighbours.plan(*bad)
        assert e.value.code == L.ERR_ARG


def test_metric_names():
    assert T.neighbours.metric_code("dot") == 0 and T.neighbours.metric_code("cosine") == 1
    with pytest.raises(ValueError):
        T.neighbours.metric_code("euclid")
