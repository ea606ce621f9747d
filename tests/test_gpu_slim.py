"""SLIM on the device against the NumPy restatement (tests/slim_ref.py): the weights, the sweeps and the updates of every
column bit for bit over catalogues at the window's edges and past the grid; the optimality conditions of the columns'
problems recomputed in long double from the weights alone; scores / top-K / ranks bit for bit from constructed weights; the
whole model end to end; errors and state.  The shapes are edges (tests/slim_cases.py), taken from tfr_slim_plan."""
import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import slim as S
from tests import itemknn_cases as IC
from tests import slim_cases as SC
from tests import slim_ref as R

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    bad = np.flatnonzero((np.asarray(gi) != np.asarray(wi)).reshape(-1) | (bits(gs) != bits(ws)).reshape(-1))
    assert bad.size == 0, "%s: %d of %d slots differ, first at flat index %d: got (%d, %r) want (%d, %r)" % (
        what, bad.size, np.asarray(wi).size, bad[0], np.asarray(gi).reshape(-1)[bad[0]], np.asarray(gs).reshape(-1)[bad[0]],
        np.asarray(wi).reshape(-1)[bad[0]], np.asarray(ws).reshape(-1)[bad[0]])


def csr_of(lists):
    p = np.zeros(len(lists) + 1, np.int64)
    p[1:] = np.cumsum([len(x) for x in lists])
    return p, (np.concatenate(lists).astype(np.int32) if len(lists) else np.zeros(0, np.int32))


def assert_solve(m, want, what):
    """the model's weights and statistics against (W, sweeps, updates, converged, W64) of the restatement"""
    W, sweeps, updates, conv, _ = want
    got = m.weights()
    bad = np.argwhere(bits(got) != bits(W))
    assert got.dtype == np.float32 and bad.size == 0, "%s: %d weights differ, first at %s: got %r want %r" % (
        what, len(bad), bad[0], got[tuple(bad[0])], W[tuple(bad[0])])
    assert np.array_equal(m.sweeps(), sweeps), what
    assert np.array_equal(m.updates(), updates), what
    assert np.array_equal(m.converged(), conv), what


def solve_with(m, l1, positive, max_iter, tol):
    m.l1, m.positive, m.max_iter, m.tol = float(l1), bool(positive), int(max_iter), float(tol)
    return m.solve()


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.BIT_CASES)
def test_solve_bit_for_bit(name):
    indptr, items, nu, ni = SC.case(name)
    if name in SC.SIZES:
        assert (nu, ni) == (80, SC.SIZES[name](S.plan(100)["window"]))
    for l1, beta in SC.PENALTIES:
        with T.SLIM(nu, ni, l2=beta) as m:
            m.load((indptr, items))
            A = m.gram()
            assert A.dtype == np.float64 and np.array_equal(bits64(A), bits64(SC.gram(name, beta))), (name, beta)
            for positive in (True, False):
                solve_with(m, l1, positive, 10, 1e-4)
                assert_solve(m, SC.solved(name, l1, beta, positive, 10, 1e-4), "%s l1 %g beta %g positive %s" % (name, l1, beta, positive))
    if name == "lengths":                                                      # nobody has item 0: d = 0 at beta = 0, its row and column stay 0
        assert SC.gram(name, 0.0)[0, 0] == 0 and SC.gram(name, 0.0)[8, 8] == nu
    if name == "duplicates":
        g = SC.gram(name, 0.0)
        assert np.array_equal(g[:40, :40], g[40:80, 40:80]) and np.array_equal(g[3], g[80])


def test_solve_bit_for_bit_past_the_grid():
    """more columns than workgroups: the column stride runs, and the workgroups that take a second column reuse q and w"""
    indptr, items, nu, ni = SC.case("stride")
    assert nu == 60 and S.plan(ni)["grid"] == ni - 3
    with T.SLIM(nu, ni, l2=5.0) as m:
        m.load((indptr, items))
        m.build_gram()
        for positive in (True, False):
            solve_with(m, 2.0, positive, 10, 1e-4)
            assert_solve(m, SC.solved("stride", 2.0, 5.0, positive, 10, 1e-4), "stride positive %s" % positive)
    with T.SLIM(nu, ni, l1=0.5, l2=1.0, max_iter=2) as m:
        m.fit((indptr, items))
        want = SC.solved("stride", 0.5, 1.0, True, 2, 1e-4)
        assert_solve(m, want, "stride l1 0.5 beta 1")
        assert want[2][-3:].min() > 0                                          # the second stride's columns have work to do


def test_stopped_early_and_tol_zero():
    for name in ("size:T+1", "duplicates"):
        indptr, items, nu, ni = SC.case(name)
        with T.SLIM(nu, ni, l2=1.0) as m:
            m.load((indptr, items))
            m.build_gram()
            for positive in (True, False):
                for max_iter, tol in ((1, 1e-4), (2, 1e-4), (12, 0.0)):
                    solve_with(m, 0.5, positive, max_iter, tol)
                    want = SC.solved(name, 0.5, 1.0, positive, max_iter, tol)
                    assert_solve(m, want, "%s positive %s max_iter %d tol %g" % (name, positive, max_iter, tol))
                    if max_iter <= 2:
                        assert want[1].max() == max_iter and not want[3].all()  # some column was stopped by max_iter


def test_l1_above_every_cooccurrence_gives_zero_weights():
    indptr, items, nu, ni = SC.case("full_user")
    A = SC.gram("full_user", 1.0)
    l1 = float(np.abs(A - np.diag(np.diag(A))).max())
    for positive in (True, False):
        with T.SLIM(nu, ni, l1=l1, l2=1.0, positive=positive) as m:
            m.fit((indptr, items))
            assert not bits(m.weights()).any()                                 # +0 everywhere
            assert m.sweeps().tolist() == [1] * ni and not m.updates().any() and m.converged().all()
            solve_with(m, np.nextafter(l1, 0.0), positive, 100, 1e-4)          # a hair below: the largest pair enters
            assert m.updates().any() and (m.weights() != 0).any()


# ---- 2. optimality, whatever the path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l1,beta", [(1.0, 5.0), (0.5, 1.0)])
def test_weights_meet_the_optimality_conditions(l1, beta):
    """With r_i = a_ij - sum over k != i of A[i, k] w_k in long double, a column at its optimum has r_i - l1 = d_i w_i where
    w_i > 0 and r_i - l1 <= 0 where w_i = 0.  The solver stops after a sweep whose largest change is at most tol max|w|;
    coordinate i was exact for the q[i] it saw, and the later coordinates of that sweep moved q[i] by at most
    tol max|w| sum over k != i of |A[i, k]|; the float64 updates of q[i] add at most 4 eps updates_j max|A|.  The weights are
    read as float32: each carries a relative 2^-24, which moves r_i - d_i w_i by at most 2^-24 sum over k of |A[i, k]| |w_k|."""
    (indptr, items, nu, ni), _, _ = SC.planted_case()
    tol = 1e-4
    with T.SLIM(nu, ni, l1=l1, l2=beta, max_iter=200, tol=tol) as m:
        m.fit((indptr, items))
        W, A, updates, conv, sweeps = m.weights(), m.gram(), m.updates(), m.converged(), m.sweeps()
    assert conv.all() and sweeps.max() < 200
    assert (W >= 0).all() and not np.diag(W).any() and (W != 0).any(axis=0).all()
    assert np.array_equal(bits64(A), bits64(SC.planted_gram(beta)))
    ex, _ = R.kkt_excess(A, W, l1, True)
    absA = np.abs(A)
    rowsum = absA.sum(axis=1) - np.diag(absA)
    wmax = np.abs(W).max(axis=0).astype(np.float64) * (1 + 2.0 ** -23)
    first = tol * wmax[None, :] * rowsum[:, None]
    b = first + 4 * R.EPS * updates[None, :].astype(np.float64) * absA.max() + 2.0 ** -24 * (absA @ np.abs(W).astype(np.float64))
    off = ~np.eye(ni, dtype=bool)
    print("l1 %g beta %g: sweeps up to %d, largest excess / bound %.3g, / its first term %.3g" % (
        l1, beta, sweeps.max(), float((ex[off] / b[off]).max()), float((ex[off] / first[off]).max())))
    assert (ex[off] <= b[off]).all()


# ---- 3. serving from constructed weights -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_recommend_and_rank_at_the_slice_edges(extra):
    w = S.plan(100, 10, 1, 1)["width"]
    ni = 2 * w + 3 if extra is None else w + extra
    assert S.plan(ni, 10, 1, 1)["slices"] == (3 if extra is None else 2 if extra == 1 else 1)
    W = SC.constructed_weights(ni)
    indptr, items, nu, _ = SC.ladder(ni)
    users = np.arange(nu, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    x = csr_of(lists)
    with T.SLIM(nu, ni) as m:
        m.load((indptr, items))
        m.set_weights(W)
        assert np.array_equal(bits(m.weights()), bits(W))
        scores = [R.user_scores(lst, W) for lst in lists]
        for k in (1, 10, 256):
            for excl in (None, lists):
                want_items = np.empty((nu, k), np.int32)
                want_scores = np.empty((nu, k), np.float32)
                for q in range(nu):
                    want_items[q], want_scores[q] = R.topk(scores[q], k, () if excl is None else excl[q])
                got = m.recommend(users, k, exclude=None if excl is None else x)
                assert_same(got, (want_items, want_scores), "recommend k=%d excluded=%s" % (k, excl is not None))
                if excl is not None:                                           # the lists alone, their own items excluded
                    assert_same(m.recommend_lists((indptr, items), k, exclude=True), got, "recommend_lists k=%d" % k)
        # targets on both sides of every slice edge, and the last item
        tg = np.unique([c for c in (0, w - 1, w, w + 1, 2 * w - 1, 2 * w, ni - 1) if 0 <= c < ni]).astype(np.int32)
        tp = np.arange(nu + 1, dtype=np.int64) * tg.size
        got = m.rank_items(users, (tp, np.tile(tg, nu)), exclude=x)
        want = np.concatenate([R.ranks(s, tg, lst) for s, lst in zip(scores, lists)])
        assert got.dtype == np.int32 and np.array_equal(got, want)
        for k in (1, 10, 256):                                                 # rank < k exactly where recommend holds the item
            top = m.recommend(users, k, exclude=x, return_scores=False)
            for q in range(nu):
                for t, r in zip(tg, got[tp[q]:tp[q + 1]]):
                    assert (0 <= r < k) == (t in top[q].tolist()), (k, q, t, r)
                    if 0 <= r < k:
                        assert top[q, r] == t


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------
def test_end_to_end_fit_metrics_and_move():
    (indptr, items, nu, ni), tu, ti = SC.planted_case()
    assert (nu, ni) == (300, 150)
    l1, beta = 1.0, 5.0
    train = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
    users = np.arange(nu, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    x = csr_of(lists)
    want = SC.planted_solved(l1, beta, True, 100, 1e-4)
    with T.SLIM(nu, ni, l1=l1, l2=beta) as m:
        m.fit(train)
        assert m.fit_ms > 0 and m.fit_ms_parts["gram"] > 0 and m.fit_ms_parts["solve"] > 0
        assert m.fit_ms == pytest.approx(m.fit_ms_parts["gram"] + m.fit_ms_parts["solve"])
        assert_solve(m, want, "planted")
        assert m.converged().all()
        W = m.weights()
        res = T.evaluate_ranking(m, tu, ti, exclude=train, ks=(10,))
        q_users = res["users"]
        want_ranks = np.concatenate([R.ranks(R.user_scores(lists[u], want[0]), res["items"][res["indptr"][q]:res["indptr"][q + 1]], lists[u])
                                     for q, u in enumerate(q_users)])
        assert np.array_equal(res["ranks"], want_ranks)
        host = T.ranking_metrics(want_ranks, res["indptr"], ni - np.diff(indptr)[q_users], ks=(10,))
        for name in ("recall@10", "ndcg@10"):
            assert np.array_equal(res[name], host[name])
            assert res["mean"][name] == float(host[name].mean())
        print("planted: mean recall@10 %.3f, ndcg@10 %.3f" % (res["mean"]["recall@10"], res["mean"]["ndcg@10"]))
        assert res["mean"]["recall@10"] > 0.3                                  # the clusters are found: chance is 10 / 138
        served = m.recommend(users, 20, exclude=x)
        with T.SLIM(nu, ni) as b:                                              # a fitted model moves without a refit
            b.set_weights(W)
            assert np.array_equal(bits(b.weights()), bits(W))
            assert_same(b.recommend_lists(x, 20), served, "lists on the second handle")
            b.load((indptr, items))
            b.set_weights(W)
            assert_same(b.recommend(users, 20, exclude=x), served, "resident on the second handle")
            assert np.array_equal(b.rank_items(res["users"], (res["indptr"], res["items"]), exclude=csr_of([lists[u] for u in q_users])),
                                  res["ranks"])
        stats = (m.sweeps(), m.updates())
        A = m.gram()                                                           # the solve kept the Gram matrix
        m.fit()                                                                # two fits: the same bits
        assert np.array_equal(bits(m.weights()), bits(W))
        assert np.array_equal(m.sweeps(), stats[0]) and np.array_equal(m.updates(), stats[1])
        with T.SLIM(nu, ni, l1=l1, l2=123.0) as c:                             # a caller's matrix: l2 is not added to it
            c.fit_gram(A)
            assert np.array_equal(bits(c.weights()), bits(W))
            assert np.array_equal(c.sweeps(), stats[0]) and np.array_equal(c.updates(), stats[1])
            assert c.fit_ms_parts["gram"] == 0
            assert_same(c.recommend_lists(x, 20), served, "lists after fit_gram")


# ---- 5. errors and state ---------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    lib = L.load()
    i64 = lambda *v: np.array(v, np.int64)
    i32 = lambda *v: np.array(v, np.int32)
    f64p = lambda a: a.ctypes.data_as(L._f64p)
    out = np.full(8, 77, np.int32)
    n = 6
    with T.SLIM(3, n, l1=0.25, l2=1.0) as m:
        h = m._h
        u = i32(0, 1)
        buf64, buf32, st = np.zeros((n, n)), np.zeros((n, n), np.float32), np.zeros(n, np.int32)
        # before a load, a Gram matrix and weights
        assert lib.tfr_slim_gram(h) == L.ERR_STATE
        assert lib.tfr_slim_solve(h, 0.25, 1, 10, 1e-4, None) == L.ERR_STATE
        assert lib.tfr_slim_get_gram(h, 0, n, f64p(buf64)) == L.ERR_STATE
        assert lib.tfr_slim_get_weights(h, 0, n, L.ptr_f32(buf32)) == L.ERR_STATE
        assert lib.tfr_slim_get_stats(h, L.ptr_i32(st), None, None) == L.ERR_STATE
        assert lib.tfr_slim_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        assert lib.tfr_slim_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(1, 2)), None, None, L.ptr_i32(out)) == L.ERR_STATE
        assert lib.tfr_slim_topk_lists(h, L.ptr_i64(i64(0, 1)), L.ptr_i32(i32(1)), 1, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        with pytest.raises(T.TfrError) as e:
            m.recommend(u, 2)
        assert e.value.code == L.ERR_STATE
        # load: each refusal leaves the handle unloaded; wrong shapes are refused before the library
        for indptr, items, code in [(i64(1, 2, 3, 4), i32(0, 1, 2, 3), L.ERR_ARG), (i64(0, 2, 1, 3), i32(0, 1, 2), L.ERR_ARG),
                                    (i64(0, 2, 3, 3), i32(4, 2, 1), L.ERR_ARG), (i64(0, 2, 3, 3), i32(2, 6, 1), L.ERR_OOB)]:
            assert lib.tfr_slim_load(h, L.ptr_i64(indptr), L.ptr_i32(items)) == code
            assert lib.tfr_slim_gram(h) == L.ERR_STATE
        with pytest.raises(ValueError):
            m.load((i64(0, 1, 2), i32(0, 1)))                                  # two rows for three users
        for bad in (np.zeros((n, n + 1)), np.zeros((n - 1, n - 1)), np.zeros(n)):
            with pytest.raises(ValueError):
                m.set_gram(bad)
            with pytest.raises(ValueError):
                m.set_weights(bad)
        m.load((i64(0, 2, 4, 4), i32(0, 1, 1, 2)))
        assert lib.tfr_slim_solve(h, 0.25, 1, 10, 1e-4, None) == L.ERR_STATE                  # loaded, no Gram matrix yet
        assert lib.tfr_slim_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        assert lib.tfr_slim_gram(h) == L.OK
        assert lib.tfr_slim_get_gram(h, 0, n, f64p(buf64)) == L.OK and buf64[:3, :3].tolist() == [[2, 1, 0], [1, 3, 1], [0, 1, 2]]
        assert lib.tfr_slim_get_gram(h, 4, 3, f64p(buf64)) == L.ERR_ARG                        # window past the items
        assert lib.tfr_slim_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE       # a Gram matrix is no fit
        # solve: its arguments are checked first, and a refused solve leaves the state alone
        for l1, max_iter, tol in ((-1.0, 10, 1e-4), (float("nan"), 10, 1e-4), (float("inf"), 10, 1e-4), (0.25, 0, 1e-4),
                                  (0.25, -3, 1e-4), (0.25, 10, -1e-4), (0.25, 10, float("nan"))):
            assert lib.tfr_slim_solve(h, l1, 1, max_iter, tol, None) == L.ERR_ARG, (l1, max_iter, tol)
        assert lib.tfr_slim_get_weights(h, 0, n, L.ptr_f32(buf32)) == L.ERR_STATE
        assert lib.tfr_slim_solve(h, 0.25, 1, 10, 1e-4, None) == L.OK
        assert lib.tfr_slim_solve(h, 0.25, 1, 10, 1e-4, None) == L.OK                          # the Gram matrix is kept
        assert lib.tfr_slim_get_weights(h, 0, n, L.ptr_f32(buf32)) == L.OK
        assert lib.tfr_slim_get_stats(h, L.ptr_i32(st), None, None) == L.OK and st.min() >= 1
        assert lib.tfr_slim_solve(h, -1.0, 1, 10, 1e-4, None) == L.ERR_ARG
        assert np.array_equal(bits(m.weights()), bits(buf32))                                  # refused: still fitted
        # queries
        assert lib.tfr_slim_topk(h, L.ptr_i32(u), 2, 0, None, None, L.ptr_i32(out), None) == L.ERR_ARG
        assert lib.tfr_slim_topk(h, L.ptr_i32(u), 2, 257, None, None, L.ptr_i32(out), None) == L.ERR_ARG
        assert lib.tfr_slim_topk(h, L.ptr_i32(i32(0, 3)), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_OOB
        assert lib.tfr_slim_topk_lists(h, L.ptr_i64(i64(0, 2)), L.ptr_i32(i32(3, 3)), 1, 2, None, None, L.ptr_i32(out), None) == L.ERR_ARG
        assert lib.tfr_slim_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(2, 9)), None, None, L.ptr_i32(out)) == L.ERR_OOB
        assert out.tolist() == [77] * 8                                        # no refused call wrote anything
        # set_gram: values that are not finite, a matrix that is not symmetric; the matrix held stays
        good = buf64.copy()
        for bad in (np.where(np.eye(n) > 0, np.nan, good), np.where(np.eye(n) > 0, np.inf, good), good + np.triu(np.full((n, n), 1e-3), 1)):
            assert lib.tfr_slim_set_gram(h, f64p(np.ascontiguousarray(bad))) == L.ERR_ARG
        assert lib.tfr_slim_get_gram(h, 0, n, f64p(buf64)) == L.OK and np.array_equal(buf64, good)
        # set_weights: values that are not finite, windows; constructed weights have no statistics
        before = m.weights()
        bad = before.copy()
        bad[4, 1] = np.inf
        assert lib.tfr_slim_set_weights(h, 0, n, L.ptr_f32(bad)) == L.ERR_ARG
        assert lib.tfr_slim_set_weights(h, 4, 3, L.ptr_f32(before)) == L.ERR_ARG
        assert np.array_equal(bits(m.weights()), bits(before))                 # untouched
        row = np.full((1, n), 0.5, np.float32)
        assert lib.tfr_slim_set_weights(h, 2, 1, L.ptr_f32(row)) == L.OK       # a fitted model takes a window
        assert m.weights()[2].tolist() == [0.5] * n and np.array_equal(bits(m.weights()[3]), bits(before[3]))
        assert lib.tfr_slim_get_stats(h, L.ptr_i32(st), None, None) == L.ERR_STATE
        # a second load forgets Gram, weights and statistics
        m.solve()
        m.load((i64(0, 1, 2, 3), i32(0, 1, 2)))
        assert lib.tfr_slim_get_gram(h, 0, n, f64p(buf64)) == L.ERR_STATE
        assert lib.tfr_slim_get_weights(h, 0, n, L.ptr_f32(buf32)) == L.ERR_STATE
        assert lib.tfr_slim_get_stats(h, L.ptr_i32(st), None, None) == L.ERR_STATE
        assert lib.tfr_slim_solve(h, 0.25, 1, 10, 1e-4, None) == L.ERR_STATE
        assert lib.tfr_slim_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        assert lib.tfr_slim_set_weights(h, 0, 2, L.ptr_f32(before)) == L.ERR_STATE              # without weights: all rows at once
        assert lib.tfr_slim_set_weights(h, 0, n, L.ptr_f32(before)) == L.OK
        assert lib.tfr_slim_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.OK
        assert np.array_equal(bits64(m.gram()), bits64(np.diag([2.0, 2, 2, 1, 1, 1])))          # gram() rebuilds from the new pattern


def test_a_refused_load_leaves_a_fitted_model_serving():
    (indptr, items, nu, ni), _, _ = SC.planted_case()
    users = np.arange(0, nu, 5, dtype=np.int32)
    x = csr_of(IC.rows_of(indptr, items, users))
    with T.SLIM(nu, ni) as m:
        m.fit((indptr, items))
        before, W, A, sweeps = m.recommend(users, 10, exclude=x), m.weights(), m.gram(), m.sweeps()
        bad = items.copy()
        bad[-1] = ni                                                           # the last id of the last row: out of range
        assert L.load().tfr_slim_load(m._h, L.ptr_i64(indptr), L.ptr_i32(bad)) == L.ERR_OOB
        assert_same(m.recommend(users, 10, exclude=x), before, "after the refused load")
        assert np.array_equal(bits(m.weights()), bits(W)) and np.array_equal(bits64(m.gram()), bits64(A))
        assert np.array_equal(m.sweeps(), sweeps)
