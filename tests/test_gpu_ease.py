"""EASE on the device against the NumPy restatement (tests/ease_ref.py), one stage per test so a failure names its stage:
the Gram matrix bit for bit, the inverse on exact integers bit for bit and on rounded cases within K eps cond2(G) max|P| of a
long double inverse (K from tests/ease_cases.py error_constant), the refusal of an indefinite matrix, the weights bit for bit
from the device's own P, scores / top-K / ranks bit for bit from constructed weights, and the whole model end to end.  The
shapes are edges (tests/ease_cases.py), taken from tfr_ease_plan."""
import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import ease as E
from tests import ease_cases as EC
from tests import ease_ref as R
from tests import itemknn_cases as IC

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


def all_but(n_items, keep):
    return np.setdiff1d(np.arange(n_items, dtype=np.int32), keep).astype(np.int32)


def exclusion_modes(lists, n_items):
    """(name, per-query exclusion lists or None): none, the own list, everything but two items (so k pads)"""
    yield "none", None
    yield "own", lists
    yield "all but two", [all_but(n_items, [q % n_items, (3 * q + 7) % n_items]) for q in range(len(lists))]


def want_topk(lists, B, k, excl=None):
    items = np.empty((len(lists), k), np.int32)
    scores = np.empty((len(lists), k), np.float32)
    for q, lst in enumerate(lists):
        items[q], scores[q] = R.topk(R.user_scores(lst, B), k, () if excl is None else excl[q])
    return items, scores


# ---- 1. the Gram matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.5, 500.0])
def test_gram_bit_for_bit(lam):
    for name in EC.gram_case_names():
        indptr, items, nu, ni = EC.case(name)
        with T.EASE(nu, ni, regularization=lam) as m:
            m.load((indptr, items))
            got = m.gram()
        want = EC.gram(name, lam)
        assert got.dtype == np.float64 and np.array_equal(bits64(got), bits64(want)), name
    n = np.diff(np.asarray(sp.csr_matrix((np.ones(EC.case("lengths")[1].size), EC.case("lengths")[1], EC.case("lengths")[0]),
                                         shape=(300, 130)).tocsc().indptr))
    assert n[:9].tolist() == [0, 1, 63, 64, 65, 255, 256, 257, 300]            # the list lengths the case is there for


# ---- 2. the inverse on exact integers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["blocks", "tiles"])
def test_inverse_exact_integers(which):
    nb, tile = EC.nb(), EC.tile()
    n, split = (2 * nb + 3, nb + 6) if which == "blocks" else (2 * tile + 1, tile - 7)
    g, p = EC.integer_case(n, split)
    assert np.array_equal(R.inverse_blocked(g, nb), p)                         # the condition the inputs must meet
    with T.EASE(5, n) as m:
        got = m.fit_gram(g, keep_inverse=True).inverse()
    bad = np.argwhere(got != p)
    assert bad.size == 0, "%d entries differ, first at %s: got %r want %r" % (len(bad), bad[0], got[tuple(bad[0])], p[tuple(bad[0])])


# ---- 3. the inverse, rounded -------------------------------------------------------------------------------------------------
def test_inverse_within_the_error_constant():
    r_max, K = EC.error_constant()
    worst = (0.0, None)
    for name, lam in EC.inverse_cases():
        g, p_ld, cond = EC.inverse_case(name, lam)
        assert cond <= EC.COND_MAX
        with T.EASE(5, g.shape[0]) as m:
            got = m.fit_gram(g, keep_inverse=True).inverse()
            again = m.fit_gram(g, keep_inverse=True).inverse()
        assert np.array_equal(bits64(got), bits64(got.T)), (name, lam)        # both triangles carry equal bits
        assert np.array_equal(bits64(got), bits64(again)), (name, lam)        # a second solve gives the same bits
        ratio = R.error_ratio(got, p_ld, cond)
        print("inverse %s lambda %g: n %d cond %.3g ratio %.3g (K %.3g)" % (name, lam, g.shape[0], cond, ratio, K))
        worst = max(worst, (ratio, (name, lam)))
        assert ratio <= K, (name, lam, ratio, K)
    print("device's largest ratio %.3g at %s; restatement r_max %.3g, K %.3g" % (worst[0], worst[1], r_max, K))


def test_inverse_of_1100_items_by_its_residual():
    """the grid-stride loops and many blocks: max|G P - I| in float64 on the host, held to 8 x that of np.linalg.inv"""
    indptr, items, nu, ni = EC.sized_case(1100, n_users=2000)
    g = R.gram(indptr, items, nu, ni, 10.0)
    with T.EASE(nu, ni, regularization=10.0) as m:
        m.load((indptr, items))
        assert np.array_equal(bits64(m.gram()), bits64(g))
        p = m.fit(keep_inverse=True).inverse()
    assert np.array_equal(bits64(p), bits64(p.T))
    eye = np.eye(ni)
    res_dev = float(np.abs(g @ p - eye).max())
    res_np = float(np.abs(g @ np.linalg.inv(g) - eye).max())
    print("n 1100: max|G P - I| device %.3g, np.linalg.inv %.3g" % (res_dev, res_np))
    assert res_dev <= 8 * res_np


# ---- 4. not positive definite ------------------------------------------------------------------------------------------------
def test_indefinite_matrix_is_refused_and_the_handle_survives():
    g = EC.indefinite_case()
    n = g.shape[0]
    good, p_good = EC.integer_case(n, 20)
    with T.EASE(5, n) as m:
        with pytest.raises(T.TfrError) as e:
            m.fit_gram(g)
        assert e.value.code == L.ERR_ARG and "column 67" in str(e.value)
        out = np.zeros((n, n), np.float32)
        lib = L.load()
        assert lib.tfr_ease_get_weights(m._h, 0, n, L.ptr_f32(out)) == L.ERR_STATE              # unfitted
        assert lib.tfr_ease_get_f64(m._h, 0, n, np.zeros((n, n)).ctypes.data_as(L._f64p)) == L.ERR_STATE
        assert lib.tfr_ease_solve(m._h, 0, None) == L.ERR_STATE                                 # nothing left to solve
        assert np.array_equal(m.fit_gram(good, keep_inverse=True).inverse(), p_good)
        # a fitted model that meets an indefinite matrix is unfitted again
        with pytest.raises(T.TfrError):
            m.fit_gram(g)
        assert lib.tfr_ease_get_weights(m._h, 0, n, L.ptr_f32(out)) == L.ERR_STATE
        for bad in (np.where(np.eye(n) > 0, np.nan, g), g + np.triu(np.full((n, n), 1e-3), 1), g - 2 * np.eye(n)):
            assert lib.tfr_ease_set_gram(m._h, np.ascontiguousarray(bad).ctypes.data_as(L._f64p)) == L.ERR_ARG


# ---- 5. the weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lam", [("lengths", 0.25), ("full_user", 500.0), ("size:131", 10.0)])
def test_weights_bit_for_bit_from_the_device_inverse(name, lam):
    indptr, items, nu, ni = EC.case(name)
    with T.EASE(nu, ni, regularization=lam) as m:
        m.fit((indptr, items), keep_inverse=True)
        p, b = m.inverse(), m.weights()
    want = R.weights(p)
    assert b.dtype == np.float32 and np.array_equal(bits(b), bits(want))
    assert not bits(np.diag(b)).any()                                          # +0 on the diagonal
    if name == "lengths":                                                      # nobody has item 0: its row and column are zero
        assert p[0, 0] == 1 / lam and not p[0, 1:].any() and not p[1:, 0].any()
        assert not b[0].any() and not b[:, 0].any()


# ---- 6. scores, top-K and ranks from constructed weights -----------------------------------------------------------------------
@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_recommend_and_rank_at_the_slice_edges(extra):
    w = EC.w_score()
    ni = 2 * w + 3 if extra is None else w + extra
    assert E.plan(ni, 10, 1, 1)["slices"] == (3 if extra is None else 2 if extra == 1 else 1)
    B = EC.constructed_weights(ni)
    indptr, items, nu, _ = EC.ladder(ni)
    users = np.arange(nu, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    with T.EASE(nu, ni) as m:
        m.load((indptr, items))
        m.set_weights(B)
        assert np.array_equal(bits(m.weights()), bits(B))
        for k in (1, 10, 256):
            for name, excl in exclusion_modes(lists, ni):
                want = want_topk(lists, B, k, excl)
                x = None if excl is None else csr_of(excl)
                assert_same(m.recommend(users, k, exclude=x), want, "recommend k=%d excl=%s" % (k, name))
                assert_same(m.recommend_lists((indptr, items), k, exclude=False if x is None else x), want,
                            "recommend_lists k=%d excl=%s" % (k, name))
        assert_same(m.recommend_lists((indptr, items), 10, exclude=True), want_topk(lists, B, 10, lists), "exclude=True")
        # an empty list scores +0 everywhere: the k lowest ids
        got = m.recommend(users[:1], 10)
        assert got[0].tolist() == [list(range(10))] and bits(got[1]).tolist() == [[0] * 10]
        # targets on both sides of every slice edge, and the last item
        tg = np.unique([c for c in (0, w - 1, w, w + 1, 2 * w - 1, 2 * w, ni - 1) if 0 <= c < ni]).astype(np.int32)
        tp = np.arange(users.size + 1, dtype=np.int64) * tg.size
        got = m.rank_items(users, (tp, np.tile(tg, users.size)), exclude=csr_of(lists))
        want = np.concatenate([R.ranks(R.user_scores(lst, B), tg, lst) for lst in lists])
        assert got.dtype == np.int32 and np.array_equal(got, want)


def test_exact_ties_go_by_id():
    ni = 200
    B = EC.constructed_weights(ni)
    with T.EASE(3, ni) as m:
        m.set_weights(B)
        lst = np.array([3, 50, 120], np.int32)
        items, scores = m.recommend_lists((np.array([0, 3], np.int64), lst), 256, exclude=None)
    sc = R.user_scores(lst, B)
    assert_same((items, scores), want_topk([lst], B, 256), "ties")
    run = [int(np.flatnonzero(items[0] == j)[0]) for j in range(100, 109)]     # nine identical columns: one score, ids ascending
    assert run == list(range(run[0], run[0] + 9)) and len(set(bits(sc[100:109]).tolist())) == 1


def test_rank_is_the_position_in_recommend():
    ni = 300
    B = EC.constructed_weights(ni)
    indptr, items, nu, _ = EC.ladder(ni, seed=41)
    rs = np.random.RandomState(6)
    users = np.array([0, 5, 5, 17, 20, 12, 6], np.int32)
    lists = IC.rows_of(indptr, items, users)
    targets = [np.sort(rs.choice(ni, n, replace=False)).astype(np.int32) for n in (ni, 0, 70, 3, 1, 0, 12)]
    targets[3] = np.sort(np.concatenate([lists[3][:2], all_but(ni, lists[3])[:1]])).astype(np.int32)    # two excluded targets
    with T.EASE(nu, ni) as m:
        m.load((indptr, items))
        m.set_weights(B)
        for name, excl in exclusion_modes(lists, ni):
            x = None if excl is None else csr_of(excl)
            got = m.rank_items(users, csr_of(targets), exclude=x)
            want = np.concatenate([R.ranks(R.user_scores(lst, B), t, () if excl is None else excl[q])
                                   for q, (lst, t) in enumerate(zip(lists, targets))])
            assert got.dtype == np.int32 and np.array_equal(got, want), name
            tp = csr_of(targets)[0]
            for k in (1, 10, 256):
                top = m.recommend(users, k, exclude=x, return_scores=False)
                for q in range(users.size):
                    for t, r in zip(targets[q], got[tp[q]:tp[q + 1]]):
                        assert (0 <= r < k) == (t in top[q].tolist()), (name, k, q, t, r)
                        if 0 <= r < k:
                            assert top[q, r] == t
            if name == "own":
                assert got[tp[3]:tp[4]].tolist().count(-1) == 2
        # rows without targets and n = 0 are no-ops
        assert m.rank_items(users, (np.zeros(users.size + 1, np.int64), np.zeros(0, np.int32))).size == 0
        out = np.full(3, 77, np.int32)
        lib = L.load()
        assert lib.tfr_ease_rank_items(m._h, None, 0, None, None, None, None, L.ptr_i32(out)) == L.OK and out.tolist() == [77] * 3
        assert lib.tfr_ease_topk(m._h, None, 0, 5, None, None, L.ptr_i32(out), None) == L.OK and out.tolist() == [77] * 3
        assert lib.tfr_ease_topk_lists(m._h, None, None, 0, 5, None, None, L.ptr_i32(out), None) == L.OK and out.tolist() == [77] * 3


def test_recommend_duplicates_and_crowd():
    ni = 300
    B = EC.constructed_weights(ni)
    indptr, items, nu, _ = EC.ladder(ni, seed=42)
    rs = np.random.RandomState(5)
    with T.EASE(nu, ni) as m:
        m.load((indptr, items))
        m.set_weights(B)
        crowd = rs.randint(0, nu, 3000).astype(np.int32)
        crowd[:4] = [9, 9, 20, 9]
        x = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
        got = m.recommend(crowd, 10, exclude=x)
        lists = IC.rows_of(indptr, items, crowd[:50])
        assert_same((got[0][:50], got[1][:50]), want_topk(lists, B, 10, lists), "the crowd's first 50")
        for u in (9, 20, int(crowd[2999])):
            alone = m.recommend(np.array([u], np.int32), 10, exclude=x)
            for q in np.flatnonzero(crowd == u):
                assert_same((got[0][q], got[1][q]), (alone[0][0], alone[1][0]), "user %d alone and at %d" % (u, q))


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------
def test_end_to_end_fit_scores_metrics_and_move():
    (indptr, items, nu, ni), tu, ti = EC.planted_case()
    assert (nu, ni) == (300, 150)
    lam = 5.0
    train = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
    g = R.gram(indptr, items, nu, ni, lam)
    p_ld = R.inverse_ld(g)
    cond = float(np.linalg.cond(g))
    assert cond <= EC.COND_MAX
    _, K = EC.error_constant()
    b64 = np.asarray(-p_ld / np.diag(p_ld)[None, :], np.float64)
    np.fill_diagonal(b64, 0.0)
    # the bound of a score.  |P_dev - P_ld| <= e = K eps cond max|P_ld| per entry (test 3), so through the division
    # |B_dev64 - B64|[i, j] <= db[i, j] = e (1 + |B64[i, j]|) / (P[j, j] - e); B rounds to float32 (2^-24 relative) and the
    # chain of |N(u)| - 1 float32 adds loses at most 2^-24 of the absolute sum each: (|N(u)| + 2) 2^-24 sum_i (|B64| + db),
    # plus sum_i db, over i in N(u).  The reference itself (long double rounded to float64) is exact beside these.
    e = K * R.EPS * cond * float(np.abs(p_ld).max())
    diag = np.diag(p_ld).astype(np.float64)
    assert (diag > 2 * e).all()
    db = e * (1.0 + np.abs(b64)) / (diag - e)[None, :]
    users = np.arange(nu, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    with T.EASE(nu, ni, regularization=lam) as m:
        m.fit(train)
        assert m.fit_ms > 0
        got_items, got_scores = m.recommend(users, ni)                         # k = the catalogue: every score, sorted
        B = m.weights()
        worst = 0.0
        for u, lst in enumerate(lists):
            assert sorted(got_items[u].tolist()) == list(range(ni))
            s = np.empty(ni, np.float64)
            s[got_items[u]] = got_scores[u]
            want = b64[lst].sum(axis=0)
            bound = (len(lst) + 2) * 2.0 ** -24 * (np.abs(b64[lst]) + db[lst]).sum(axis=0) + db[lst].sum(axis=0)
            worst = max(worst, float((np.abs(s - want) / bound).max()))
            assert (np.abs(s - want) <= bound).all(), u
        print("end to end: largest |score - X B64| / bound = %.3g" % worst)
        res = T.evaluate_ranking(m, tu, ti, exclude=train, ks=(10,))
        q_users = res["users"]
        want_ranks = np.concatenate([R.ranks(R.user_scores(lists[u], B), res["items"][res["indptr"][q]:res["indptr"][q + 1]], lists[u])
                                     for q, u in enumerate(q_users)])
        assert np.array_equal(res["ranks"], want_ranks)
        host = T.ranking_metrics(want_ranks, res["indptr"], ni - np.diff(indptr)[q_users], ks=(10,))
        for name in ("recall@10", "ndcg@10"):
            assert np.array_equal(res[name], host[name])
            assert res["mean"][name] == float(host[name].mean())
        assert res["mean"]["recall@10"] > 0.3                                  # the clusters are found: chance is 10 / 138
        x = csr_of(lists)
        with T.EASE(nu, ni) as b:                                              # a fitted model moves without a refit
            b.set_weights(B)
            assert np.array_equal(bits(b.weights()), bits(B))
            assert_same(b.recommend_lists(x, 20), m.recommend(users, 20, exclude=x), "lists on the second handle")
            b.load((indptr, items))
            b.set_weights(B)
            assert_same(b.recommend(users, 20, exclude=x), m.recommend(users, 20, exclude=x), "resident on the second handle")


# ---- 8. errors that need a handle (tests/test_ease_host.py has the ones that do not) -------------------------------------------
def test_argument_and_state_errors():
    lib = L.load()
    i64 = lambda *v: np.array(v, np.int64)
    i32 = lambda *v: np.array(v, np.int32)
    f64p = lambda a: a.ctypes.data_as(L._f64p)
    out = np.full(8, 77, np.int32)
    n = 6
    with T.EASE(3, n, regularization=1.0) as m:
        h = m._h
        u = i32(0, 1)
        buf64, buf32 = np.zeros((n, n)), np.zeros((n, n), np.float32)
        # before a load, a Gram matrix and weights
        assert lib.tfr_ease_gram(h) == L.ERR_STATE
        assert lib.tfr_ease_solve(h, 0, None) == L.ERR_STATE
        assert lib.tfr_ease_get_f64(h, 0, n, f64p(buf64)) == L.ERR_STATE
        assert lib.tfr_ease_get_weights(h, 0, n, L.ptr_f32(buf32)) == L.ERR_STATE
        assert lib.tfr_ease_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        assert lib.tfr_ease_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(1, 2)), None, None, L.ptr_i32(out)) == L.ERR_STATE
        assert lib.tfr_ease_topk_lists(h, L.ptr_i64(i64(0, 1)), L.ptr_i32(i32(1)), 1, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        # load: each refusal leaves the handle unloaded
        for indptr, items, code in [(i64(1, 2, 3, 4), i32(0, 1, 2, 3), L.ERR_ARG),         # does not start at 0
                                    (i64(0, 2, 1, 3), i32(0, 1, 2), L.ERR_ARG),            # decreases
                                    (i64(0, 2, 3, 3), i32(4, 2, 1), L.ERR_ARG),            # unsorted row
                                    (i64(0, 2, 3, 3), i32(2, 2, 1), L.ERR_ARG),            # repeated item
                                    (i64(0, 2, 3, 3), i32(2, 6, 1), L.ERR_OOB),            # id out of range
                                    (i64(0, 2, 3, 3), i32(-1, 2, 1), L.ERR_OOB)]:
            assert lib.tfr_ease_load(h, L.ptr_i64(indptr), L.ptr_i32(items)) == code
            assert lib.tfr_ease_gram(h) == L.ERR_STATE
        m.load((i64(0, 2, 4, 4), i32(0, 1, 1, 2)))
        assert lib.tfr_ease_solve(h, 0, None) == L.ERR_STATE                               # loaded, no Gram matrix yet
        assert lib.tfr_ease_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE       # loaded, not fitted
        assert lib.tfr_ease_gram(h) == L.OK
        assert lib.tfr_ease_get_f64(h, 0, n, f64p(buf64)) == L.OK and buf64[:3, :3].tolist() == [[2, 1, 0], [1, 3, 1], [0, 1, 2]]
        assert lib.tfr_ease_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE       # a Gram matrix is no fit
        assert lib.tfr_ease_get_f64(h, 4, 3, f64p(buf64)) == L.ERR_ARG                     # window past the items
        assert lib.tfr_ease_solve(h, 0, None) == L.OK
        assert lib.tfr_ease_get_f64(h, 0, n, f64p(buf64)) == L.ERR_STATE                   # the solve did not keep the inverse
        assert lib.tfr_ease_solve(h, 0, None) == L.ERR_STATE                               # and G is gone
        assert lib.tfr_ease_get_weights(h, 0, n, L.ptr_f32(buf32)) == L.OK
        # queries
        assert lib.tfr_ease_topk(h, L.ptr_i32(u), 2, 0, None, None, L.ptr_i32(out), None) == L.ERR_ARG
        assert lib.tfr_ease_topk(h, L.ptr_i32(u), 2, 257, None, None, L.ptr_i32(out), None) == L.ERR_ARG
        assert lib.tfr_ease_topk(h, L.ptr_i32(i32(0, 3)), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_OOB
        assert lib.tfr_ease_topk(h, L.ptr_i32(u), 2, 2, L.ptr_i64(i64(0, 2, 2)), L.ptr_i32(i32(3, 1)), L.ptr_i32(out), None) == L.ERR_ARG
        for indptr, items, code in [(i64(1, 2), i32(0, 1), L.ERR_ARG), (i64(0, 2), i32(3, 3), L.ERR_ARG),
                                    (i64(0, 2), i32(4, 1), L.ERR_ARG), (i64(0, 2), i32(1, 6), L.ERR_OOB)]:
            assert lib.tfr_ease_topk_lists(h, L.ptr_i64(indptr), L.ptr_i32(items), 1, 2, None, None, L.ptr_i32(out), None) == code
        assert lib.tfr_ease_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 2, 2)), L.ptr_i32(i32(2, 2)), None, None, L.ptr_i32(out)) == L.ERR_ARG
        assert lib.tfr_ease_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(2, 9)), None, None, L.ptr_i32(out)) == L.ERR_OOB
        assert out.tolist() == [77] * 8                                        # no refused call wrote anything
        # set_weights: values that are not finite, windows
        before = m.weights()
        bad = before.copy()
        bad[4, 1] = np.inf
        assert lib.tfr_ease_set_weights(h, 0, n, L.ptr_f32(bad)) == L.ERR_ARG
        bad[4, 1] = np.nan
        assert lib.tfr_ease_set_weights(h, 0, n, L.ptr_f32(bad)) == L.ERR_ARG
        assert lib.tfr_ease_set_weights(h, 4, 3, L.ptr_f32(before)) == L.ERR_ARG
        assert np.array_equal(bits(m.weights()), bits(before))                 # untouched
        row = np.full((1, n), 0.5, np.float32)
        assert lib.tfr_ease_set_weights(h, 2, 1, L.ptr_f32(row)) == L.OK       # a fitted model takes a window
        assert m.weights()[2].tolist() == [0.5] * n and np.array_equal(bits(m.weights()[3]), bits(before[3]))
        # a second load forgets Gram and weights
        m.build_gram()
        m.load((i64(0, 1, 2, 3), i32(0, 1, 2)))
        assert lib.tfr_ease_get_f64(h, 0, n, f64p(buf64)) == L.ERR_STATE
        assert lib.tfr_ease_get_weights(h, 0, n, L.ptr_f32(buf32)) == L.ERR_STATE
        assert lib.tfr_ease_solve(h, 0, None) == L.ERR_STATE
        assert lib.tfr_ease_set_weights(h, 0, 2, L.ptr_f32(before)) == L.ERR_STATE          # without weights: all rows at once
        assert lib.tfr_ease_set_weights(h, 0, n, L.ptr_f32(before)) == L.OK
        assert lib.tfr_ease_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.OK


# ---- 9. what EASE shares with ItemKNN (csrc/item_lists.h) ------------------------------------------------------------------------
def test_a_refused_load_leaves_a_fitted_model_serving():
    (indptr, items, nu, ni), _, _ = EC.planted_case()
    users = np.arange(0, nu, 5, dtype=np.int32)
    x = csr_of(IC.rows_of(indptr, items, users))
    with T.EASE(nu, ni, regularization=5.0) as m:
        m.fit((indptr, items), keep_inverse=True)
        before, B, P = m.recommend(users, 10, exclude=x), m.weights(), m.inverse()
        bad = items.copy()
        bad[-1] = ni                                                           # the last id of the last row: out of range
        assert L.load().tfr_ease_load(m._h, L.ptr_i64(indptr), L.ptr_i32(bad)) == L.ERR_OOB
        assert_same(m.recommend(users, 10, exclude=x), before, "after the refused load")
        assert np.array_equal(bits(m.weights()), bits(B)) and np.array_equal(bits64(m.inverse()), bits64(P))


def test_the_two_scoring_tails_agree():
    """ItemKNN's neighbour table and the dense weights that spell it out (tests/ease_cases.py twin_case: every sum exact in
    either order, tests/test_ease_host.py holds the two restatements to one set of keys): the two kernels accumulate in
    their own ways and then run the one shared tail, so items, scores and ranks are the same bits - over one slice there,
    over two here"""
    from tests import itemknn_ref as KR
    nb, sc, B = EC.twin_case()
    ni, K = B.shape[0], nb.shape[1]
    assert E.plan(ni, 10, 1, 1)["slices"] == 2
    indptr, items, nu, _ = EC.ladder(ni, seed=43)
    users = np.arange(nu, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    assert len(lists[0]) == 0                                                  # a query with an empty list
    rs = np.random.RandomState(7)
    targets = [np.sort(rs.choice(ni, 6, replace=False)).astype(np.int32) for _ in users]
    others = all_but(ni, lists[5])                                             # query 5: one target of its own list, three not
    targets[5] = np.sort(np.concatenate([lists[5][:1], others[[0, others.size // 2, -1]]])).astype(np.int32)
    with T.ItemKNN(nu, ni, K=K) as knn, T.EASE(nu, ni) as ease:
        knn.load((indptr, items))
        knn.set_neighbours(nb, sc)
        ease.load((indptr, items))
        ease.set_weights(B)
        for name, excl in exclusion_modes(lists, ni):
            x = None if excl is None else csr_of(excl)
            for k in (1, 10):
                got = knn.recommend(users, k, exclude=x)
                assert_same(ease.recommend(users, k, exclude=x), got, "recommend k=%d excl=%s" % (k, name))
                assert_same(got, want_topk(lists, B, k, excl), "both against the restatement k=%d excl=%s" % (k, name))
                assert_same(ease.recommend_lists((indptr, items), k, exclude=False if x is None else x), got, "lists k=%d" % k)
            ranks = knn.rank_items(users, csr_of(targets), exclude=x)
            assert np.array_equal(ease.rank_items(users, csr_of(targets), exclude=x), ranks), name
            want = np.concatenate([KR.ranks(KR.user_scores(lst, nb, sc, ni), t, () if excl is None else excl[q])
                                   for q, (lst, t) in enumerate(zip(lists, targets))])
            assert np.array_equal(ranks, want), name
            if name == "own":
                assert (ranks[30:34] == -1).sum() == 1                         # the excluded target
