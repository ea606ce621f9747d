"""UserKNN on the device against the NumPy restatement (tests/userknn_ref.py), bit for bit: neighbour ids equal, similarities,
user scores and ranks equal as bits.  The cases (tests/userknn_cases.py) are the smallest at which the kernels can go wrong:
user rows around the 64 row bounds a fit wave loads at once and the 256 of its block, user counts at the edges of the fit
slices and catalogues at the edges of the scoring slices (taken from tfr_uknn_plan), exact ties, 70 000 users for the strided
grid and the row chunks, neighbour lists of every row width the scoring kernel is compiled for, with scores whose sum depends
on the order of the adds, and query lists whose neighbours are found at query time."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import userknn as UK
from tests import itemknn_cases as IC
from tests import userknn_cases as UC
from tests import userknn_ref as R

pytestmark = pytest.mark.gpu

METRICS = [("cosine", 0.0), ("cosine", 2.5), ("jaccard", 0.0), ("jaccard", 2.5), ("count", 0.0)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    bad = np.flatnonzero((np.asarray(gi) != np.asarray(wi)).reshape(-1) | (bits(gs) != bits(ws)).reshape(-1))
    assert bad.size == 0, "%s: %d of %d slots differ, first at flat index %d: got (%d, %r) want (%d, %r)" % (
        what, bad.size, np.asarray(wi).size, bad[0], np.asarray(gi).reshape(-1)[bad[0]], np.asarray(gs).reshape(-1)[bad[0]],
        np.asarray(wi).reshape(-1)[bad[0]], np.asarray(ws).reshape(-1)[bad[0]])


def fitted_model(name, K, metric="cosine", shrink=0.0):
    indptr, items, nu, ni = UC.case(name)
    m = T.UserKNN(nu, ni, K=K, metric=metric, shrink=shrink)
    m.fit((indptr, items))
    return m


def check_fit(name, K, metric="cosine", shrink=0.0):
    with fitted_model(name, K, metric, shrink) as m:
        got = m.neighbours()
    assert_same(got, UC.fitted(name, K, metric, shrink), "%s K=%d %s shrink=%g" % (name, K, metric, shrink))
    return got


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


def want_topk(score_rows, k, excl=None):
    items = np.empty((len(score_rows), k), np.int32)
    scores = np.empty((len(score_rows), k), np.float32)
    for q, row in enumerate(score_rows):
        items[q], scores[q] = R.topk(row, k, () if excl is None else excl[q])
    return items, scores


# ---- fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,shrink", METRICS)
def test_fit_row_lengths_and_k(metric, shrink):
    """user rows of 0, 1, 63, 64, 65, 255, 256, 257 items, with an item every user has and without; K 256 over 130 users pads
    every row"""
    for K in (1, 10, 65, 256):
        nb, sc = check_fit("lengths", K, metric, shrink)
        assert (nb[0] == -1).all() and np.isneginf(sc[0]).all()                # user 0 has nothing
        assert (nb[1:, 0] >= 0).all()                                          # item 299 links all the others
        check_fit("sparse_lengths", K, metric, shrink)
    assert (nb[:, 129:] == -1).all()                                           # 130 users: at most 129 neighbours


def test_fit_counts_are_the_integers_of_xxt():
    for name in ("lengths", "sparse_lengths", "ties"):
        with fitted_model(name, 256, "count") as m:
            nb, sc = m.neighbours()
        indptr, items, nu, ni = UC.case(name)
        dense = R.cooccurrence(indptr, items, nu, ni)[0].toarray()
        for u in range(nu):
            kept = nb[u][nb[u] >= 0]
            assert sc[u][:kept.size].astype(np.int64).tolist() == dense[u, kept].tolist()
            others = np.setdiff1d(np.flatnonzero(dense[u]), [u])
            assert sorted(kept.tolist()) == others.tolist()                    # K = 256 keeps every co-rater


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_fit_user_count_at_the_slice_edges(extra):
    w = UC.w_fit()
    n_users = 2 * w + 3 if extra is None else w + extra
    assert UK.plan(n_users, 10, n_users, 0)["slices"] == (3 if extra is None else 2 if extra == 1 else 1)
    nb, _ = check_fit("edge:%d" % n_users, 10)
    assert (nb[[0, n_users - 1], 0] >= 0).all()                                # the first and the last user have co-raters


@pytest.mark.parametrize("metric,shrink", METRICS)
def test_fit_exact_ties_go_by_id(metric, shrink):
    nb, sc = check_fit("ties", 10, metric, shrink)
    assert nb[80, :10].tolist() == [75, 76, 77, 78, 79, 81, 82, 83, 84, 85]    # block 3: all tie, lowest ids first, not itself
    assert len(set(bits(sc[80]).tolist())) == 1


def test_fit_70000_users():
    p = UK.plan(70000, 10, 70000, 0)
    assert p["chunk"] < 70000 and p["slices"] == 5
    check_fit("big", 10)


def test_fit_again_and_after_another_load():
    a = UC.case("lengths")
    b = UC.case("sparse_lengths")
    assert a[2:] == b[2:]
    nu, ni = a[2], a[3]
    with T.UserKNN(nu, ni, K=10) as m:
        first = m.fit(a[:2]).neighbours()
        assert_same(first, UC.fitted("lengths", 10), "the first fit")
        assert_same(m.fit().neighbours(), first, "a repeated fit")
        m.load(b[:2])
        with pytest.raises(T.TfrError) as e:
            m.neighbours()                                                     # the load forgot the lists
        assert e.value.code == L.ERR_STATE
        assert_same(m.fit().neighbours(), UC.fitted("sparse_lengths", 10), "a fit after a second load")
        assert m.fit_ms > 0


@pytest.mark.parametrize("name", ["lengths", "ties", "edge:16385"])
def test_fit_is_itemknn_of_the_transpose(name):
    indptr, items, nu, ni = UC.case(name)
    tp, ti, tnu, tni = UC.transpose((indptr, items, nu, ni))
    for K, metric, shrink in ((10, "cosine", 0.0), (65, "jaccard", 2.5)):
        with T.UserKNN(nu, ni, K=K, metric=metric, shrink=shrink) as um, T.ItemKNN(tnu, tni, K=K, metric=metric, shrink=shrink) as im:
            assert_same(um.fit((indptr, items)).neighbours(), im.fit((tp, ti)).neighbours(), "%s K=%d" % (name, K))


# ---- scoring -------------------------------------------------------------------------------------------------------------
QUERIES = np.array([0, 1, 2, 3, 4, 5, 7, 8, 9, 13, 13, 20, 299] + list(range(30, 290, 13)), np.int32)


@functools.lru_cache(maxsize=None)
def constructed(K):
    """(nb, sc, the float32 score rows of QUERIES) of the constructed lists over the scoring case"""
    indptr, items, nu, ni = UC.case("scoring")
    nb, sc = UC.constructed_lists(nu, K)
    return nb, sc, [R.user_scores(nb[u], sc[u], indptr, items, ni) for u in QUERIES]


@pytest.mark.parametrize("K", [7, 64, 65, 128, 130, 256])
def test_scores_of_constructed_lists_at_every_row_width(K):
    """K on both sides of the three ways a wave covers a neighbour row; mixed signs and magnitudes far apart aimed at item 6
    (rows 7 and 8), rows with fewer than K neighbours and none (row 9), an empty neighbour and a padding slot in the middle
    (row 13), neighbour rows of 1, 63, 64, 65 and 200 items; k 1, 10, 256; exclusions none, own, all but two"""
    indptr, items, nu, ni = UC.case("scoring")
    assert np.diff(indptr)[:6].tolist() == [0, 1, 63, 64, 65, 200]
    nb, sc, rows = constructed(K)
    lists = IC.rows_of(indptr, items, QUERIES)
    with T.UserKNN(nu, ni, K=K) as m:
        m.load((indptr, items))
        m.set_neighbours(nb, sc)
        assert_same(m.neighbours(), (nb, sc), "set then get")
        for k in (1, 10, 256):
            for name, excl in exclusion_modes(lists, ni):
                x = None if excl is None else csr_of(excl)
                got = m.recommend(QUERIES, k, exclude=x)
                assert_same(got, want_topk(rows, k, excl), "K=%d k=%d excl=%s" % (K, k, name))
                if name == "all but two" and k > 2:
                    assert (got[0][:, 2:] == -1).all() and np.isneginf(got[1][:, 2:]).all()
        # the whole score row of users 7 and 8, by asking for every item: item 6 carries the order-dependent sums
        for q in (6, 7):
            full = m.recommend(QUERIES[q:q + 1], 256, exclude=(np.array([0, ni - 256], np.int64), all_but(ni, np.arange(256))))
            order = np.argsort(full[0][0])
            assert full[0][0][order].tolist() == list(range(256))
            assert np.array_equal(bits(full[1][0][order]), bits(rows[q][:256]))
        assert bits(rows[6])[6] == 0                                           # (1 + 1e8) - 1e8
        # nobody to ask: every score +0, the k lowest eligible ids
        got = m.recommend(np.array([9], np.int32), 10)
        assert got[0].tolist() == [list(range(10))] and bits(got[1]).tolist() == [[0] * 10]
        got = m.recommend(np.array([9], np.int32), 3, exclude=(np.array([0, 3], np.int64), np.array([0, 1, 3], np.int32)))
        assert got[0].tolist() == [[2, 4, 5]] and bits(got[1]).tolist() == [[0] * 3]
        assert np.array_equal(m.recommend(QUERIES, 10, return_scores=False), m.recommend(QUERIES, 10)[0])
        ids, sims = m.similar_users([8, 13, 0], min(5, K))
        assert np.array_equal(ids, nb[[8, 13, 0], :5]) and np.array_equal(bits(sims), bits(sc[[8, 13, 0], :5]))


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_scores_and_ranks_at_the_slice_edges(extra):
    """catalogues at the scoring slice width: neighbour rows that straddle each edge, a neighbour with nothing in a slice,
    targets on both sides of every edge and the last item"""
    w = UC.w_score()
    ni = 2 * w + 3 if extra is None else w + extra
    assert UK.plan(ni, 10, 1, 1)["slices"] == (3 if extra is None else 2 if extra == 1 else 1)
    indptr, items, nu, _ = UC.case("score_edge:%d" % ni)
    nb, sc = IC.constructed_lists(nu, 10, seed=37)
    nb[5], sc[5] = -1, -np.inf
    nb[5, :4], sc[5, :4] = [1, 2, 3, 4], [0.5, -0.25, 2.0, 1.0]                # the straddling, the far and the near neighbour, the marks
    users = np.arange(nu, dtype=np.int32)
    rows = [R.user_scores(nb[u], sc[u], indptr, items, ni) for u in users]
    lists = IC.rows_of(indptr, items, users)
    tg = np.unique([c for c in (0, w - 1, w, w + 1, 2 * w - 1, 2 * w, ni - 1) if c < ni]).astype(np.int32)
    tp = np.arange(users.size + 1, dtype=np.int64) * tg.size
    with T.UserKNN(nu, ni, K=10) as m:
        m.load((indptr, items))
        m.set_neighbours(nb, sc)
        for k in (10, 256):
            assert_same(m.recommend(users, k, exclude=csr_of(lists)), want_topk(rows, k, lists), "ni=%d k=%d" % (ni, k))
        assert_same(m.recommend(users, 10), want_topk(rows, 10), "ni=%d no exclusion" % ni)
        got = m.rank_items(users, (tp, np.tile(tg, users.size)), exclude=csr_of(lists))
        want = np.concatenate([R.ranks(rows[u], tg, lists[u]) for u in users])
        assert np.array_equal(got, want)


def test_scores_with_count_are_the_integers_of_the_product():
    """metric count, K >= every neighbour count: score(u, .) = the row of (X X^T - diag) X, exact in float32"""
    indptr, items, nu, ni = UC.case("full_user")
    x = R.IR.pattern(indptr, items, nu, ni)
    c = (x @ x.T).toarray()
    np.fill_diagonal(c, 0)
    want = c @ x.toarray()
    assert want.max() < 2 ** 24
    with fitted_model("full_user", 256, "count") as m:
        got_i, got_s = m.recommend(np.arange(nu, dtype=np.int32), ni)
    for u in range(nu):
        order = np.argsort(got_i[u])
        assert got_i[u][order].tolist() == list(range(ni))
        assert got_s[u][order].astype(np.int64).tolist() == want[u].tolist()


def test_recommend_duplicates_and_crowd():
    indptr, items, nu, ni = UC.case("lengths")
    row = UC.scores_of("lengths", 10)
    rs = np.random.RandomState(5)
    with fitted_model("lengths", 10) as m:
        crowd = rs.randint(0, nu, 3000).astype(np.int32)
        crowd[:4] = [9, 9, 100, 9]
        x = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
        got = m.recommend(crowd, 10, exclude=x)
        lists = IC.rows_of(indptr, items, crowd[:50])
        assert_same((got[0][:50], got[1][:50]), want_topk([row(int(u)) for u in crowd[:50]], 10, lists), "the crowd's first 50")
        alone = m.recommend(np.arange(nu, dtype=np.int32), 10, exclude=x)
        one = m.recommend(np.array([9], np.int32), 10, exclude=x)
        assert_same((alone[0][9], alone[1][9]), (one[0][0], one[1][0]), "user 9 alone")
        assert_same(got, (alone[0][crowd], alone[1][crowd]), "each of the crowd as asked alone")


# ---- lists ---------------------------------------------------------------------------------------------------------------
def want_lists(case, lists, K, metric, shrink, k, excl=None):
    indptr, items, nu, ni = case
    nbs = [R.list_neighbours(lst, indptr, items, nu, ni, K, metric, shrink) for lst in lists]
    rows = [R.user_scores(nb, sc, indptr, items, ni) for nb, sc in nbs]
    return nbs, want_topk(rows, k, excl)


@pytest.mark.parametrize("metric,shrink", METRICS)
def test_lists_of_every_length_on_an_unfitted_handle(metric, shrink):
    """query lists of 0, 1, 63, 64, 65 and 257 items; a list equal to a resident row; a list sharing nothing; exclude True,
    False and a CSR; no fit, and set lists are ignored"""
    case = UC.case("scoring")
    indptr, items, nu, ni = case
    rs = np.random.RandomState(41)
    lists = [np.sort(rs.choice(ni - 1, n, replace=False)).astype(np.int32) for n in (0, 1, 63, 64, 65, 257)]
    lists += [items[indptr[5]:indptr[6]], np.array([ni - 1], np.int32), items[indptr[40]:indptr[41]]]
    K = 20
    with T.UserKNN(nu, ni, K=K, metric=metric, shrink=shrink) as m:
        m.load((indptr, items))
        for k in (1, 10, 256):
            nbs, want = want_lists(case, lists, K, metric, shrink, k, lists)
            assert_same(m.recommend_lists(csr_of(lists), k), want, "exclude=True k=%d" % k)
            assert_same(m.recommend_lists(csr_of(lists), k, exclude=csr_of(lists)), want, "exclude=own CSR k=%d" % k)
            assert_same(m.recommend_lists(csr_of(lists), k, exclude=False), want_lists(case, lists, K, metric, shrink, k)[1],
                        "exclude=False k=%d" % k)
        assert nbs[6][0][0] == 5                                               # the resident row's owner comes first
        if (metric, shrink) == ("cosine", 0.0):
            assert bits(nbs[6][1])[0] == 0x3f800000
        assert (nbs[7][0] == -1).all() and (nbs[0][0] == -1).all()             # nobody shares the last item, or nothing
        got = m.recommend_lists(csr_of(lists[7:8]), 10, exclude=False)
        assert got[0].tolist() == [list(range(10))] and bits(got[1]).tolist() == [[0] * 10]
        with pytest.raises(T.TfrError) as e:
            m.recommend(np.array([0], np.int32), 5)                            # still no lists of its own
        assert e.value.code == L.ERR_STATE
        # set lists do not reach the answer
        nb, sc = UC.constructed_lists(nu, K)
        m.set_neighbours(nb, sc)
        assert_same(m.recommend_lists(csr_of(lists), 10), want_lists(case, lists, K, metric, shrink, 10, lists)[1], "after set_neighbours")


def test_lists_find_the_resident_row_first_through_the_device_lists():
    """the list path's neighbours themselves, read back through a fitted twin: a list equal to user u's row has u's fitted
    neighbours behind u itself at 1.0"""
    case = UC.case("lengths")
    indptr, items, nu, ni = case
    lists = IC.rows_of(indptr, items, [5, 9, 64])
    nbs, want = want_lists(case, lists, 10, "cosine", 0.0, 10)
    fnb, fsc = UC.fitted("lengths", 10)
    for q, u in enumerate((5, 9, 64)):
        assert nbs[q][0][0] == u and bits(nbs[q][1])[0] == 0x3f800000
        assert nbs[q][0][1:].tolist() == fnb[u][:9].tolist() and bits(nbs[q][1][1:]).tolist() == bits(fsc[u][:9]).tolist()
    with fitted_model("lengths", 10) as m:
        assert_same(m.recommend_lists(csr_of(lists), 10, exclude=False), want, "lists equal to resident rows")


def test_lists_ties_go_by_id():
    case = UC.case("ties")
    indptr, items, nu, ni = case
    lists = [items[indptr[80]:indptr[81]], items[indptr[3]:indptr[4]]]
    nbs, want = want_lists(case, lists, 10, "cosine", 0.0, 10, lists)
    assert nbs[0][0].tolist() == list(range(75, 85)) and set(bits(nbs[0][1]).tolist()) == {0x3f800000}
    with T.UserKNN(nu, ni, K=10) as m:
        m.load((indptr, items))
        assert_same(m.recommend_lists(csr_of(lists), 10), want, "ties")


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_lists_resident_users_at_the_slice_edges(extra):
    w = UC.w_lists()
    nu = 2 * w + 3 if extra is None else w + extra
    assert UK.plan(nu, 10, 1, 2)["slices"] == (3 if extra is None else 2 if extra == 1 else 1)
    case = UC.case("edge:%d" % nu)
    indptr, items, _, ni = case
    marks = [u for u in (0, w - 1, w, w + 1, 2 * w - 1, 2 * w, nu - 1) if u < nu]
    lists = IC.rows_of(indptr, items, marks) + [np.arange(ni, dtype=np.int32)]   # and a list that meets every user with a row
    nbs, want = want_lists(case, lists, 10, "jaccard", 0.0, 10, lists)
    assert all(nbs[q][0][0] >= 0 for q in range(len(lists)))
    with T.UserKNN(nu, ni, K=10, metric="jaccard") as m:
        m.load((indptr, items))
        assert_same(m.recommend_lists(csr_of(lists), 10), want, "nu=%d" % nu)


# ---- rank ----------------------------------------------------------------------------------------------------------------
def test_rank_items_against_the_restatement_and_recommend():
    indptr, items, nu, ni = UC.case("lengths")
    row = UC.scores_of("lengths", 10)
    rs = np.random.RandomState(6)
    users = np.array([0, 5, 5, 17, 129, 120, 64], np.int32)
    lists = IC.rows_of(indptr, items, users)
    targets = [np.sort(rs.choice(ni, n, replace=False)).astype(np.int32) for n in (ni, 0, 70, 3, 1, 0, 12)]
    targets[3] = np.sort(np.concatenate([lists[3][:2], all_but(ni, lists[3])[:1]])).astype(np.int32)    # two excluded targets
    with fitted_model("lengths", 10) as m:
        for name, excl in exclusion_modes(lists, ni):
            x = None if excl is None else csr_of(excl)
            got = m.rank_items(users, csr_of(targets), exclude=x)
            want = np.concatenate([R.ranks(row(int(u)), t, () if excl is None else excl[q]) for q, (u, t) in enumerate(zip(users, targets))])
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
        # rows without targets and n = 0 write nothing
        none = m.rank_items(users, (np.zeros(users.size + 1, np.int64), np.zeros(0, np.int32)))
        assert none.size == 0
        assert m.rank_items(np.zeros(0, np.int32), (np.zeros(1, np.int64), np.zeros(0, np.int32))).size == 0
        out = np.full(3, 77, np.int32)
        lib = L.load()
        assert lib.tfr_uknn_rank_items(m._h, None, 0, None, None, None, None, L.ptr_i32(out)) == L.OK and out.tolist() == [77] * 3
        assert lib.tfr_uknn_rank_items(m._h, L.ptr_i32(users), users.size, L.ptr_i64(np.zeros(users.size + 1, np.int64)), None, None, None,
                                       L.ptr_i32(out)) == L.OK and out.tolist() == [77] * 3
        assert lib.tfr_uknn_topk(m._h, None, 0, 5, None, None, L.ptr_i32(out), None) == L.OK and out.tolist() == [77] * 3
        assert lib.tfr_uknn_topk_lists(m._h, None, None, 0, 5, None, None, L.ptr_i32(out), None) == L.OK and out.tolist() == [77] * 3


def test_evaluate_ranking_takes_the_model():
    (indptr, items, nu, ni), tu, ti = IC.planted_case()
    assert (nu, ni) == (300, 200)
    train = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
    nb, sc = R.fit(indptr, items, nu, ni, 20, "cosine", 0.0)
    with T.UserKNN(nu, ni, K=20) as m:
        m.fit(train)
        assert_same(m.neighbours(), (nb, sc), "planted fit")
        res = T.evaluate_ranking(m, tu, ti, exclude=train, ks=(10,))
    users = res["users"]
    lists = IC.rows_of(indptr, items, users)
    want = np.concatenate([R.ranks(R.user_scores(nb[u], sc[u], indptr, items, ni), res["items"][res["indptr"][q]:res["indptr"][q + 1]], lists[q])
                           for q, u in enumerate(users)])
    assert np.array_equal(res["ranks"], want)
    host = T.ranking_metrics(want, res["indptr"], ni - np.diff(indptr)[users], ks=(10,))
    for name in ("recall@10", "ndcg@10"):
        assert np.array_equal(res[name], host[name])
        assert res["mean"][name] == float(host[name].mean())
    assert res["mean"]["recall@10"] > 0.15                                     # the restatement gives 0.334; chance is 10 / 187


# ---- errors and state ----------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    lib = L.load()
    i64 = lambda *v: np.array(v, np.int64)
    i32 = lambda *v: np.array(v, np.int32)
    out = np.full(8, 77, np.int32)
    fout = np.full(8, 77, np.float32)
    o, fo = L.ptr_i32(out), L.ptr_f32(fout)
    with T.UserKNN(6, 4, K=2) as m:
        h = m._h
        u = i32(0, 1)
        lp, li = L.ptr_i64(i64(0, 1)), L.ptr_i32(i32(1))
        # before a load and before a fit
        assert lib.tfr_uknn_fit(h, None) == L.ERR_STATE
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 2, None, None, o, fo) == L.ERR_STATE
        assert lib.tfr_uknn_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(1, 2)), None, None, o) == L.ERR_STATE
        assert lib.tfr_uknn_get_neighbours(h, 0, 6, o, fo) == L.ERR_STATE
        assert lib.tfr_uknn_topk_lists(h, lp, li, 1, 2, None, None, o, fo) == L.ERR_STATE
        assert b"tfr_uknn_load" in lib.tfr_uknn_last_error()
        # load: each refusal leaves the handle unloaded
        for indptr, items, code in [(i64(1, 2, 3, 4, 4, 4, 4), i32(0, 1, 2, 3), L.ERR_ARG),         # does not start at 0
                                    (i64(0, 2, 1, 3, 3, 3, 3), i32(0, 1, 2), L.ERR_ARG),            # decreases
                                    (i64(0, 2, 3, 3, 3, 3, 3), i32(3, 2, 1), L.ERR_ARG),            # unsorted row
                                    (i64(0, 2, 3, 3, 3, 3, 3), i32(2, 2, 1), L.ERR_ARG),            # repeated item
                                    (i64(0, 2, 3, 3, 3, 3, 3), i32(2, 4, 1), L.ERR_OOB),            # id out of range
                                    (i64(0, 2, 3, 3, 3, 3, 3), i32(-1, 2, 1), L.ERR_OOB)]:
            assert lib.tfr_uknn_load(h, L.ptr_i64(indptr), L.ptr_i32(items)) == code
            assert lib.tfr_uknn_fit(h, None) == L.ERR_STATE
        # set_neighbours needs no load; the scoring of users does
        nb = np.full((6, 2), -1, np.int32)
        nb[:, 0] = [1, 2, 3, 4, 5, 0]
        ok_sc = np.zeros((6, 2), np.float32)
        assert lib.tfr_uknn_set_neighbours(h, 0, 6, L.ptr_i32(nb), L.ptr_f32(ok_sc)) == L.OK
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 2, None, None, o, fo) == L.ERR_STATE
        assert lib.tfr_uknn_topk_lists(h, lp, li, 1, 2, None, None, o, fo) == L.ERR_STATE          # lists need the load, not lists
        # rows {0,1}, {1,2}, {}, {3}, {}, {}: users 0 and 1 share item 1
        m.load((i64(0, 2, 4, 4, 5, 5, 5), i32(0, 1, 1, 2, 3)))
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 2, None, None, o, fo) == L.ERR_STATE            # loaded, not fitted
        assert lib.tfr_uknn_get_neighbours(h, 0, 6, o, fo) == L.ERR_STATE
        assert out.tolist() == [77] * 8 and fout.tolist() == [77] * 8
        m.fit()
        want_nb = [[1, -1], [0, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
        assert m.neighbours()[0].tolist() == want_nb
        # queries
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 0, None, None, o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 257, None, None, o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), -1, 2, None, None, o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk(h, None, 2, 2, None, None, o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 2, None, None, None, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk(h, L.ptr_i32(i32(0, 6)), 2, 2, None, None, o, fo) == L.ERR_OOB
        assert lib.tfr_uknn_topk(h, L.ptr_i32(i32(0, -1)), 2, 2, None, None, o, fo) == L.ERR_OOB
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 2, L.ptr_i64(i64(0, 2, 2)), L.ptr_i32(i32(3, 1)), o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk(h, L.ptr_i32(u), 2, 2, L.ptr_i64(i64(0, 2, 2)), L.ptr_i32(i32(1, 4)), o, fo) == L.ERR_OOB
        assert lib.tfr_uknn_topk_lists(h, lp, li, 1, 0, None, None, o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk_lists(h, lp, li, 1, 257, None, None, o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk_lists(h, lp, li, -1, 2, None, None, o, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk_lists(h, lp, li, 1, 2, None, None, None, fo) == L.ERR_ARG
        assert lib.tfr_uknn_topk_lists(h, lp, li, 1, 2, L.ptr_i64(i64(0, 2)), L.ptr_i32(i32(3, 1)), o, fo) == L.ERR_ARG
        for indptr, items, code in [(i64(1, 2), i32(0, 1), L.ERR_ARG), (i64(0, 2), i32(3, 3), L.ERR_ARG),
                                    (i64(0, 2), i32(3, 1), L.ERR_ARG), (i64(0, 2), i32(1, 4), L.ERR_OOB)]:
            assert lib.tfr_uknn_topk_lists(h, L.ptr_i64(indptr), L.ptr_i32(items), 1, 2, None, None, o, fo) == code
        assert lib.tfr_uknn_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 2, 2)), L.ptr_i32(i32(2, 2)), None, None, o) == L.ERR_ARG
        assert lib.tfr_uknn_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(2, 9)), None, None, o) == L.ERR_OOB
        assert lib.tfr_uknn_rank_items(h, L.ptr_i32(i32(0, 6)), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(2, 3)), None, None, o) == L.ERR_OOB
        assert lib.tfr_uknn_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(2, 3)), None, None, None) == L.ERR_ARG
        assert lib.tfr_uknn_get_neighbours(h, 4, 3, o, fo) == L.ERR_ARG                                # window past the users
        assert lib.tfr_uknn_get_neighbours(h, -1, 1, o, fo) == L.ERR_ARG
        assert b"6 users" in lib.tfr_uknn_last_error()
        assert out.tolist() == [77] * 8 and fout.tolist() == [77] * 8          # no refused call wrote anything
        # set_neighbours
        for bad, code in [((0, 0, 0), L.ERR_ARG),                              # row 0 lists itself
                          ((1, 0, 6), L.ERR_OOB), ((1, 0, -2), L.ERR_OOB),
                          ((2, 0, 4), None)]:
            nb = np.full((6, 2), -1, np.int32)
            nb[:, 0] = [1, 2, 3, 4, 5, 0]
            nb[bad[0], bad[1]] = bad[2]
            if code is None:
                nb[2, 1] = 4                                                   # row 2 repeats user 4
                code = L.ERR_ARG
            assert lib.tfr_uknn_set_neighbours(h, 0, 6, L.ptr_i32(nb), L.ptr_f32(ok_sc)) == code
        nb = np.full((6, 2), -1, np.int32)
        nb[:, 0] = [1, 2, 3, 4, 5, 0]
        for bad in (np.nan, np.inf):
            bad_sc = ok_sc.copy()
            bad_sc[4, 0] = bad
            assert lib.tfr_uknn_set_neighbours(h, 0, 6, L.ptr_i32(nb), L.ptr_f32(bad_sc)) == L.ERR_ARG
        assert lib.tfr_uknn_set_neighbours(h, 4, 3, L.ptr_i32(nb), L.ptr_f32(ok_sc)) == L.ERR_ARG   # window past the users
        assert lib.tfr_uknn_set_neighbours(h, 0, 6, None, L.ptr_f32(ok_sc)) == L.ERR_ARG
        assert lib.tfr_uknn_set_neighbours(h, 0, 6, L.ptr_i32(nb), None) == L.ERR_ARG
        m._nb = None                                                           # read the device's lists again
        assert m.neighbours()[0].tolist() == want_nb                           # untouched
        # a window of rows: the others keep what they hold
        assert lib.tfr_uknn_set_neighbours(h, 2, 1, L.ptr_i32(i32(5, 0)), L.ptr_f32(np.array([0.5, 0.25], np.float32))) == L.OK
        m._nb = None
        assert m.neighbours()[0].tolist() == want_nb[:2] + [[5, 0]] + want_nb[3:]
        with pytest.raises(ValueError):
            m.set_neighbours(np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32))             # [item_num, K] is not the shape


def test_a_refused_load_leaves_a_fitted_model_serving():
    indptr, items, nu, ni = UC.case("lengths")
    users = np.arange(0, nu, 5, dtype=np.int32)
    x = csr_of(IC.rows_of(indptr, items, users))
    with fitted_model("lengths", 10) as m:
        before = m.recommend(users, 10, exclude=x)
        before_l = m.recommend_lists(x, 10)
        bad = items.copy()
        bad[-1] = ni                                                           # the last id of the last row: out of range
        assert L.load().tfr_uknn_load(m._h, L.ptr_i64(indptr), L.ptr_i32(bad)) == L.ERR_OOB
        assert_same(m.recommend(users, 10, exclude=x), before, "after the refused load")
        assert_same(m.recommend_lists(x, 10), before_l, "lists after the refused load")
        assert_same(m.neighbours(), UC.fitted("lengths", 10), "the lists after the refused load")


def test_set_neighbours_on_a_second_handle_serves_as_the_first():
    indptr, items, nu, ni = UC.case("lengths")
    users = np.arange(0, nu, 7, dtype=np.int32)
    x = csr_of(IC.rows_of(indptr, items, users))
    with fitted_model("lengths", 65, "jaccard", 2.5) as a, T.UserKNN(nu, ni, K=65, metric="jaccard", shrink=2.5) as b:
        nb, sc = a.neighbours()
        b.load((indptr, items))
        b.set_neighbours(nb, sc)
        assert_same(b.neighbours(), (nb, sc), "the lists")
        assert_same(b.recommend(users, 20, exclude=x), a.recommend(users, 20, exclude=x), "resident on the second handle")
        assert_same(b.recommend_lists(x, 20), a.recommend_lists(x, 20), "lists on the second handle")
        assert np.array_equal(b.rank_items(users, x), a.rank_items(users, x))
        ids, sims = a.similar_users([3, 8, 0], 5)
        assert np.array_equal(ids, nb[[3, 8, 0], :5]) and np.array_equal(bits(sims), bits(sc[[3, 8, 0], :5]))
