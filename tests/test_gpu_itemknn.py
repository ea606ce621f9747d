"""ItemKNN on the device against the NumPy restatement (tests/itemknn_ref.py), bit for bit: neighbour ids equal, similarities,
user scores and ranks equal as bits.  The cases (tests/itemknn_cases.py) are the smallest at which the kernels can go wrong:
list lengths around the 64 row bounds a fit wave loads at once and the 256 of its block, catalogues at the edges of the fit
and scoring slices (taken from tfr_knn_plan), exact ties, a staircase that forces the queue's sort-cut, 70 000 items for the
strided grid and the row chunks, query lists around the scoring look-ahead."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import itemknn as IK
from tests import itemknn_cases as IC
from tests import itemknn_ref as R

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
    indptr, items, nu, ni = IC.case(name)
    m = T.ItemKNN(nu, ni, K=K, metric=metric, shrink=shrink)
    m.fit((indptr, items))
    return m


def check_fit(name, K, metric, shrink):
    with fitted_model(name, K, metric, shrink) as m:
        got = m.neighbours()
    assert_same(got, IC.fitted(name, K, metric, shrink), "%s K=%d %s shrink=%g" % (name, K, metric, shrink))
    return got


# ---- fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,shrink", METRICS)
def test_fit_list_lengths_and_k(metric, shrink):
    """item lists of 0, 1, 63, 64, 65, 255, 256, 257 users, an item every user has, a user who has every item; K 256 over
    130 and 90 items pads every row"""
    for K in (1, 10, 64, 65, 256):
        nb, sc = check_fit("lengths", K, metric, shrink)
        assert (nb[0] == -1).all() and np.isneginf(sc[0]).all()                # nobody has item 0
        check_fit("full_user", K, metric, shrink)
    assert (nb[:, 129:] == -1).all()                                           # 130 items: at most 129 neighbours


def test_fit_counts_are_the_integers_of_xtx():
    for name in ("lengths", "full_user", "ties"):
        with fitted_model(name, 256, "count") as m:
            nb, sc = m.neighbours()
        c, n = IC.counts(name)
        dense = c.toarray()
        for i in range(n.size):
            kept = nb[i][nb[i] >= 0]
            assert sc[i][:kept.size].astype(np.int64).tolist() == dense[i, kept].tolist()
            others = np.setdiff1d(np.flatnonzero(dense[i]), [i])
            assert sorted(kept.tolist()) == others.tolist()                    # K = 256 keeps every co-rated item


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_fit_catalogue_at_the_slice_edges(extra):
    w = IC.w_fit()
    n_items = 2 * w + 3 if extra is None else w + extra
    assert IK.plan(n_items, 10, n_items, 0)["slices"] == (3 if extra is None else 2 if extra == 1 else 1)
    check_fit("edge:%d" % n_items, 10, "cosine", 0.0)


@pytest.mark.parametrize("metric,shrink", METRICS)
def test_fit_exact_ties_go_by_id(metric, shrink):
    nb, sc = check_fit("ties", 10, metric, shrink)
    assert nb[80, :10].tolist() == [75, 76, 77, 78, 79, 81, 82, 83, 84, 85]    # block 3: all tie, lowest ids first, not itself
    assert len(set(bits(sc[80]).tolist())) == 1


@pytest.mark.parametrize("K", [10, 200])
@pytest.mark.parametrize("metric", ["cosine", "jaccard", "count"])
def test_fit_rising_scores_sort_cut_the_queue(metric, K):
    """the staircase: row 0's similarities rise along the catalogue, so each 64 columns a wave scans beat all it kept"""
    nb, sc = check_fit("staircase", K, metric, 0.0)
    n_items = IC.case("staircase")[3]
    assert nb[0, :64].tolist() == list(range(n_items - 64, n_items))[:K]       # the best are the last step, by id


def test_fit_70000_items():
    p = IK.plan(70000, 10, 70000, 0)
    assert p["chunk"] < 70000 and p["slices"] == 5
    check_fit("big", 10, "cosine", 0.0)


def test_fit_again_and_after_another_load():
    a = IC.case("lengths")
    b = IC.case("full_user")
    nu, ni = max(a[2], b[2]), max(a[3], b[3])

    def padded(c):
        indptr = np.concatenate([c[0], np.full(nu - c[2], c[0][-1], np.int64)])
        return indptr, c[1]
    with T.ItemKNN(nu, ni, K=10) as fresh:
        want = fresh.fit(padded(b)).neighbours()
    with T.ItemKNN(nu, ni, K=10) as m:
        first = m.fit(padded(a)).neighbours()
        assert_same(m.fit().neighbours(), first, "a repeated fit")
        m.load(padded(b))
        with pytest.raises(T.TfrError) as e:
            m.neighbours()                                                     # the load forgot the lists
        assert e.value.code == L.ERR_STATE
        assert_same(m.fit().neighbours(), want, "a fit after a second load")
        assert (np.asarray(first[0]) != np.asarray(want[0])).any()


# ---- recommend -----------------------------------------------------------------------------------------------------------
def ladder(n_items, ahead, seed=21):
    """query lists of 0, 1, ahead - 1, ahead, ahead + 1, 2 ahead, 2 ahead + 1 and 40 items, several of each"""
    rs = np.random.RandomState(seed)
    lens = [0, 1, ahead - 1, ahead, ahead + 1, 2 * ahead, 2 * ahead + 1, 40] * 3
    return IC.csr_of_rows([rs.choice(n_items, n, replace=False) for n in lens], n_items)


def want_topk(lists, nb, sc, n_items, k, excl=None):
    items = np.empty((len(lists), k), np.int32)
    scores = np.empty((len(lists), k), np.float32)
    for q, lst in enumerate(lists):
        items[q], scores[q] = R.topk(R.user_scores(lst, nb, sc, n_items), k, () if excl is None else excl[q])
    return items, scores


def all_but(n_items, keep):
    return np.setdiff1d(np.arange(n_items, dtype=np.int32), keep).astype(np.int32)


def exclusion_modes(lists, n_items):
    """(name, per-query exclusion lists or None): none, the own list, everything but two items (so k pads)"""
    yield "none", None
    yield "own", lists
    yield "all but two", [all_but(n_items, [q % n_items, (3 * q + 7) % n_items]) for q in range(len(lists))]


def csr_of(lists):
    p = np.zeros(len(lists) + 1, np.int64)
    p[1:] = np.cumsum([len(x) for x in lists])
    return p, (np.concatenate(lists).astype(np.int32) if len(lists) else np.zeros(0, np.int32))


@pytest.mark.parametrize("source", ["fitted", "constructed"])
def test_recommend_resident_users_and_lists(source):
    ahead = IK.plan(130, 10, 1, 1)["ahead"]
    indptr, items, nu, ni = ladder(130, ahead)
    with T.ItemKNN(nu, ni, K=10) as m:
        if source == "fitted":
            nb, sc = m.fit((indptr, items)).neighbours()
            assert_same((nb, sc), R.fit(*R.cooccurrence(indptr, items, nu, ni), 10, "cosine", 0.0), "ladder fit")
        else:
            m.load((indptr, items))
            nb, sc = IC.constructed_lists(ni, 10)
            m.set_neighbours(nb, sc)
            assert_same(m.neighbours(), (nb, sc), "set then get")
        users = np.arange(nu, dtype=np.int32)
        lists = IC.rows_of(indptr, items, users)
        for k in (1, 10, 256):
            for name, excl in exclusion_modes(lists, ni):
                want = want_topk(lists, nb, sc, ni, k, excl)
                x = None if excl is None else csr_of(excl)
                got = m.recommend(users, k, exclude=x)
                assert_same(got, want, "recommend k=%d excl=%s" % (k, name))
                got_l = m.recommend_lists((indptr, items), k, exclude=False if x is None else x)
                assert_same(got_l, want, "recommend_lists k=%d excl=%s" % (k, name))
                if name == "all but two":
                    assert (got[0][:, 2:] == -1).all() and np.isneginf(got[1][:, 2:]).all() if k > 2 else True
        # an empty list scores nothing: the k lowest ids that are not excluded, all at +0
        got = m.recommend(users[:1], 10)
        assert got[0].tolist() == [list(range(10))] and bits(got[1]).tolist() == [[0] * 10]
        assert_same(m.recommend_lists((indptr, items), 10, exclude=True), want_topk(lists, nb, sc, ni, 10, lists), "exclude=True")
        assert np.array_equal(m.recommend(users, 10, return_scores=False), m.recommend(users, 10)[0])
        # an unsorted exclusion row is refused, as tfr_topk refuses it
        with pytest.raises(T.TfrError) as e:
            m.recommend(users[:2], 5, exclude=(np.array([0, 2, 2], np.int64), np.array([5, 3], np.int32)))
        assert e.value.code == L.ERR_ARG
        with pytest.raises(T.OutOfRangeError):
            m.recommend(users[:1], 5, exclude=(np.array([0, 1], np.int64), np.array([ni], np.int32)))


@pytest.mark.parametrize("K", [7, 100, 130, 256])
def test_recommend_every_neighbour_row_width(K):
    """constructed lists at K below 64, up to 128 and beyond: the three ways a wave covers a neighbour row"""
    n_items = 300
    nb, sc = IC.constructed_lists(n_items, K, seed=K)
    indptr, items, nu, _ = ladder(n_items, IK.plan(n_items, 10, 1, 1)["ahead"], seed=K)
    lists = IC.rows_of(indptr, items, range(nu))
    with T.ItemKNN(nu, n_items, K=K) as m:
        m.set_neighbours(nb, sc)
        assert_same(m.recommend_lists((indptr, items), 10, exclude=True), want_topk(lists, nb, sc, n_items, 10, lists), "K=%d" % K)
        assert_same(m.recommend_lists((indptr, items), 256, exclude=None), want_topk(lists, nb, sc, n_items, 256), "K=%d k=256" % K)


def test_recommend_duplicates_and_crowd():
    indptr, items, nu, ni = IC.case("lengths")
    nb, sc = IC.fitted("lengths", 10, "cosine", 0.0)
    rs = np.random.RandomState(5)
    with fitted_model("lengths", 10) as m:
        crowd = rs.randint(0, nu, 3000).astype(np.int32)
        crowd[:4] = [9, 9, 200, 9]
        x = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
        got = m.recommend(crowd, 10, exclude=x)
        lists = IC.rows_of(indptr, items, crowd[:50])
        assert_same((got[0][:50], got[1][:50]), want_topk(lists, nb, sc, ni, 10, lists), "the crowd's first 50")
        for u in (9, 200, int(crowd[2999])):
            alone = m.recommend(np.array([u], np.int32), 10, exclude=x)
            for q in np.flatnonzero(crowd == u):
                assert_same((got[0][q], got[1][q]), (alone[0][0], alone[1][0]), "user %d alone and at %d" % (u, q))


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_recommend_and_rank_at_the_slice_edges(extra):
    w = IC.w_score()
    n_items = 2 * w + 3 if extra is None else w + extra
    name = "edge:%d" % n_items
    indptr, items, nu, ni = IC.case(name)
    nb, sc = IC.fitted(name, 10, "cosine", 0.0)
    users = np.arange(0, nu, 16, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    with fitted_model(name, 10) as m:
        assert_same(m.neighbours(), (nb, sc), name)
        for k in (10, 256):
            assert_same(m.recommend(users, k, exclude=csr_of(lists)), want_topk(lists, nb, sc, ni, k, lists), "%s k=%d" % (name, k))
        # targets on both sides of every slice edge, and the last item
        tg = np.unique([c for c in (0, w - 1, w, w + 1, 2 * w - 1, 2 * w, ni - 1) if c < ni]).astype(np.int32)
        tp = np.arange(users.size + 1, dtype=np.int64) * tg.size
        got = m.rank_items(users, (tp, np.tile(tg, users.size)), exclude=csr_of(lists))
        want = np.concatenate([R.ranks(R.user_scores(lst, nb, sc, ni), tg, lst) for lst in lists])
        assert np.array_equal(got, want)


# ---- rank ----------------------------------------------------------------------------------------------------------------
def test_rank_items_against_the_restatement_and_recommend():
    indptr, items, nu, ni = IC.case("lengths")
    nb, sc = IC.fitted("lengths", 10, "cosine", 0.0)
    rs = np.random.RandomState(6)
    users = np.array([0, 5, 5, 17, 299, 120, 64], np.int32)
    lists = IC.rows_of(indptr, items, users)
    targets = [np.sort(rs.choice(ni, n, replace=False)).astype(np.int32) for n in (ni, 0, 70, 3, 1, 0, 12)]
    targets[3] = np.sort(np.concatenate([lists[3][:2], all_but(ni, lists[3])[:1]])).astype(np.int32)    # two excluded targets
    with fitted_model("lengths", 10) as m:
        for name, excl in exclusion_modes(lists, ni):
            x = None if excl is None else csr_of(excl)
            got = m.rank_items(users, csr_of(targets), exclude=x)
            want = np.concatenate([R.ranks(R.user_scores(lst, nb, sc, ni), t, () if excl is None else excl[q])
                                   for q, (lst, t) in enumerate(zip(lists, targets))])
            assert got.dtype == np.int32 and np.array_equal(got, want), name
            tp = csr_of(targets)[0]
            for K in (1, 10, 256):
                top = m.recommend(users, K, exclude=x, return_scores=False)
                for q in range(users.size):
                    for t, r in zip(targets[q], got[tp[q]:tp[q + 1]]):
                        assert (0 <= r < K) == (t in top[q].tolist()), (name, K, q, t, r)
                        if 0 <= r < K:
                            assert top[q, r] == t
            if name == "own":
                assert got[tp[3]:tp[4]].tolist().count(-1) == 2
        # rows without targets and n = 0 are no-ops
        none = m.rank_items(users, (np.zeros(users.size + 1, np.int64), np.zeros(0, np.int32)))
        assert none.size == 0
        assert m.rank_items(np.zeros(0, np.int32), (np.zeros(1, np.int64), np.zeros(0, np.int32))).size == 0
        out = np.full(3, 77, np.int32)
        lib = L.load()
        assert lib.tfr_knn_rank_items(m._h, None, 0, None, None, None, None, L.ptr_i32(out)) == L.OK and out.tolist() == [77] * 3
        assert lib.tfr_knn_topk(m._h, None, 0, 5, None, None, L.ptr_i32(out), None) == L.OK and out.tolist() == [77] * 3


def test_evaluate_ranking_takes_the_model():
    (indptr, items, nu, ni), tu, ti = IC.planted_case()
    assert (nu, ni) == (300, 200)
    train = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
    nb, sc = R.fit(*R.cooccurrence(indptr, items, nu, ni), 20, "cosine", 0.0)
    with T.ItemKNN(nu, ni, K=20) as m:
        m.fit(train)
        res = T.evaluate_ranking(m, tu, ti, exclude=train, ks=(10,))
    users = res["users"]
    lists = IC.rows_of(indptr, items, users)
    want = np.concatenate([R.ranks(R.user_scores(lst, nb, sc, ni), res["items"][res["indptr"][q]:res["indptr"][q + 1]], lst)
                           for q, lst in enumerate(lists)])
    assert np.array_equal(res["ranks"], want)
    host = T.ranking_metrics(want, res["indptr"], ni - np.diff(indptr)[users], ks=(10,))
    for name in ("recall@10", "ndcg@10"):
        assert np.array_equal(res[name], host[name])
        assert res["mean"][name] == float(host[name].mean())
    assert res["mean"]["recall@10"] > 0.15                                     # the clusters are found: chance is 10 / 187


def test_reload_without_a_fit():
    indptr, items, nu, ni = IC.case("lengths")
    users = np.arange(0, nu, 7, dtype=np.int32)
    x = csr_of(IC.rows_of(indptr, items, users))
    with fitted_model("lengths", 65, "jaccard", 2.5) as a, T.ItemKNN(nu, ni, K=65, metric="jaccard", shrink=2.5) as b:
        nb, sc = a.neighbours()
        b.set_neighbours(nb, sc)
        assert_same(b.neighbours(), (nb, sc), "the lists")
        assert_same(b.recommend_lists(x, 20), a.recommend(users, 20, exclude=x), "lists on the second handle")
        b.load((indptr, items))
        b.set_neighbours(nb, sc)
        assert_same(b.recommend(users, 20, exclude=x), a.recommend(users, 20, exclude=x), "resident on the second handle")
        assert np.array_equal(b.rank_items(users, x), a.rank_items(users, x))
        ids, sims = a.similar_items([3, 8, 0], 5)
        assert np.array_equal(ids, nb[[3, 8, 0], :5]) and np.array_equal(bits(sims), bits(sc[[3, 8, 0], :5]))


# ---- errors that need a handle (tests/test_itemknn_host.py has the ones that do not) ---------------------------------------
def test_argument_and_state_errors():
    lib = L.load()
    i64 = lambda *v: np.array(v, np.int64)
    i32 = lambda *v: np.array(v, np.int32)
    out = np.full(8, 77, np.int32)
    with T.ItemKNN(3, 6, K=2) as m:
        h = m._h
        u = i32(0, 1)
        # before a load and before a fit
        assert lib.tfr_knn_fit(h, None) == L.ERR_STATE
        assert lib.tfr_knn_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        assert lib.tfr_knn_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(1, 2)), None, None, L.ptr_i32(out)) == L.ERR_STATE
        assert lib.tfr_knn_get_neighbours(h, 0, 6, L.ptr_i32(out), None) == L.ERR_STATE
        assert lib.tfr_knn_topk_lists(h, L.ptr_i64(i64(0, 1)), L.ptr_i32(i32(1)), 1, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE
        # load: each refusal leaves the handle unloaded
        for indptr, items, code in [(i64(1, 2, 3, 4), i32(0, 1, 2, 3), L.ERR_ARG),         # does not start at 0
                                    (i64(0, 2, 1, 3), i32(0, 1, 2), L.ERR_ARG),            # decreases
                                    (i64(0, 2, 3, 3), i32(4, 2, 1), L.ERR_ARG),            # unsorted row
                                    (i64(0, 2, 3, 3), i32(2, 2, 1), L.ERR_ARG),            # repeated item
                                    (i64(0, 2, 3, 3), i32(2, 6, 1), L.ERR_OOB),            # id out of range
                                    (i64(0, 2, 3, 3), i32(-1, 2, 1), L.ERR_OOB)]:
            assert lib.tfr_knn_load(h, L.ptr_i64(indptr), L.ptr_i32(items)) == code
            assert lib.tfr_knn_fit(h, None) == L.ERR_STATE
        m.load((i64(0, 2, 4, 4), i32(0, 1, 1, 2)))
        assert lib.tfr_knn_topk(h, L.ptr_i32(u), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_STATE       # loaded, not fitted
        m.fit()
        assert m.neighbours()[0].tolist() == [[1, -1], [0, 2], [1, -1], [-1, -1], [-1, -1], [-1, -1]]
        # queries
        assert lib.tfr_knn_topk(h, L.ptr_i32(u), 2, 0, None, None, L.ptr_i32(out), None) == L.ERR_ARG
        assert lib.tfr_knn_topk(h, L.ptr_i32(u), 2, 257, None, None, L.ptr_i32(out), None) == L.ERR_ARG
        assert lib.tfr_knn_topk(h, L.ptr_i32(i32(0, 3)), 2, 2, None, None, L.ptr_i32(out), None) == L.ERR_OOB
        assert lib.tfr_knn_topk(h, L.ptr_i32(u), 2, 2, L.ptr_i64(i64(0, 2, 2)), L.ptr_i32(i32(3, 1)), L.ptr_i32(out), None) == L.ERR_ARG
        for indptr, items, code in [(i64(1, 2), i32(0, 1), L.ERR_ARG), (i64(0, 2), i32(3, 3), L.ERR_ARG),
                                    (i64(0, 2), i32(4, 1), L.ERR_ARG), (i64(0, 2), i32(1, 6), L.ERR_OOB)]:
            assert lib.tfr_knn_topk_lists(h, L.ptr_i64(indptr), L.ptr_i32(items), 1, 2, None, None, L.ptr_i32(out), None) == code
        assert lib.tfr_knn_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 2, 2)), L.ptr_i32(i32(2, 2)), None, None, L.ptr_i32(out)) == L.ERR_ARG
        assert lib.tfr_knn_rank_items(h, L.ptr_i32(u), 2, L.ptr_i64(i64(0, 1, 2)), L.ptr_i32(i32(2, 9)), None, None, L.ptr_i32(out)) == L.ERR_OOB
        assert out.tolist() == [77] * 8                                        # no refused call wrote anything
        # set_neighbours
        ok_sc = np.zeros((6, 2), np.float32)
        for bad, code in [((0, 0, 0), L.ERR_ARG),                              # row 0 lists itself
                          ((1, 0, 6), L.ERR_OOB), ((1, 0, -2), L.ERR_OOB),
                          ((2, 0, 4), None)]:
            nb = np.full((6, 2), -1, np.int32)
            nb[:, 0] = [1, 2, 3, 4, 5, 0]
            nb[bad[0], bad[1]] = bad[2]
            if code is None:
                nb[2, 1] = 4                                                   # row 2 repeats item 4
                code = L.ERR_ARG
            assert lib.tfr_knn_set_neighbours(h, 0, 6, L.ptr_i32(nb), L.ptr_f32(ok_sc)) == code
        nb = np.full((6, 2), -1, np.int32)
        nb[:, 0] = [1, 2, 3, 4, 5, 0]
        bad_sc = ok_sc.copy()
        bad_sc[4, 0] = np.nan
        assert lib.tfr_knn_set_neighbours(h, 0, 6, L.ptr_i32(nb), L.ptr_f32(bad_sc)) == L.ERR_ARG
        assert lib.tfr_knn_set_neighbours(h, 4, 3, L.ptr_i32(nb), L.ptr_f32(ok_sc)) == L.ERR_ARG              # window past the items
        m._nb = None                                                           # read the device's lists again
        assert m.neighbours()[0].tolist() == [[1, -1], [0, 2], [1, -1], [-1, -1], [-1, -1], [-1, -1]]         # untouched


# ---- what ItemKNN shares with EASE (csrc/item_lists.h): one set of checks behind both handles ------------------------------------
def malformed_csrs():
    """(name, indptr of two rows, ids, code as a from-0 strict CSR, code as an exclusion CSR): every rule of check_csr.  The
    user CSR of a load, a list CSR and a target CSR are strict; list and user CSRs start at 0; an exclusion CSR may start
    anywhere and repeat an id.  None as a code: not malformed for that kind."""
    A, O = L.ERR_ARG, L.ERR_OOB
    return [("null indptr", None, [0, 1], A, None),                        # no exclusion CSR at all is legal
            ("indptr starts at 1", [1, 2, 3], [0, 1, 2], A, L.OK),
            ("indptr starts below 0", [-1, 1, 2], [0, 1, 2], A, A),
            ("indptr decreases", [0, 2, 1], [0, 1], A, A),
            ("ids missing", [0, 1, 2], None, A, A),
            ("id -1", [0, 2, 2], [-1, 2], O, O),
            ("id n_items", [0, 2, 2], [2, 5], O, O),
            ("row repeats an id", [0, 2, 2], [3, 3], A, L.OK),
            ("row decreases", [0, 2, 2], [4, 1], A, A)]


def test_shared_checks_refuse_alike_through_both_handles():
    lib = L.load()
    i64 = lambda v: None if v is None else L.ptr_i64(np.array(v, np.int64))
    i32 = lambda v: None if v is None else L.ptr_i32(np.array(v, np.int32))
    indptr, items = np.array([0, 2, 4, 4], np.int64), np.array([0, 1, 1, 2], np.int32)
    out = np.full(8, 77, np.int32)
    o = L.ptr_i32(out)
    u, good = [0, 1], ([0, 1, 2], [1, 2])
    with T.ItemKNN(3, 5, K=2) as knn, T.EASE(3, 5, regularization=1.0) as ease:
        knn.fit((indptr, items))
        ease.fit((indptr, items))
        served = knn.recommend(u, 5), ease.recommend(u, 5)
        fam = {"knn": knn._h, "ease": ease._h}
        fn = lambda f, name: getattr(lib, "tfr_%s_%s" % (f, name))
        text = lambda f: fn(f, "last_error")().decode()

        def mark():
            """each family's last error set to a text of its own"""
            for f in fam:
                assert fn(f, "plan")(5, 1, 1, 7, *[None] * (5 if f == "knn" else 9)) == L.ERR_ARG
                assert text(f).startswith(f + " plan: which")
            return {f: text(f) for f in fam}

        def both(what, want, call, *words):
            got = {}
            for f, other in (("knn", "ease"), ("ease", "knn")):
                marks = mark()
                assert call(f, fam[f]) == want, (what, f)
                assert text(other) == marks[other], (what, f, "wrote to the other family's text")
                if want == L.OK:
                    assert text(f) == marks[f], (what, f)
                else:
                    assert all(w in text(f) for w in words), (what, f, text(f))
                got[f] = text(f)
            assert want == L.OK or got["knn"] == got["ease"], (what, got)

        for name, p, ids, strict0, excl in malformed_csrs():
            # the target CSR is strict but need not start at 0
            tgt = (L.OK if name == "indptr starts at 1" else strict0)
            p3 = None if p is None else p + p[-1:]                             # three rows for the load
            both("load: " + name, strict0, lambda f, h: fn(f, "load")(h, i64(p3), i32(ids)), "load: ", "user ")
            both("lists: " + name, strict0, lambda f, h: fn(f, "topk_lists")(h, i64(p), i32(ids), 2, 2, None, None, o, None),
                 "top-K of lists: ", "list ")
            both("targets: " + name, tgt, lambda f, h: fn(f, "rank_items")(h, i32(u), 2, i64(p), i32(ids), None, None, o),
                 "rank: ", "target ")
            if excl is None:
                continue
            both("top-K exclusions: " + name, excl, lambda f, h: fn(f, "topk")(h, i32(u), 2, 2, i64(p), i32(ids), o, None),
                 "top-K: ", "exclusion ")
            both("lists' exclusions: " + name, excl,
                 lambda f, h: fn(f, "topk_lists")(h, i64(good[0]), i32(good[1]), 2, 2, i64(p), i32(ids), o, None),
                 "top-K of lists: ", "exclusion ")
            both("rank exclusions: " + name, excl,
                 lambda f, h: fn(f, "rank_items")(h, i32(u), 2, i64(good[0]), i32(good[1]), i64(p), i32(ids), o), "rank: ", "exclusion ")
        for bad in (-1, 3):                                                    # a user id of -1 and one of n_users
            both("top-K user %d" % bad, L.ERR_OOB, lambda f, h: fn(f, "topk")(h, i32([0, bad]), 2, 2, None, None, o, None),
                 "top-K: user id %d " % bad)
            both("rank user %d" % bad, L.ERR_OOB,
                 lambda f, h: fn(f, "rank_items")(h, i32([0, bad]), 2, i64(good[0]), i32(good[1]), None, None, o), "rank: user id %d " % bad)
        for k in (0, 257):                                                     # k of 0 and KMAX + 1
            both("top-K k %d" % k, L.ERR_ARG, lambda f, h: fn(f, "topk")(h, i32(u), 2, k, None, None, o, None), "top-K: k must be", "%d" % k)
            both("lists k %d" % k, L.ERR_ARG, lambda f, h: fn(f, "topk_lists")(h, i64(good[0]), i32(good[1]), 2, k, None, None, o, None),
                 "top-K of lists: k must be", "%d" % k)
        # no refused load reached either model: both still serve what they were fitted to
        assert_same(knn.recommend(u, 5), served[0], "ItemKNN after the refusals")
        assert_same(ease.recommend(u, 5), served[1], "EASE after the refusals")


def test_a_refused_load_leaves_a_fitted_model_serving():
    indptr, items, nu, ni = IC.case("lengths")
    users = np.arange(0, nu, 5, dtype=np.int32)
    x = csr_of(IC.rows_of(indptr, items, users))
    with fitted_model("lengths", 10) as m:
        before = m.recommend(users, 10, exclude=x)
        bad = items.copy()
        bad[-1] = ni                                                           # the last id of the last row: out of range
        assert L.load().tfr_knn_load(m._h, L.ptr_i64(indptr), L.ptr_i32(bad)) == L.ERR_OOB
        assert_same(m.recommend(users, 10, exclude=x), before, "after the refused load")
        assert_same(m.neighbours(), IC.fitted("lengths", 10, "cosine", 0.0), "the lists after the refused load")
