"""The weighted co-occurrence fit (tfr_knn_fit_weighted) and RP3beta on the device against the NumPy restatement
(tests/rp3_ref.py), bit for bit: neighbour ids equal, similarities equal as bits.  The interaction matrices are ItemKNN's
constructed cases (tests/itemknn_cases.py) with the catalogue edges taken from tfr_knn_weighted_plan; the weighted counters
get cases of their own: a carry past 2^32 inside one counter, sums past 2^53 on a 257-user item with one sum placed so that
a truncating uint64 -> float64 conversion would show, a 64-user group in which every lost or doubled user shows, a user of
weight 0 as the only link, ties by id, and a row scale of 0.  Serving is ItemKNN's and is held to tests/itemknn_ref.py on
the restated lists."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import rp3beta as RP
from tests import itemknn_cases as IC
from tests import itemknn_ref as R
from tests import rp3_ref as R3

pytestmark = pytest.mark.gpu

AB = [(1.0, 0.6), (0.5, 0.0), (2.0, 1.0)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    gi, gs = got
    wi, ws = want
    bad = np.flatnonzero((np.asarray(gi) != np.asarray(wi)).reshape(-1) | (bits(gs) != bits(ws)).reshape(-1))
    assert bad.size == 0, "%s: %d of %d slots differ, first at flat index %d: got (%d, %r) want (%d, %r)" % (
        what, bad.size, np.asarray(wi).size, bad[0], np.asarray(gi).reshape(-1)[bad[0]], np.asarray(gs).reshape(-1)[bad[0]],
        np.asarray(wi).reshape(-1)[bad[0]], np.asarray(ws).reshape(-1)[bad[0]])


def w_wfit(K=10):
    return RP.weighted_plan(100, K, 100)["width"]


@functools.lru_cache(maxsize=None)
def rp3_sums(name, alpha, beta):
    """(S, row_scale, col_scale, shift, q) of RP3beta on a named case of tests/itemknn_cases.py; built once"""
    indptr, items, nu, ni = IC.case(name)
    q, rs, cs, shift = R3.rp3_terms(indptr, items, nu, ni, alpha, beta)
    return R3.weighted_sums(indptr, items, nu, ni, q), rs, cs, shift, q


@functools.lru_cache(maxsize=None)
def rp3_want(name, K, alpha=1.0, beta=0.6):
    s, rs, cs, shift, _ = rp3_sums(name, alpha, beta)
    return R3.fit(s, rs, cs, shift, K)


def check_rp3(name, K, alpha=1.0, beta=0.6):
    indptr, items, nu, ni = IC.case(name)
    with T.RP3beta(nu, ni, K=K, alpha=alpha, beta=beta) as m:
        got = m.fit((indptr, items)).neighbours()
        _, _, _, shift, q = rp3_sums(name, alpha, beta)
        assert m.shift == shift and np.array_equal(m.q, q) and m.fit_ms > 0
    assert_same(got, rp3_want(name, K, alpha, beta), "%s K=%d alpha=%g beta=%g" % (name, K, alpha, beta))
    return got


def u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def f64p(a):
    return a.ctypes.data_as(L._f64p)


# ---- the constructed matrices of ItemKNN --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lengths", "full_user", "ties", "staircase"])
def test_fit_constructed_cases_at_every_k(name):
    """item lists of 0, 1, 63, 64, 65, 255, 256, 257 users; a user with every item; exact ties; rising scores that sort-cut
    both queue sizes"""
    for K in (1, 10, 64, 65, 256):
        nb, sc = check_rp3(name, K)
    if name == "lengths":
        assert (nb[0] == -1).all() and np.isneginf(sc[0]).all()               # nobody has item 0
        assert (nb[:, 129:] == -1).all()                                      # 130 items: at most 129 neighbours
    if name == "ties":
        nb, sc = rp3_want(name, 10)
        assert nb[80, :10].tolist() == [75, 76, 77, 78, 79, 81, 82, 83, 84, 85]   # block 3: all tie, lowest ids first
        assert len(set(bits(sc[80]).tolist())) == 1


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_fit_catalogue_at_the_slice_edges(extra):
    w = w_wfit()
    n_items = 2 * w + 3 if extra is None else w + extra
    assert RP.weighted_plan(n_items, 10, n_items)["slices"] == (3 if extra is None else 2 if extra == 1 else 1)
    check_rp3("edge:%d" % n_items, 10)


def test_fit_70000_items():
    p = RP.weighted_plan(70000, 10, 70000)
    assert p["chunk"] < 70000 and p["slices"] == 9
    check_rp3("big", 10)


# ---- the weighted counters alone -------------------------------------------------------------------------------------------
def carry_case():
    """two users of weight 2^31 + 1 share items 0 and 1: S = 2^32 + 2 carries out of the low word of one counter; a third
    pair of items shares one of them"""
    csr = IC.csr_of_item_lists({0: [0, 1], 1: [0, 1], 2: [1], 3: [2]}, 3, 5)
    return csr, np.array([2 ** 31 + 1, 2 ** 31 + 1, 7], np.uint64), np.ones(5), np.ones(5), 0


def past_2_53_case():
    """item 0 has 257 users of raw weights near 2^54 at shift 40; item 1 has them all (S near 2^62), items 2.. random
    subsets of at least 8 (S past 2^57), and item 41 users 0 and 1, whose weights sum to 2^55 + 2^32 + 2^31 - 1: the correctly
    rounded float64 is the float32 midpoint 2^55 + 2^32 + 2^31, which goes to the even 2^55 + 2^33; a truncated one goes
    down to 2^55 + 2^32"""
    rs = np.random.RandomState(41)
    n_users = 257
    q = (2 ** 54 + 2 * rs.randint(0, 2 ** 19, n_users).astype(np.int64) + 1).astype(np.uint64)
    q[0], q[1] = 2 ** 54 + 2 ** 32, 2 ** 54 + 2 ** 31 - 1
    lists = {0: range(n_users), 1: range(n_users), 41: [0, 1]}
    for i in range(2, 41):
        lists[i] = rs.choice(n_users, rs.randint(8, 200), replace=False)
    return IC.csr_of_item_lists(lists, n_users, 42), q, np.ones(42), np.ones(42), 40


def group_case():
    """one item of 64 users - a single round of one wave - with weights (u + 1) * 2^39; item j shares users 0..j-1, so each
    sum is another triangle number times 2^39 and a lost or doubled user moves it by at least 2^39, which float32 shows"""
    lists = {0: range(64)}
    for j in range(1, 65):
        lists[j] = range(j)
    q = ((np.arange(64, dtype=np.int64) + 1) << 39).astype(np.uint64)
    return IC.csr_of_item_lists(lists, 64, 65), q, np.ones(65), np.ones(65), 40


def links_case():
    """user 3 (weight 0) is the only link between items 4 and 5: not neighbours.  Row 0: S_01 = S_02 with col_scale 1 and
    0.5 are told apart, S_03 = 2^31 + 1 and S_06 = 2^31 + 3 are one float32 and go by id.  Row 7 has row_scale 0: its
    candidates stay, all at +0, in id order"""
    lists = {0: [0, 1, 2], 1: [0], 2: [0], 3: [1], 6: [1, 2], 4: [3, 4], 5: [3, 5], 7: [0, 1, 2, 4]}
    q = np.array([5, 2 ** 31 + 1, 2, 0, 9, 11], np.uint64)
    rs, cs = np.ones(8), np.ones(8)
    cs[1], rs[7] = 0.5, 0.0
    return IC.csr_of_item_lists(lists, 6, 8), q, rs, cs, 0


WEIGHTED = {"carry": carry_case, "past_2_53": past_2_53_case, "group": group_case, "links": links_case}


@pytest.mark.parametrize("name", sorted(WEIGHTED))
def test_weighted_counters(name):
    (indptr, items, nu, ni), q, rs, cs, shift = WEIGHTED[name]()
    s = R3.weighted_sums(indptr, items, nu, ni, q)
    dense = s.toarray()
    for K in (3, 256):
        want = R3.fit(s, rs, cs, shift, K)
        with T.WeightedItemKNN(nu, ni, K=K) as m:
            m.load((indptr, items))
            got = m.fit_raw(q, rs, cs, shift).neighbours()
        assert_same(got, want, "%s K=%d" % (name, K))
    nb, sc = want
    if name == "carry":
        assert dense[0, 1] == 2 ** 32 + 2 and nb[0, 0] == 1 and sc[0, 0] == np.float32(2 ** 32)
    if name == "past_2_53":
        assert dense[0, 1] > 2 ** 62 and dense[0, 2:41].min() > 2 ** 53
        assert dense[0, 41] == 2 ** 55 + 2 ** 32 + 2 ** 31 - 1
        at = nb[0].tolist().index(41)
        assert float(sc[0, at]) * 2.0 ** 40 == 2 ** 55 + 2 ** 33                # not 2^55 + 2^32: the conversion rounds
    if name == "group":
        assert [int(v) >> 39 for v in dense[0, 1:65]] == [j * (j + 1) // 2 for j in range(1, 65)]
        assert len(set(bits(sc[0, :64]).tolist())) == 64
    if name == "links":
        assert 5 not in nb[4].tolist() and 4 not in nb[5].tolist() and dense[4, 5] == 0
        assert dense[0, 1] == dense[0, 2] == 5 and nb[0].tolist().index(2) < nb[0].tolist().index(1)
        assert (dense[0, 3], dense[0, 6]) == (2 ** 31 + 1, 2 ** 31 + 3)
        assert nb[0, :2].tolist() == [3, 6] and sc[0, :2].tolist() == [2.0 ** 31] * 2
        kept = nb[7][nb[7] >= 0]
        assert kept.tolist() == [0, 1, 2, 3, 4, 6] and bits(sc[7, :6]).tolist() == [0] * 6


# ---- fit twice -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", AB)
def test_rp3beta_fits_twice_to_the_same_bits(alpha, beta):
    name = "edge:%d" % (w_wfit() + 1)
    indptr, items, nu, ni = IC.case(name)
    assert nu == 400
    with T.RP3beta(nu, ni, K=100, alpha=alpha, beta=beta) as m:
        first = tuple(a.copy() for a in m.fit((indptr, items)).neighbours())
        second = m.fit((indptr, items)).neighbours()
    assert_same(second, first, "a second fit")
    assert_same(first, rp3_want(name, 100, alpha, beta), "alpha=%g beta=%g" % (alpha, beta))


# ---- serving follows -------------------------------------------------------------------------------------------------------
def csr_of(lists):
    p = np.zeros(len(lists) + 1, np.int64)
    p[1:] = np.cumsum([len(x) for x in lists])
    return p, (np.concatenate(lists).astype(np.int32) if len(lists) else np.zeros(0, np.int32))


def want_topk(lists, nb, sc, n_items, k, excl=None):
    items = np.empty((len(lists), k), np.int32)
    scores = np.empty((len(lists), k), np.float32)
    for z, lst in enumerate(lists):
        items[z], scores[z] = R.topk(R.user_scores(lst, nb, sc, n_items), k, () if excl is None else excl[z])
    return items, scores


def test_serving_follows_the_restated_lists():
    (indptr, items, nu, ni), tu, ti = IC.planted_case()
    train = sp.csr_matrix((np.ones(items.size, np.float32), items, indptr), shape=(nu, ni))
    nb, sc = R3.rp3_fit(indptr, items, nu, ni, 20, 1.0, 0.6)
    users = np.arange(0, nu, 3, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    x = csr_of(lists)
    with T.RP3beta(nu, ni, K=20) as m, T.ItemKNN(nu, ni, K=20) as plain:
        m.fit(train)
        assert_same(m.neighbours(), (nb, sc), "the lists")
        for k in (10, 256):
            want = want_topk(lists, nb, sc, ni, k, lists)
            assert_same(m.recommend(users, k, exclude=train), want, "recommend k=%d" % k)
            assert_same(m.recommend_lists(x, k, exclude=True), want, "recommend_lists k=%d" % k)
        tg = [np.unique(np.random.RandomState(int(u)).choice(ni, 9)).astype(np.int32) for u in users]
        got = m.rank_items(users, csr_of(tg), exclude=x)
        want = np.concatenate([R.ranks(R.user_scores(lst, nb, sc, ni), t, lst) for lst, t in zip(lists, tg)])
        assert np.array_equal(got, want)
        ids, sims = m.similar_items([3, 8, 0], 5)
        assert np.array_equal(ids, nb[[3, 8, 0], :5]) and np.array_equal(bits(sims), bits(sc[[3, 8, 0], :5]))

        res = T.evaluate_ranking(m, tu, ti, exclude=train, ks=(10,))
        eu = res["users"]
        el = IC.rows_of(indptr, items, eu)
        want = np.concatenate([R.ranks(R.user_scores(lst, nb, sc, ni), res["items"][res["indptr"][z]:res["indptr"][z + 1]], lst)
                               for z, lst in enumerate(el)])
        assert np.array_equal(res["ranks"], want)
        host = T.ranking_metrics(want, res["indptr"], ni - np.diff(indptr)[eu], ks=(10,))
        for name in ("recall@10", "ndcg@10"):
            assert np.array_equal(res[name], host[name])
        assert res["mean"]["recall@10"] > 0.15                                # the clusters are found: chance is 10 / 187

        # the lists move to a plain ItemKNN handle and serve the same bits there
        plain.load((indptr, items))
        plain.set_neighbours(*m.neighbours())
        assert_same(plain.recommend(users, 10, exclude=train), m.recommend(users, 10, exclude=train), "on an ItemKNN handle")
        assert np.array_equal(plain.rank_items(users, csr_of(tg), exclude=x), got)


# ---- state ---------------------------------------------------------------------------------------------------------------
def test_state_and_refused_calls():
    lib = L.load()
    indptr, items, nu, ni = IC.case("lengths")
    users = np.arange(0, nu, 5, dtype=np.int32)
    x = csr_of(IC.rows_of(indptr, items, users))
    q, rs, cs, shift, = R3.rp3_terms(indptr, items, nu, ni, 1.0, 0.6)
    fit = lambda h, q_=q, rs_=rs, cs_=cs, shift_=shift: lib.tfr_knn_fit_weighted(
        h, None if q_ is None else u64p(q_), None if rs_ is None else f64p(rs_), None if cs_ is None else f64p(cs_), shift_, None)
    with T.WeightedItemKNN(nu, ni, K=10) as m:
        h = m._h
        assert fit(h) == L.ERR_STATE and b"tfr_knn_load" in lib.tfr_knn_last_error()           # before a load
        m.load((indptr, items))
        assert lib.tfr_knn_topk(h, L.ptr_i32(users), users.size, 5, None, None, L.ptr_i32(np.empty(users.size * 5, np.int32)),
                                None) == L.ERR_STATE                                           # loaded, not fitted
        m.fit_raw(q, rs, cs, shift)
        want = rp3_want("lengths", 10)
        assert_same(m.neighbours(), want, "the fit")
        before = m.recommend(users, 10, exclude=x)

        def scale(at, value, base):
            out = base.copy()
            out[at] = value
            return out
        longest = int(np.bincount(items).max())
        assert longest == nu                                                                   # item 8: every user
        refused = [("shift -1", dict(shift_=-1)), ("shift 63", dict(shift_=63)),
                   ("null weights", dict(q_=None)), ("null row scales", dict(rs_=None)), ("null column scales", dict(cs_=None)),
                   ("negative row scale", dict(rs_=scale(5, -1e-300, rs))), ("negative column scale", dict(cs_=scale(129, -1.0, cs))),
                   ("NaN row scale", dict(rs_=scale(0, np.nan, rs))), ("NaN column scale", dict(cs_=scale(7, np.nan, cs))),
                   ("infinite row scale", dict(rs_=scale(3, np.inf, rs))), ("infinite column scale", dict(cs_=scale(3, np.inf, cs))),
                   ("a sum could reach 2^63", dict(q_=scale(200, (2 ** 63 - 1) // longest + 1, q), shift_=62)),
                   ("a similarity past float32", dict(rs_=scale(3, 1e300, rs)))]
        for what, kw in refused:
            assert fit(h, **kw) == L.ERR_ARG, what
            assert lib.tfr_knn_last_error().startswith(b"fit_weighted: "), what
        assert lib.tfr_knn_fit_weighted(None, u64p(q), f64p(rs), f64p(cs), shift, None) == L.ERR_ARG
        m._nb = None                                                                           # read the device's lists again
        assert_same(m.neighbours(), want, "the lists after the refusals")
        assert_same(m.recommend(users, 10, exclude=x), before, "serving after the refusals")
        # the largest weight that keeps every sum below 2^63 is taken
        assert fit(h, q_=scale(200, (2 ** 63 - 1) // longest, q), shift_=62) == L.OK

        # tfr_knn_fit and tfr_knn_fit_weighted replace each other's lists on one handle
        m.fit_raw(q, rs, cs, shift)
        assert lib.tfr_knn_fit(h, None) == L.OK
        m._nb = None
        assert_same(m.neighbours(), IC.fitted("lengths", 10, "count", 0.0), "tfr_knn_fit after the weighted fit")
        assert_same(m.fit_raw(q, rs, cs, shift).neighbours(), want, "the weighted fit after tfr_knn_fit")
        # a load forgets them
        m.load((indptr, items))
        with pytest.raises(T.TfrError) as e:
            m.neighbours()
        assert e.value.code == L.ERR_STATE
        assert_same(m.fit_raw(q, rs, cs, shift).neighbours(), want, "a fit after the second load")


def test_catalogue_past_the_weighted_plan():
    """8192 * 32 + 1 items at K 256 fit tfr_knn_fit's plan (slices of 16384) and not the weighted one"""
    n_items = w_wfit() * 32 + 1
    q, s = np.ones(3, np.uint64), np.ones(n_items)
    with T.WeightedItemKNN(3, n_items, K=256) as m:
        with pytest.raises(T.TfrError) as e:
            m.fit_raw(q, s, s, 0)
        assert e.value.code == L.ERR_ARG and "slices" in str(e.value)
