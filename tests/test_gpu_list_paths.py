"""Every launch path of the interaction-list layer (csrc/item_lists.h) that the families' own suites leave out, at the values of
tests/list_paths.py, bit for bit against the restatements (tests/itemknn_ref.py, userknn_ref.py, rp3_ref.py, ease_ref.py):

    a. k_knn_score<R, MODE> and k_uknn_score<R, MODE> at every (R, MODE), the neighbour row exactly full and one slot over
    b. the key queue of the three fit kernels at K + 64 == CAP and at the smallest K of the larger queue, on the staircase
    c. a second query chunk through tfr::topk_run (topk and topk_lists of four families) and UknnServe::lists_prepare, with
       exclusion rows that depend on the query's position: q_lo is no longer 0
tests/test_list_path_coverage.py checks, without a device, that these lists reach every kernel of profiles/kernel_manifest.txt."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import ease as E
from tfrecomm_amd import itemknn as IK
from tfrecomm_amd import slim as S
from tfrecomm_amd import userknn as UK
from tests import ease_cases as EC
from tests import ease_ref as ER
from tests import itemknn_cases as IC
from tests import itemknn_ref as R
from tests import list_paths as LP
from tests import rp3_ref as R3
from tests import userknn_cases as UC
from tests import userknn_ref as UR

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what="", rows=()):
    """ids equal, scores equal as bits; ``rows``: (name, row) pairs the message reports on"""
    gi, gs = np.asarray(got[0]), np.asarray(got[1])
    wi, ws = np.asarray(want[0]), np.asarray(want[1])
    assert gi.shape == wi.shape and gs.shape == ws.shape, (what, gi.shape, wi.shape)
    diff = (gi != wi) | (bits(gs) != bits(ws))
    if diff.any():
        bad = np.flatnonzero(diff.reshape(-1))
        named = ", ".join("%s (row %d) %s" % (n, r, "differs" if diff[r].any() else "agrees") for n, r in rows)
        bad_rows = np.flatnonzero(diff.reshape(diff.shape[0], -1).any(1)) if diff.ndim > 1 else bad
        raise AssertionError("%s: %d of %d slots differ in %d rows (first row %d, last row %d), first at flat index %d: got (%d, %r) "
                             "want (%d, %r)%s" % (what, bad.size, wi.size, bad_rows.size, bad_rows[0], bad_rows[-1], bad[0],
                                                  gi.reshape(-1)[bad[0]], gs.reshape(-1)[bad[0]], wi.reshape(-1)[bad[0]],
                                                  ws.reshape(-1)[bad[0]], "; " + named if named else ""))


def csr_of(lists):
    p = np.zeros(len(lists) + 1, np.int64)
    p[1:] = np.cumsum([len(x) for x in lists])
    return p, (np.concatenate(lists).astype(np.int32) if len(lists) and p[-1] else np.zeros(0, np.int32))


def want_topk(score_rows, k, excl=None):
    items = np.empty((len(score_rows), k), np.int32)
    scores = np.empty((len(score_rows), k), np.float32)
    for q, row in enumerate(score_rows):
        items[q], scores[q] = R.topk(row, k, () if excl is None else excl[q])
    return items, scores


# ---- a. every (R, MODE) of both scoring kernels ----------------------------------------------------------------------------------
def fill_row(nb, sc, row, seed):
    """row ``row`` of constructed lists completely full: K distinct ids that are not the row's own, float32 scores of both signs"""
    n, K = nb.shape
    rs = np.random.RandomState(seed)
    cand = rs.permutation(n - 1)[:K]
    nb[row] = cand + (cand >= row)
    sc[row] = rs.normal(0, 1, K).astype(np.float32)


def knn_scoring_case(K):
    """(model, users, their lists, their float32 score rows, n_items): 300 items, constructed lists with a full row that a query
    list names, the ladder of query lists around the look-ahead"""
    n_items = 300
    ahead = IK.plan(n_items, 10, 1, 1)["ahead"]
    rs = np.random.RandomState(200 + K)
    lens = [0, 1, ahead - 1, ahead, ahead + 1, 2 * ahead, 2 * ahead + 1, 40] * 2
    indptr, items, nu, _ = IC.csr_of_rows([rs.choice(n_items, n, replace=False) for n in lens], n_items)
    users = np.arange(nu, dtype=np.int32)
    lists = IC.rows_of(indptr, items, users)
    nb, sc = IC.constructed_lists(n_items, K, seed=K)
    fill_row(nb, sc, int(lists[-1][0]), K)
    assert min(K, n_items - 1) == int((nb >= 0).sum(1).max())
    m = T.ItemKNN(nu, n_items, K=K)
    m.load((indptr, items))
    m.set_neighbours(nb, sc)
    return m, users, lists, [R.user_scores(lst, nb, sc, n_items) for lst in lists], n_items


def uknn_scoring_case(K):
    """the scoring case of tests/userknn_cases.py (300 users, 400 items) with its constructed lists, user 20's row full"""
    indptr, items, nu, ni = UC.case("scoring")
    users = np.array([0, 1, 2, 3, 4, 5, 7, 8, 9, 13, 13, 20, 299] + list(range(30, 290, 26)), np.int32)
    # (the rows UC.constructed_lists sets by hand need four slots)
    nb, sc = UC.constructed_lists(nu, K) if K >= 4 else IC.constructed_lists(nu, K, seed=36)
    fill_row(nb, sc, 20, K)
    assert K == int((nb >= 0).sum(1).max())
    m = T.UserKNN(nu, ni, K=K)
    m.load((indptr, items))
    m.set_neighbours(nb, sc)
    return m, users, IC.rows_of(indptr, items, users), [UR.user_scores(nb[u], sc[u], indptr, items, ni) for u in users], ni


@pytest.mark.parametrize("K", LP.KNN_SCORE_KS)
@pytest.mark.parametrize("family", ["knn", "uknn"])
def test_every_scoring_round_and_mode_against_the_restatement(family, K):
    """recommend (MODE 0) at k 10 and 256 with and without exclusion, rank_items (MODE 1 and 2) against R.ranks of the restated
    score rows - targets that are excluded, more than 64 targets for one user, a user without targets - and rank < k exactly
    when recommend holds the target at that position"""
    m, users, lists, rows, ni = (knn_scoring_case if family == "knn" else uknn_scoring_case)(K)
    rs = np.random.RandomState(300 + K)
    targets = []
    for q, lst in enumerate(lists):
        if q == 1:
            targets.append(np.zeros(0, np.int32))                              # a user without targets
        elif q in (0, 7):
            targets.append(np.sort(rs.choice(ni, 70 + 30 * q, replace=False)).astype(np.int32))   # more than 64, more than 256
        else:
            targets.append(np.unique(np.concatenate([lst[:2], rs.choice(ni, 5, replace=False)])).astype(np.int32))
    tp, tids = csr_of(targets)
    assert np.diff(tp).max() > 256 and sum(np.isin(t, lst).sum() for t, lst in zip(targets, lists)) > 10
    with m:
        for name, excl in (("none", None), ("own", lists)):
            x = None if excl is None else csr_of(excl)
            what = "%s K=%d excl=%s" % (family, K, name)
            top = {}
            for k in (10, 256):
                got = m.recommend(users, k, exclude=x)
                assert_same(got, want_topk(rows, k, excl), what + " recommend k=%d" % k)
                top[k] = got[0]
            got = m.rank_items(users, (tp, tids), exclude=x)
            want = np.concatenate([R.ranks(rows[q], targets[q], () if excl is None else excl[q]) for q in range(users.size)])
            bad = np.flatnonzero(got != want)
            assert got.dtype == np.int32 and bad.size == 0, "%s rank_items: %d of %d differ, first target %d: got %d want %d" % (
                what, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])
            if excl is not None:
                assert (got == -1).sum() == sum(np.isin(t, lst).sum() for t, lst in zip(targets, lists))
            for k in (10, 256):
                for q in range(users.size):
                    held = top[k][q].tolist()
                    for t, r in zip(targets[q], got[tp[q]:tp[q + 1]]):
                        assert (0 <= r < k) == (int(t) in held), (what, k, q, t, r)
                        if 0 <= r < k:
                            assert held[r] == t, (what, k, q, t, r)


# ---- b. the queue edges of the three fit kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", LP.KNN_FIT_KS)
@pytest.mark.parametrize("kind", ["cosine", "count", "weighted"])
def test_fit_queue_edges_on_the_staircase(kind, K):
    """the staircase (tests/itemknn_cases.py: row 0's similarities rise along the catalogue, so every 64 columns a wave scans
    beat all it has kept) at K = 192, where K plus one append fills the 256-key queue to its last slot, and at K = 193, the
    first K on 512 keys: k_knn_cooc by tfr_knn_fit, k_knn_cooc_w by RP3beta's weighted fit"""
    indptr, items, nu, ni = IC.case("staircase")
    assert ni == 2304
    if kind == "weighted":
        want = R3.rp3_fit(indptr, items, nu, ni, K, 1.0, 0.6)
        with T.RP3beta(nu, ni, K=K, alpha=1.0, beta=0.6) as m:
            got = m.fit((indptr, items)).neighbours()
    else:
        want = IC.fitted("staircase", K, kind, 0.0)
        with T.ItemKNN(nu, ni, K=K, metric=kind) as m:
            got = m.fit((indptr, items)).neighbours()
    assert want[0][0, :64].tolist() == list(range(ni - 64, ni))               # the best are the last step, by id
    assert (want[0][0] >= 0).all() and (want[0][:, K - 1] >= 0).sum() > ni // 2   # rows that fill all K slots
    assert_same(got, want, "staircase %s K=%d" % (kind, K))


def transposed_staircase(private):
    """2304 users; user v holds items 0 .. v // 64, so a list of all 36 items shares v // 64 + 1 of them with user v: under the
    count metric the similarities rise along the users as the staircase's do along the items.  ``private``: user v also holds
    an item 36 + v of its own, whose score tells which users were kept as neighbours (users of one step hold the same common
    items, so without it a wrong pick inside a step would not show)"""
    nu, steps = 2304, 36
    rows = [list(range(v // 64 + 1)) + ([steps + v] if private else []) for v in range(nu)]
    return IC.csr_of_rows(rows, steps + (nu if private else 0))


@pytest.mark.parametrize("K", LP.UKNN_LIST_KS)
@pytest.mark.parametrize("private", [False, True], ids=["common", "private"])
def test_list_neighbours_queue_edges_on_the_transposed_staircase(private, K):
    """k_uknn_query_cooc<256> at its tightest K and k_uknn_query_cooc<512> at its first, on a loaded handle without a fit: the
    neighbours of the lists are searched at query time, and their scores go through k_uknn_score<4, 0>"""
    case = transposed_staircase(private)
    indptr, items, nu, ni = case
    every = np.arange(ni, dtype=np.int32)
    lists = [every, every[:36], every[:20], np.array([35], np.int32), np.zeros(0, np.int32), every[5:36]]
    nbs = [UR.list_neighbours(lst, indptr, items, nu, ni, K, "count", 0.0) for lst in lists]
    assert nbs[1][0].tolist() == list(range(nu - 64, nu)) + list(range(nu - 128, nu - 64)) + list(range(nu - 192, nu - 128)) + \
        ([nu - 256] if K == 193 else [])                                       # the last steps, each by id
    assert (nbs[4][0] == -1).all() and nbs[3][0][:64].tolist() == list(range(nu - 64, nu)) and nbs[3][0][64] == -1
    rows = [UR.user_scores(nb, sc, indptr, items, ni) for nb, sc in nbs]
    with T.UserKNN(nu, ni, K=K, metric="count") as m:
        m.load((indptr, items))
        for k in (36, 256):
            assert_same(m.recommend_lists(csr_of(lists), k, exclude=False), want_topk(rows, k), "K=%d k=%d" % (K, k))
        assert_same(m.recommend_lists(csr_of(lists), 10), want_topk(rows, 10, lists), "K=%d k=10, own items excluded" % K)


# ---- c. a second query chunk through every serving driver ------------------------------------------------------------------------
N_USERS, N_ITEMS = 7, 9


def tiny_rows():
    """7 users over 9 items: an empty row, a full one, the others two to five items"""
    rs = np.random.RandomState(51)
    rows = [[], list(range(N_ITEMS))] + [rs.choice(N_ITEMS, n, replace=False) for n in (2, 3, 5, 4, 2)]
    return IC.csr_of_rows(rows, N_ITEMS)


def tiny_model(family, n_items=N_ITEMS, n_users=N_USERS, rows=None):
    """(model, score of a list -> float32 row, list plan, K or None): constructed weights / lists whose scores are multiples of
    1/8, so equal sums tie exactly and go by id"""
    indptr, items, nu, ni = tiny_rows() if rows is None else rows
    if family == "knn":
        nb, sc, _ = EC.twin_case(ni, 4, seed=52)
        m = T.ItemKNN(nu, ni, K=4)
        m.load((indptr, items))
        m.set_neighbours(nb, sc)
        return m, (lambda lst: R.user_scores(lst, nb, sc, ni)), IK.plan
    if family in ("ease", "slim"):
        B = EC.constructed_weights(ni)
        m = T.EASE(nu, ni, regularization=1.0) if family == "ease" else T.SLIM(nu, ni)
        m.load((indptr, items))
        m.set_weights(B)
        return m, (lambda lst: ER.user_scores(lst, B)), (E.plan if family == "ease" else S.plan)
    nb, sc, _ = EC.twin_case(nu, 3, seed=53)                                   # neighbour users of every fill, scores in eighths
    m = T.UserKNN(nu, ni, K=3, metric="jaccard", shrink=0.5)
    m.load((indptr, items))
    m.set_neighbours(nb, sc)
    return m, (lambda lst: None), UK.plan


def positional_exclusions(own, n, n_items):
    """row q excludes item q % n_items, and its own list too where q % 3 == 0: (rows of one period, period).  ``own``: the
    lists the queries cycle through"""
    period = int(np.lcm.reduce([len(own), n_items, 3]))
    return [np.unique(np.concatenate([[q % n_items], own[q % len(own)] if q % 3 == 0 else []])).astype(np.int32)
            for q in range(period)], period


def tiled_csr(rows, n):
    """the CSR of n rows that cycle through ``rows``"""
    p, ids = csr_of(rows)
    reps, rem = divmod(n, len(rows))
    lens = np.concatenate([np.tile(np.diff(p), reps), np.diff(p)[:rem]])
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    return indptr, np.concatenate([np.tile(ids, reps), ids[:p[rem]]]).astype(np.int32)


def check_chunked(call, score_rows, own, n, k, n_items, chunk, what):
    """``call(exclusion CSR)`` -> (items, scores) of n queries that cycle through ``own`` (their lists) and ``score_rows``"""
    excl, period = positional_exclusions(own, n, n_items)
    want = want_topk([score_rows[q % len(own)] for q in range(period)], k, excl)
    at = np.arange(n) % period
    assert n > chunk and (n - chunk) % period != 0                             # a chunk-relative index reads other rows
    named = [("chunk - 1", chunk - 1), ("chunk", chunk), ("chunk + 1", chunk + 1), ("last", n - 1)]
    assert any(not np.array_equal(excl[(chunk + d) % period], excl[d]) for d in range(period))
    assert_same(call(tiled_csr(excl, n)), (want[0][at], want[1][at]), what, named)


@pytest.mark.parametrize("k", LP.CHUNKED_KS)
@pytest.mark.parametrize("family", LP.CHUNKED_FAMILIES)
def test_a_second_query_chunk(family, k):
    """chunk + 2 queries, chunk from the family's plan: the launches of the second chunk have q_lo = chunk, read their
    exclusion rows, query lists and (UserKNN's lists) neighbour rows at the absolute query and write part at the relative one;
    the merge writes at out + chunk * k.  Resident users through topk, lists through topk_lists"""
    indptr, items, nu, ni = tiny_rows()
    m, score, plan = tiny_model(family)
    chunk = plan(ni, k, 10 ** 7, 1)["chunk"]
    n = chunk + 2
    with m:
        users = (np.arange(n) % nu).astype(np.int32)
        own = IC.rows_of(indptr, items, range(nu))
        if family == "uknn":
            nb, sc = m.neighbours()
            rows = [UR.user_scores(nb[u], sc[u], indptr, items, ni) for u in range(nu)]
        else:
            rows = [score(lst) for lst in own]
        check_chunked(lambda x: m.recommend(users, k, exclude=x), rows, own, n, k, ni, chunk, "%s recommend k=%d n=%d" % (family, k, n))

        # ten distinct lists: an empty one, one equal to a resident row, every item, single items
        rs = np.random.RandomState(54)
        lists = [np.zeros(0, np.int32), own[4], np.arange(ni, dtype=np.int32), np.array([8], np.int32), np.array([0], np.int32)]
        lists += [np.sort(rs.choice(ni, c, replace=False)).astype(np.int32) for c in (2, 3, 4, 6, 7)]
        if family == "uknn":
            with T.UserKNN(nu, ni, K=3, metric="jaccard", shrink=0.5) as bare:      # loaded, not fitted: the neighbours are searched
                bare.load((indptr, items))
                chunk = max(chunk, UK.plan(nu, 3, 10 ** 7, 2)["chunk"])
                n = chunk + 2
                assert n > 8192                                                    # and the search's grid takes rows in strides
                nbs = [UR.list_neighbours(lst, indptr, items, nu, ni, 3, "jaccard", 0.5) for lst in lists]
                rows = [UR.user_scores(a, b, indptr, items, ni) for a, b in nbs]
                check_chunked(lambda x: bare.recommend_lists(tiled_csr(lists, n), k, exclude=x), rows, lists, n, k, ni, chunk,
                              "uknn recommend_lists k=%d n=%d" % (k, n))
        else:
            rows = [score(lst) for lst in lists]
            check_chunked(lambda x: m.recommend_lists(tiled_csr(lists, n), k, exclude=x), rows, lists, n, k, ni, chunk,
                          "%s recommend_lists k=%d n=%d" % (family, k, n))


def test_a_second_query_chunk_set_by_the_key_bytes():
    """two scoring slices at k = 256: the chunk is 128 MiB / (2 * 256 * 8) = 32768 queries, not the cap of 65536, and part is
    written at (query of the chunk) * slices + slice"""
    family, ni, k = LP.CHUNKED_BY_BYTES
    rs = np.random.RandomState(55)
    nu = 5
    case = IC.csr_of_rows([[], [0, ni - 1]] + [rs.choice(ni, c, replace=False) for c in (3, 5, 8)], ni)
    m, score, plan = tiny_model(family, rows=case)
    p = plan(ni, k, 10 ** 7, 1)
    assert p["slices"] == 2 and p["chunk"] == (128 << 20) // (2 * k * 8) < plan(N_ITEMS, k, 10 ** 7, 1)["chunk"]
    n = p["chunk"] + 2
    with m:
        own = IC.rows_of(case[0], case[1], range(nu))
        rows = [score(lst) for lst in own]
        users = (np.arange(n) % nu).astype(np.int32)
        check_chunked(lambda x: m.recommend(users, k, exclude=x), rows, own, n, k, ni, p["chunk"], "%s recommend k=%d n=%d" % (family, k, n))
        check_chunked(lambda x: m.recommend_lists(tiled_csr(own, n), k, exclude=x), rows, own, n, k, ni, p["chunk"],
                      "%s recommend_lists k=%d n=%d" % (family, k, n))
