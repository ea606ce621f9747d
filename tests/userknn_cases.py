"""The constructed interaction matrices of tests/test_gpu_userknn.py, as (indptr int64, items int32, n_users, n_items), and
cached restatements of them (tests/userknn_ref.py).  Each builder names the edge it is there for; the slice widths come from
tfr_uknn_plan, so the cases move with the launchers.  Where ItemKNN's cases (tests/itemknn_cases.py) already hold the edge
on the item side, the case here is their transpose."""
import functools

import numpy as np

from tests import itemknn_cases as IC
from tests import userknn_ref as R
from tfrecomm_amd import userknn as UK

csr_of_rows, rows_of = IC.csr_of_rows, IC.rows_of


def transpose(case):
    indptr, items, nu, ni = case
    t = R.IR.pattern(indptr, items, nu, ni).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(np.int64), t.indices.astype(np.int32), ni, nu


def w_fit(K=10):
    return UK.plan(100, K, 100, 0)["width"]


def w_score(k=10):
    return UK.plan(100, k, 1, 1)["width"]


def w_lists(K=10):
    return UK.plan(100, K, 1, 2)["width"]


def lengths_case():
    """User rows of 0, 1, 63, 64, 65 items (the 64 row bounds a fit wave loads at once), 255, 256, 257 (the block's four
    waves), item 299 that every user with a row has, and 130 users in all, so K = 256 pads every row"""
    n_users, n_items = 130, 300
    rs = np.random.RandomState(31)
    rows = [[], [299]]
    for n in (63, 64, 65, 255, 256, 257):
        rows.append(list(rs.choice(n_items - 1, n - 1, replace=False)) + [299])
    while len(rows) < n_users:
        rows.append(list(rs.choice(n_items - 1, rs.randint(1, 40), replace=False)) + [299])
    return csr_of_rows(rows, n_items)


def sparse_lengths_case():
    """the same row lengths without the common item: users with few, one or no co-raters"""
    n_users, n_items = 130, 300
    rs = np.random.RandomState(32)
    rows = [[], [7]]
    for n in (63, 64, 65, 255, 256, 257):
        rows.append(rs.choice(n_items, n, replace=False))
    while len(rows) < n_users:
        rows.append(rs.choice(n_items, rs.randint(0, 6), replace=False))
    return csr_of_rows(rows, n_items)


def edge_case(n_users):
    """a user count at a slice edge: the users next to every multiple of the fit width that exist share items"""
    return transpose(IC.edge_case(n_users, seed=33))


def scoring_case(n_items=400):
    """300 users for set_neighbours lists of any K up to 256.  User 0 has nothing, users 1..5 have rows of 1, 63, 64, 65 and
    200 items, users 20..79 all have item 6 (one item reached through up to 60 neighbours), nobody has the last item"""
    n_users = 300
    rs = np.random.RandomState(34)
    rows = [[], [17]] + [rs.choice(n_items - 1, n, replace=False) for n in (63, 64, 65, 200)]
    while len(rows) < n_users:
        u = len(rows)
        r = list(rs.choice(n_items - 1, rs.randint(0, 30), replace=False))
        rows.append(r + [6] if 20 <= u < 80 else r)
    return csr_of_rows(rows, n_items)


def scoring_edge_case(n_items):
    """80 users over a catalogue at a scoring slice edge: user 1 straddles the first edge, user 2 has nothing in slice 0 (where
    there is a second slice), user 3 only the first 100 items, user 4 the columns next to every edge and the last item, the
    others a dozen items and three of those columns"""
    w = w_score()
    rs = np.random.RandomState(35)
    marks = sorted({c for m in range(0, n_items + w, w) for c in (m - 1, m, m + 1) if 0 <= c < n_items} | {0, n_items - 1})
    rows = [[], [c for c in range(w - 40, w + 40) if c < n_items],
            list(range(w, n_items)) if n_items > w else [n_items - 1], list(range(100)), marks]
    while len(rows) < 80:
        rows.append(list(rs.randint(0, n_items, 12)) + list(rs.choice(marks, 3)))
    return csr_of_rows(rows, n_items)


def constructed_lists(n_users, K, seed=36):
    """neighbour lists that no fit gave (IC.constructed_lists over users: random distinct non-self ids, float32 scores of both
    signs, every fill from empty to full), then by hand: row 8 reaches item 6 through users 20.. with scores of either sign
    and magnitudes from 1e-3 to 1e8, so any other order of the adds changes the bits; row 7 holds 1, 1e8, -1e8 (0 in this
    order, 1 backwards); row 9 has nobody; row 13 names the empty user 0 and has a padding slot between kept ones"""
    nb, sc = IC.constructed_lists(n_users, K, seed)
    rs = np.random.RandomState(seed + 1)
    n = min(K, 60)
    nb[8], sc[8] = -1, -np.inf
    nb[8, :n] = 20 + rs.permutation(60)[:n]
    sc[8, :n] = (rs.choice([-1.0, 1.0], n) * 10.0 ** rs.uniform(-3, 8, n)).astype(np.float32)
    for row, ids, vals in ((7, [20, 21, 22], [1.0, 1e8, -1e8]), (9, [], []), (13, [0, 1, -1, 2], [0.5, 0.25, -np.inf, 2.0])):
        nb[row], sc[row] = -1, -np.inf
        nb[row, :len(ids)] = ids
        sc[row, :len(ids)] = vals
    return nb, sc


CASES = {"lengths": lengths_case, "sparse_lengths": sparse_lengths_case, "scoring": scoring_case,
         "full_user": lambda: IC.full_user_case(), "ties": lambda: transpose(IC.ties_case()),
         "big": lambda: transpose(IC.big_case()), "planted": lambda: IC.planted_case()[0]}


@functools.lru_cache(maxsize=None)
def case(name):
    """a named case, "edge:<n_users>" or "score_edge:<n_items>"; built once"""
    if name.startswith("edge:"):
        return edge_case(int(name.split(":")[1]))
    if name.startswith("score_edge:"):
        return scoring_edge_case(int(name.split(":")[1]))
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def fitted(name, K, metric="cosine", shrink=0.0):
    return R.fit(*case(name), K, metric, shrink)


@functools.lru_cache(maxsize=None)
def scores_of(name, K, metric="cosine", shrink=0.0):
    """the float32 score rows of every user of a fitted case, computed when first asked for"""
    indptr, items, nu, ni = case(name)
    nb, sc = fitted(name, K, metric, shrink)

    @functools.lru_cache(maxsize=None)
    def row(u):
        return R.user_scores(nb[u], sc[u], indptr, items, ni)
    return row
