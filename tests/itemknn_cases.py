"""The constructed interaction matrices of tests/test_gpu_itemknn.py, as (indptr int64, items int32, n_users, n_items), and
cached restatements of them (tests/itemknn_ref.py).  Each builder names the edge it is there for; the slice widths come from
tfr_knn_plan, so the cases move with the launchers."""
import functools

import numpy as np

from tests import itemknn_ref as R
from tfrecomm_amd import itemknn as IK


def csr_of_rows(rows, n_items):
    """rows: a list of iterables of item ids -> (indptr, items, n_users, n_items) with sorted, distinct rows"""
    rows = [np.unique(np.asarray(list(r), np.int64)) for r in rows]
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    items = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return indptr, items, len(rows), int(n_items)


def csr_of_item_lists(lists, n_users, n_items):
    """lists: {item: users} -> the user CSR"""
    rows = [[] for _ in range(n_users)]
    for i, users in lists.items():
        for u in users:
            rows[u].append(i)
    return csr_of_rows(rows, n_items)


def w_fit(K=10):
    return IK.plan(100, K, 100, 0)["width"]


def w_score(k=10):
    return IK.plan(100, k, 1, 1)["width"]


def lengths_case():
    """Item lists of 0, 1, 63, 64, 65 users (the 64 row bounds a wave loads at once), 255, 256, 257 (the block's four waves),
    an item every user has, and 130 items in all, so K = 256 pads every row"""
    n_users, n_items = 300, 130
    rs = np.random.RandomState(11)
    lists = {1: [7], 2: range(63), 3: range(100, 164), 4: range(30, 95), 5: range(255), 6: range(256), 7: range(20, 277),
             8: range(n_users)}                            # item 0: nobody
    for i in range(9, n_items):
        lists[i] = rs.choice(n_users, rs.randint(1, 40), replace=False)
    return csr_of_item_lists(lists, n_users, n_items)


def full_user_case():
    """one user has every item (every pair co-occurs, every row is full), the others a few"""
    n_users, n_items = 60, 90
    rs = np.random.RandomState(12)
    rows = [rs.choice(n_items, rs.randint(0, 12), replace=False) for _ in range(n_users)]
    rows[17] = np.arange(n_items)
    return csr_of_rows(rows, n_items)


def edge_case(n_items, seed=13, n_users=400, per_user=12):
    """a sparse matrix over a catalogue at a slice edge; the columns next to every multiple of the fit and scoring widths that
    exist are co-rated, so the first and last counter of a slice are used"""
    rs = np.random.RandomState(seed)
    marks = sorted({c for w in (w_score(), w_fit()) for m in range(0, n_items + w, w) for c in (m - 1, m, m + 1)
                    if 0 <= c < n_items} | {0, n_items - 1})
    rows = []
    for u in range(n_users):
        r = list(rs.randint(0, n_items, per_user))
        r += list(rs.choice(marks, 3))
        rows.append(r)
    return csr_of_rows(rows, n_items)


def ties_case():
    """8 blocks of 25 items; every user of a block has the whole block: inside a block all pairs tie exactly, the id decides"""
    n_items, block, users_per = 200, 25, 6
    rows = []
    for b in range(n_items // block):
        rows += [range(b * block, (b + 1) * block)] * users_per
    rows.append([3, 30, 60])                               # and a few links between blocks, weaker than the ties
    rows.append([3, 31])
    return csr_of_rows(rows, n_items)


def staircase_case(n_items=2304, step=64):
    """user t has item 0 and every item from step * t on: c(0, j) = j // step + 1 rises along the catalogue, and so do the
    cosine and the jaccard of (0, j).  Every 64 columns a wave scans beat all it has kept: its queue fills and is sort-cut
    again and again, at either queue size"""
    rows = [[0] + list(range(step * t, n_items)) for t in range(n_items // step)]
    return csr_of_rows(rows, n_items)


def big_case():
    """70 000 items with about two users each: more rows than one chunk and than the grid"""
    n_users, n_items, per_user = 7000, 70000, 20
    rs = np.random.RandomState(14)
    return csr_of_rows([rs.randint(0, n_items, per_user) for _ in range(n_users)], n_items)


def planted_case():
    """300 users x 200 items in 5 clusters: a user draws most items from its cluster; returns (train CSR, test pairs)"""
    n_users, n_items, n_clusters = 300, 200, 5
    rs = np.random.RandomState(15)
    per = n_items // n_clusters
    train, tu, ti = [], [], []
    for u in range(n_users):
        c = u % n_clusters
        own = c * per + rs.choice(per, 14, replace=False)
        other = rs.choice(n_items, 3, replace=False)
        train.append(list(own[:10]) + list(other))
        held = [i for i in own[10:] if i not in set(other)]
        tu += [u] * len(held)
        ti += held
    return csr_of_rows(train, n_items), np.asarray(tu, np.int32), np.asarray(ti, np.int32)


CASES = {"lengths": lengths_case, "full_user": full_user_case, "ties": ties_case, "staircase": staircase_case, "big": big_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """a named case, or "edge:<n_items>"; built once"""
    if name.startswith("edge:"):
        return edge_case(int(name.split(":")[1]))
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def counts(name):
    indptr, items, nu, ni = case(name)
    return R.cooccurrence(indptr, items, nu, ni)


@functools.lru_cache(maxsize=None)
def fitted(name, K, metric, shrink):
    c, n = counts(name)
    return R.fit(c, n, K, metric, shrink)


def rows_of(indptr, items, users):
    return [items[indptr[u]:indptr[u + 1]] for u in users]


def sub_csr(indptr, items, users):
    """the rows `users` of a CSR as a CSR of their own"""
    rows = rows_of(indptr, items, users)
    p = np.zeros(len(rows) + 1, np.int64)
    p[1:] = np.cumsum([r.size for r in rows])
    return p, (np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32))


def constructed_lists(n_items, K, seed=16):
    """neighbour lists that no fit gave: random distinct non-self ids with random float32 scores (negative ones too), rows
    of every fill from empty to full, -1 padding after the kept ones"""
    rs = np.random.RandomState(seed)
    nb = np.full((n_items, K), -1, np.int32)
    sc = np.full((n_items, K), -np.inf, np.float32)
    for i in range(n_items):
        fill = rs.randint(0, K + 1)
        cand = rs.choice(n_items - 1, min(fill, n_items - 1), replace=False)
        cand = cand + (cand >= i)                          # skip i itself
        nb[i, :cand.size] = cand
        sc[i, :cand.size] = rs.normal(0, 1, cand.size).astype(np.float32)
    return nb, sc
