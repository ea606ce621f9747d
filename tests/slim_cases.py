"""The constructed inputs of tests/test_gpu_slim.py and tests/test_slim_host.py, with cached restatements of them
(tests/slim_ref.py).  The patterns are those of tests/itemknn_cases.py and tests/ease_cases.py where they fit; the window and
the grid come from tfr_slim_plan, so the cases move with the launcher."""
import functools

import numpy as np

from tests import ease_cases as EC
from tests import itemknn_cases as IC
from tests import slim_ref as R
from tfrecomm_amd import slim as S

PENALTIES = ((0.0, 0.0), (0.5, 1.0), (2.0, 5.0))           # (l1, beta)
planted_case = EC.planted_case
constructed_weights = EC.constructed_weights
ladder = EC.ladder


def window():
    return S.plan(100)["window"]


@functools.lru_cache(maxsize=None)
def stride_items():
    """the smallest catalogue with more columns than the solver's grid, and two more: three columns are a second stride"""
    n = 1
    while S.plan(n)["grid"] >= n:
        n += 1
    return n + 2


def duplicates_case(n_users=80, seed=37):
    """40 random item columns, each of them twice (items i and i + 40 have the same users), and item 80 as item 3 once more"""
    indptr, items, nu, _ = EC.sized_case(40, n_users, seed)
    rows = []
    for r in IC.rows_of(indptr, items, range(nu)):
        r = np.asarray(r, np.int64)
        rows.append(np.concatenate([r, r + 40, np.full(int((r == 3).sum()), 80)]))
    return IC.csr_of_rows(rows, 81)


# Catalogues of 1, 2, T - 1, T, T + 1 and 2 T + 3 items over 80 users (T = the window; the names are resolved when a case is
# built, so listing them loads no library), item lists of every length with an item nobody has and one everybody has
# ("lengths"), a user with every item ("full_user"), duplicate columns ("duplicates").
SIZES = {"size:1": lambda t: 1, "size:2": lambda t: 2, "size:T-1": lambda t: t - 1, "size:T": lambda t: t,
         "size:T+1": lambda t: t + 1, "size:2T+3": lambda t: 2 * t + 3}
BIT_CASES = tuple(SIZES) + ("lengths", "full_user", "duplicates")


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SIZES:
        return EC.sized_case(SIZES[name](window()))
    if name == "duplicates":
        return duplicates_case()
    if name == "stride":
        return EC.sized_case(stride_items(), n_users=60)
    return EC.case(name)


@functools.lru_cache(maxsize=None)
def gram(name, beta):
    indptr, items, nu, ni = case(name)
    g = R.gram(indptr, items, nu, ni, beta)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def solved(name, l1, beta, positive, max_iter, tol):
    """(W, sweeps, updates, converged, W64) of the restatement on a named case"""
    out = R.solve(gram(name, beta), l1, positive, max_iter, tol)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def planted_gram(beta):
    (indptr, items, nu, ni), _, _ = planted_case()
    g = R.gram(indptr, items, nu, ni, beta)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def planted_solved(l1, beta, positive=True, max_iter=200, tol=1e-4):
    out = R.solve(planted_gram(beta), l1, positive, max_iter, tol)
    for a in out:
        a.setflags(write=False)
    return out
