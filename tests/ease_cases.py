"""The constructed inputs of tests/test_gpu_ease.py and tests/test_ease_host.py, with cached restatements of them
(tests/ease_ref.py).  Each builder names the edge it is there for; the block size, the update tile, the scoring width and
the look-ahead come from tfr_ease_plan, so the cases move with the launchers."""
import functools

import numpy as np

from tests import ease_ref as R
from tests import itemknn_cases as IC
from tfrecomm_amd import ease as E

LAMBDAS = (0.01, 0.5, 10.0, 500.0)
COND_MAX = 1e6


def nb():
    return E.plan(100)["nb"]


def tile():
    return E.plan(100)["tile"]


def w_score():
    return E.plan(100, 10, 1, 1)["width"]


def ahead():
    return E.plan(100, 10, 1, 1)["ahead"]


def sized_case(n_items, n_users=80, seed=31):
    """a random pattern over a catalogue of a given size: about a sixth of the entries, the popular items first"""
    rs = np.random.RandomState(seed + n_items)
    p = np.clip(0.5 / np.sqrt(1.0 + np.arange(n_items)), 0.04, 1.0)
    rows = [np.flatnonzero(rs.random_sample(n_items) < p) for _ in range(n_users)]
    return IC.csr_of_rows(rows, n_items)


def gram_case_names():
    """item lists of 0, 1, 63, 64, 65, 255, 256 and 257 users and an item every user has ("lengths"), a user with every item
    ("full_user"), catalogues of 1, 2, NB - 1, NB, NB + 1 and 2 NB + 3 items"""
    return ["lengths", "full_user"] + ["size:%d" % n for n in (1, 2, nb() - 1, nb(), nb() + 1, 2 * nb() + 3)]


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("size:"):
        return sized_case(int(name.split(":")[1]))
    return IC.case(name)


@functools.lru_cache(maxsize=None)
def gram(name, lam):
    indptr, items, nu, ni = case(name)
    g = R.gram(indptr, items, nu, ni, lam)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def inverse_case(name, lam):
    """(G, P long double, cond2(G)) of one Gram matrix"""
    g = gram(name, lam)
    p = R.inverse_ld(g)
    p.setflags(write=False)
    return g, p, float(np.linalg.cond(g))


@functools.lru_cache(maxsize=None)
def inverse_cases():
    """the (name, lambda) pairs whose Gram matrix has cond2 <= COND_MAX"""
    return tuple((name, lam) for name in gram_case_names() for lam in LAMBDAS if inverse_case(name, lam)[2] <= COND_MAX)


@functools.lru_cache(maxsize=None)
def error_constant():
    """(r_max, K): r_max = the largest ratio max|P_blocked - P_ld| / (eps cond2(G) max|P_ld|) of the float64 restatement
    of the device's order over the inverse cases; K = 8 r_max bounds the device (the factor covers fma
    contraction and the MFMA's internal order, which NumPy cannot mirror)"""
    r_max = 0.0
    for name, lam in inverse_cases():
        g, p_ld, cond = inverse_case(name, lam)
        r_max = max(r_max, R.error_ratio(R.inverse_blocked(g, nb()), p_ld, cond))
    return r_max, 8.0 * r_max


def integer_case(n, split, seed=32):
    """(G, P) with G = L L^T, L = I + N, N integer in [-2, 2] at rows > split and columns <= split only: N N = 0, so
    L^-1 = I - N, P = (I - N)^T (I - N), and every intermediate of the factorisation is a small integer"""
    rs = np.random.RandomState(seed + n)
    N = np.zeros((n, n))
    N[split + 1:, :split + 1] = rs.randint(-2, 3, (n - split - 1, split + 1))
    assert not np.array_equal(N, N.T) and not (N @ N).any()
    L = np.eye(n) + N
    M = np.eye(n) - N
    return L @ L.T, M.T @ M


def indefinite_case(n=70, at=66):
    """a symmetric matrix with a positive diagonal and one negative eigenvalue: identity plus a 2 x 2 block [[1, 2], [2, 1]]
    at (at, at + 1); the pivot of column at + 1 is 1 - 4 = -3"""
    g = np.eye(n)
    g[at, at + 1] = g[at + 1, at] = 2.0
    return g


def planted_case(n_users=300, n_items=150, n_clusters=5, seed=33):
    """300 users x 150 items in 5 clusters: a user draws most items from its cluster; (train CSR, test users, test items)"""
    rs = np.random.RandomState(seed)
    per = n_items // n_clusters
    train, tu, ti = [], [], []
    for u in range(n_users):
        c = u % n_clusters
        own = c * per + rs.choice(per, 12, replace=False)
        other = rs.choice(n_items, 3, replace=False)
        train.append(list(own[:9]) + list(other))
        held = [i for i in own[9:] if i not in set(other)]
        tu += [u] * len(held)
        ti += held
    return IC.csr_of_rows(train, n_items), np.asarray(tu, np.int32), np.asarray(ti, np.int32)


def constructed_weights(n_items, seed=34):
    """weights no fit gave: float32 multiples of 1/8 in [-2, 2] (sums of a few are exact, so equal sums tie exactly and go
    by id), a zero diagonal, and three runs of identical columns"""
    rs = np.random.RandomState(seed + n_items)
    B = (rs.randint(-16, 17, (n_items, n_items)) / 8.0).astype(np.float32)
    for lo in (0, n_items // 2, max(0, n_items - 9)):
        B[:, lo:lo + 9] = B[:, lo:lo + 1]
    np.fill_diagonal(B, np.float32(0))
    return B


def ladder(n_items, seed=35):
    """query lists of 0, 1, ahead - 1, ahead, ahead + 1, 2 ahead + 1 and 40 items, three of each"""
    rs = np.random.RandomState(seed)
    a = ahead()
    lens = [0, 1, a - 1, a, a + 1, 2 * a + 1, 40] * 3
    return IC.csr_of_rows([rs.choice(n_items, min(n, n_items), replace=False) for n in lens], n_items)


def twin_case(n_items=1025, K=4, seed=36):
    """one model spelt both ways, for the two scoring tails to be held against each other: ItemKNN neighbour lists (nb, sc)
    of every fill whose scores are multiples of 1/8 in [-2, 2] - the sums of a few are exact in any order - and the dense
    weights they spell out, B[i, nb[i, c]] = sc[i, c] and +0 elsewhere.  1025 items: one ItemKNN scoring slice, two of EASE."""
    rs = np.random.RandomState(seed)
    nb = np.full((n_items, K), -1, np.int32)
    sc = np.full((n_items, K), -np.inf, np.float32)
    B = np.zeros((n_items, n_items), np.float32)
    for i in range(n_items):
        cand = rs.choice(n_items - 1, rs.randint(0, K + 1), replace=False)
        cand = cand + (cand >= i)                          # skip i itself
        nb[i, :cand.size] = cand
        sc[i, :cand.size] = (rs.randint(-16, 17, cand.size) / 8.0).astype(np.float32)
        B[i, cand] = sc[i, :cand.size]
    return nb, sc, B
