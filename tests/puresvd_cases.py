"""The cases of tests/test_puresvd_host.py and tests/test_gpu_puresvd.py.  Shapes follow tfr_psvd_plan (``plan()``): the list
lengths sit at the edges of the id load (64), of the look-ahead and of the chunk, the widths at both ends of every lane
count, with the widths where the lane masks change.  Everything is made once per process and left unchanged."""
import functools

import numpy as np

from tests import list_paths as LP
from tests import puresvd_ref as R


@functools.lru_cache(None)
def plan(factors=64, oversample=16, n_users=6040, n_items=3706):
    from tfrecomm_amd import puresvd
    return puresvd.plan(n_users, n_items, factors, oversample)


def lane_edges():
    """{lanes: (narrowest r, widest r)} from the plan itself: one entry, a whole wave takes a row at every width"""
    out = {}
    for r in range(1, 129):
        lanes = plan(r, 0)["lanes"]
        lo, hi = out.get(lanes, (r, r))
        out[lanes] = (min(lo, r), max(hi, r))
    return out


def product_widths():
    """both ends of the compiled lane count, odd and even widths, and the widths at which a sixteenth, a quarter and a half of
    the wave's lanes own columns, with their neighbours: the masks are what differs between widths"""
    w = {2, 7, 32, 33, 64, 65, 127}
    for lo, hi in lane_edges().values():
        w |= {lo, hi}
    return sorted(w)


def product_lengths():
    p = plan()
    ch, ah = p["chunk"], p["ahead"]
    return [0, 1, 63, 64, 65, ah - 1, ah + 1, ch - 1, ch, ch + 1, 2 * ch + 1]


@functools.lru_cache(None)
def product_lists():
    """(indptr, ids, n_rows, n_cols): one row per length of product_lengths(), then a crowd of 40 short rows; ids ascending"""
    rs = np.random.RandomState(11)
    lengths = product_lengths() + [int(v) for v in rs.randint(0, 30, 40)]
    n_cols = 2 * plan()["chunk"] + 40
    rows = [np.sort(rs.choice(n_cols, n, replace=False)).astype(np.int32) for n in lengths]
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), len(lengths), n_cols


@functools.lru_cache(None)
def product_block(n, r):
    """entries of mixed sign and magnitude: any other order of the adds changes bits"""
    rs = np.random.RandomState(100 + r)
    vals = np.array([1e16, 1.0, -1e16, 3.0, -1.0, 2.0 ** -30, 1e8 + 1, -1e8, 0.1, -0.3])
    B = vals[rs.randint(0, vals.size, (n, r))] * (1 + rs.randint(0, 8, (n, r)) * 2.0 ** -50)
    B.setflags(write=False)
    return B


def as_matrix(indptr, ids, n_rows, n_cols, transpose=False):
    """the lists as the user x item CSR a handle loads: as they are (the rows are the users), or transposed (the rows are the
    items' lists of a matrix with n_cols users)"""
    if not transpose:
        return (indptr, ids), n_rows, n_cols
    tptr, tids = R.transpose_lists(indptr, ids, n_rows, n_cols)
    return (tptr, tids), n_cols, n_rows


# ----------------------------------------------------------------------------- orthonormalise
ORTH_SHAPES = {"narrow": (200, 5), "tiled": (300, 24), "one": (140, 1), "odd": (270, 37), "wide": (260, 128)}


@functools.lru_cache(None)
def orth_block(name):
    """float32 values in float64 (tests/puresvd_ref.py on the Gram's products), columns scaled by powers of two and mixed so
    that cond2(S) is a few thousand"""
    n, r = ORTH_SHAPES[name]
    rs = np.random.RandomState(len(name) * 7 + r)
    Z = rs.standard_normal((n, r)).astype(np.float32).astype(np.float64)
    if r > 1:
        Z[:, 1] = (Z[:, 0] + 0.125 * Z[:, 1]).astype(np.float32)
    Z = Z * (2.0 ** rs.randint(-3, 4, r))[None, :]
    assert np.array_equal(Z, Z.astype(np.float32))
    Z.setflags(write=False)
    return Z


def repeated_column_block():
    Z = np.array(orth_block("tiled"))
    Z[:, 9] = Z[:, 4]
    return Z


# ----------------------------------------------------------------------------- eigen step
EIG_SIZES = LP.PSVD_EIG_SIZES                             # tests/list_paths.py says what each size is there for


@functools.lru_cache(None)
def eig_input(kind, r):
    rs = np.random.RandomState(1000 + r)
    if kind == "diagonal":
        T = np.diag(rs.permutation(r) + 1.0)
    elif kind == "planted":                                # a repeated and a zero eigenvalue where r allows
        Q0, _ = np.linalg.qr(rs.standard_normal((r, r)))
        lam = np.sort(rs.uniform(1, 100, r))[::-1].copy()
        if r >= 3:
            lam[1] = lam[0]
            lam[-1] = 0.0
        T = (Q0 * lam[None, :]) @ Q0.T
        T = (T + T.T) / 2
    else:
        raise KeyError(kind)
    T.setflags(write=False)
    return T


# ----------------------------------------------------------------------------- fits
BLOCKS = ((12, 9), (7, 8), (5, 5), (3, 4), (2, 2))
BLOCK_FIT = dict(factors=3, oversample=2, iterations=6)
RANDOM_FIT = dict(factors=8, oversample=16, iterations=8)


@functools.lru_cache(None)
def block_case():
    """disjoint all-ones blocks: sigma_k^2 = a_k b_k, right vectors the block indicators over sqrt(b_k)"""
    nu, ni = sum(a for a, _ in BLOCKS), sum(b for _, b in BLOCKS)
    rows, u0, i0 = [], 0, 0
    Q = np.zeros((ni, len(BLOCKS)))
    for k, (a, b) in enumerate(BLOCKS):
        rows += [np.arange(i0, i0 + b, dtype=np.int32)] * a
        Q[i0:i0 + b, k] = 1 / np.sqrt(b)
        u0, i0 = u0 + a, i0 + b
    indptr = np.concatenate(([0], np.cumsum([x.size for x in rows]))).astype(np.int64)
    return dict(nu=nu, ni=ni, indptr=indptr, items=np.concatenate(rows), sigma2=np.array([a * b for a, b in BLOCKS], np.float64), Q=Q)


@functools.lru_cache(None)
def random_case():
    """70 x 90 with 900 distinct Zipf pairs"""
    nu, ni, nnz = 70, 90, 900
    rs = np.random.RandomState(5)
    w = 1.0 / np.arange(1, ni + 1)
    seen = set()
    while len(seen) < nnz:
        u, i = int(rs.randint(nu)), int(rs.choice(ni, p=w / w.sum()))
        seen.add((u, i))
    pairs = np.array(sorted(seen))
    indptr = np.searchsorted(pairs[:, 0], np.arange(nu + 1)).astype(np.int64)
    return dict(nu=nu, ni=ni, indptr=indptr, items=pairs[:, 1].astype(np.int32))


WIDE_FIT = dict(factors=LP.PSVD_WIDE_FIT[0], oversample=LP.PSVD_WIDE_FIT[1], iterations=4)


@functools.lru_cache(None)
def wide_case():
    """300 x 280 at density 0.15: user 1 and item 1 are empty; user 0 has every other item (279) and item 0 is held by every
    other user (299), so both lists are longer than the chunk and are cut inside a fit; both sides take several Gram slices"""
    nu, ni = 300, 280
    X = np.random.RandomState(6).random_sample((nu, ni)) < 0.15
    X[0, :] = True
    X[:, 0] = True
    X[1, :] = False
    X[:, 1] = False
    rows, cols = np.nonzero(X)
    indptr = np.searchsorted(rows, np.arange(nu + 1)).astype(np.int64)
    return dict(nu=nu, ni=ni, indptr=indptr, items=cols.astype(np.int32))


def dense(case):
    X = np.zeros((case["nu"], case["ni"]))
    X[np.repeat(np.arange(case["nu"]), np.diff(case["indptr"])), case["items"]] = 1
    return X


def start_block(case, fit, seed=0):
    return np.random.RandomState(seed).standard_normal((case["ni"], fit["factors"] + fit["oversample"]))


@functools.lru_cache(None)
def fit_ref(which, dtype=np.float64):
    case, fit = {"block": (block_case(), BLOCK_FIT), "random": (random_case(), RANDOM_FIT), "wide": (wide_case(), WIDE_FIT)}[which]
    return R.fit(case["indptr"], case["items"], case["nu"], case["ni"], fit["factors"], fit["oversample"], fit["iterations"],
                 start_block(case, fit), plan()["chunk"], dtype)


def block_exact():
    """(sigma^2, Q, P) of the block case's three factors"""
    case, f = block_case(), BLOCK_FIT["factors"]
    Q = case["Q"][:, :f]
    return case["sigma2"][:f], Q, dense(case) @ Q


def block_ratios(sigma, Q, P):
    """the errors of a fit of the block case against the exact answer, in units of eps times the largest exact entry.  The sign
    rule is the eigen step's, on Qe; the sign of a column of Q = V Qe follows the start block, so column k of Q and of P is
    compared under the one sign that makes Q's entry at the block's first item positive."""
    s2, Qx, Px = block_exact()
    sign = np.sign(Q[np.abs(Qx).argmax(0), np.arange(Q.shape[1])])[None, :]
    return (float(np.abs(sigma.astype(R.LD) ** 2 - s2).max() / s2.max()) / R.EPS,
            float(np.abs((sign * Q).astype(R.LD) - Qx).max() / Qx.max()) / R.EPS,
            float(np.abs((sign * P).astype(R.LD) - Px).max() / Px.max()) / R.EPS)
