"""NumPy statement of the nearest-neighbour contract (include/tfrecomm.h tfr_neighbours): one table T [R, D] gives the query
rows and the candidate rows; dot(a, b) is the f32 fmaf chain over f ascending from +0, cosine (dot * rn[a]) * rn[b] with
rn = 1 / sqrtf(ss), ss the same chain of the squares and rn = 0 for a zero row; order by score descending, then row id
ascending (the top-K key); the query row, its excluded rows and NaN scores are never returned; id -1 / score -inf past the
eligible candidates; candidates restricted to rows [lo, hi), ids always row ids of T."""
import numpy as np

from tests.topk_ref import ordered_u32


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product of two f32 is exact in float64, the sum is rounded to float64 and then to
    f32.  Equal to the single rounding of a true fmaf except on double-rounding ties (none on the dyadic tables the exact
    tests use, about one step in 2^29 otherwise)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def table_rows(T, item_abs=False):
    T = np.ascontiguousarray(T, np.float32)
    return np.abs(T) if item_abs else T


def chain_dot(A, B):
    """[n, D] x [R, D] -> f32 [n, R]: every pair's fmaf chain over f = 0..D-1 ascending from +0."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for f in range(A.shape[1]):
        acc = _fma32(A[:, f][:, None], B[:, f][None, :], acc)
    return acc


def row_rnorm(T):
    """rn [R] f32: 1 / sqrt(ss) with both operations rounded to f32, 0 where ss == 0."""
    T = np.asarray(T, np.float32)
    ss = np.zeros(T.shape[0], np.float32)
    for f in range(T.shape[1]):
        ss = _fma32(T[:, f], T[:, f], ss)
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = (np.float32(1) / np.sqrt(ss, dtype=np.float32)).astype(np.float32)
    return np.where(ss == 0, np.float32(0), rn).astype(np.float32)


def neighbour_scores(T, rows, metric="cosine", item_abs=False):
    """f32 [n, R] scores of the query rows against every row of T (the self pair included)."""
    Tp = table_rows(T, item_abs)
    rows = np.asarray(rows, np.int64)
    S = chain_dot(Tp[rows], Tp)
    if metric == "dot":
        return S
    if metric != "cosine":
        raise ValueError("metric must be 'dot' or 'cosine'")
    rn = row_rnorm(Tp)
    with np.errstate(invalid="ignore", over="ignore"):
        S = (S * rn[rows][:, None]).astype(np.float32)
        return (S * rn[None, :]).astype(np.float32)


def neighbours_from_scores(S, rows, k, excl=None, lo=0, hi=None):
    """S f32 [n, R] -> (ids int32 [n, k], scores f32 [n, k]) under the ordering, masking and padding rules."""
    S = np.asarray(S, np.float32)
    n, R = S.shape
    hi = R if hi is None else hi
    ids = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), -np.inf, np.float32)
    for r in range(n):
        ok = ~np.isnan(S[r])
        ok[:lo] = False
        ok[hi:] = False
        ok[int(rows[r])] = False
        if excl is not None and len(excl[r]):
            ok[np.asarray(excl[r], np.int64)] = False
        cand = np.flatnonzero(ok)
        o = ordered_u32(S[r, cand]).astype(np.int64)
        order = np.lexsort((cand, -o))[:k]
        ids[r, :order.size] = cand[order]
        scores[r, :order.size] = S[r, cand[order]]
    return ids, scores


def neighbours_ref(T, rows, k, metric="cosine", excl=None, lo=0, hi=None, item_abs=False):
    """T [R, D]; rows the query row ids; excl None or a list of n arrays of row ids.  Returns (ids, scores)."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    return neighbours_from_scores(neighbour_scores(T, rows, metric, item_abs), rows, k, excl, lo, hi)


def scores_f64(T, rows, metric="cosine", item_abs=False):
    """The brute-force float64 scores [n, R]; a zero row's cosine is 0."""
    T64 = np.abs(np.asarray(T, np.float64)) if item_abs else np.asarray(T, np.float64)
    rows = np.asarray(rows, np.int64)
    S = T64[rows] @ T64.T
    if metric == "cosine":
        nrm = np.sqrt((T64 * T64).sum(1))
        inv = np.where(nrm == 0, 0.0, 1.0 / np.where(nrm == 0, 1.0, nrm))
        S = S * inv[rows][:, None] * inv[None, :]
    return S


def dyadic_table(rs, R, D):
    """entries k / 8, |k| <= 8: every product and every partial sum of a dot is exact in f32 (and in float64)."""
    return (rs.randint(-8, 9, (R, D)) * 0.125).astype(np.float32)


def pow4_table(rs, R, D):
    """each row: 4^m entries of one magnitude 2^-j (signs free), the rest 0 - ss is a power of four, rn a power of two, so the
    cosine is exact as well"""
    t = np.zeros((R, D), np.float32)
    ms = [m for m in range(5) if 4 ** m <= D]
    for r in range(R):
        cnt = 4 ** ms[rs.randint(len(ms))]
        cols = rs.choice(D, cnt, replace=False)
        t[r, cols] = rs.choice([-1.0, 1.0], cnt) * 2.0 ** -rs.randint(0, 4)
    return t
