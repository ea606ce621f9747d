"""Shared inputs of the FM snapshot tests (tests/test_fm_bf16_host.py, tests/test_gpu_fm_bf16.py), as plain seeded data, and a
float32 NumPy restatement of csrc/fm_bf16.hip's order of operations.

Every design holds, among rows of 1 .. 9 entries: an empty row and rows of 1, 3, 4, 5, 8 and 9 entries (the kernel walks a
row four entries at a time: one short, one full, one over, two full, two over), a row of fm_cases.LONG_ROW entries, a column
twice in one row, an explicit zero, negative and fractional values, features 0 and F - 1, and n no multiple of the rows a
block owns (256 / G)."""
import functools

import numpy as np

from tfrecomm_amd import bf16
from tests import fm_cases as C
from tests import fm_ref as FR
from tests import step_ref as R
from tests import widths as W

F4 = np.float32
WIDTHS = W.BF16_PNT                       # all ten (lanes per row G, the group is wider than the row) classes
F, N = 400, 701
EDGE_LENS = (0, 1, 3, 4, 5, 8, 9, C.LONG_ROW)
GRID_CAP = 8192                           # csrc/fm_bf16.hip fm_bf16_grid: blocks of a launch; further rows by the grid stride
TOPK_WIDTHS = (25, 64, 200)               # D % 8 != 0, D % 8 == 0, a width above 128


def lanes(D):
    return bf16.lanes(D)


@functools.lru_cache(maxsize=None)
def tables(D, seed=0):
    """(mu, W, V) at the scale of fm_cases.tables_of"""
    rs = np.random.RandomState(1000 * seed + D)
    out = (F4(0.1), rs.normal(0, 0.1, F).astype(F4), rs.normal(0, 0.1 / np.sqrt(max(D, 16) / 16), (F, D)).astype(F4))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _values(rs, k):
    v = rs.randint(1, 4, k).astype(F4)
    return np.where(rs.rand(k) < 0.33, rs.normal(0, 1, k), v).astype(F4)


@functools.lru_cache(maxsize=None)
def design(seed=0, n=N):
    """(indptr, indices, data), read-only"""
    rs = np.random.RandomState(77 + seed)
    lens = rs.randint(1, 10, n)
    lens[:len(EDGE_LENS)] = EDGE_LENS
    rows = []
    for r in range(n):
        k = int(lens[r])
        cols, vals = rs.randint(0, F, k), _values(rs, k)
        if lens[r] == C.LONG_ROW:
            cols = rs.choice(F, k, replace=False)
        elif r == 8:                                      # a column twice in one row
            cols, vals = np.array([7, 7, 9]), np.array([2.0, -0.75, 1.0], F4)
        elif r == 9:                                      # an explicit zero
            cols, vals = np.array([11, 12, 13]), np.array([1.0, 0.0, 3.0], F4)
        elif r == 10:                                     # both ends of the table
            cols, vals = np.array([F - 1, 0, 5, 123]), np.array([1.0, 2.0, -1.5, 0.25], F4)
        rows.append((cols, vals))
    out = (np.concatenate(([0], np.cumsum([len(c) for c, _ in rows]))).astype(np.int64),
           np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([v for _, v in rows]).astype(F4))
    got = set(np.diff(out[0]).tolist())
    assert set(EDGE_LENS) <= got and all(n % (256 // g) for g in (2, 4, 8, 16, 32)) and n > 256
    assert (out[2] == 0).any() and (out[2] < 0).any() and (out[2] != np.round(out[2])).any()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stride_design(G):
    """more rows than one grid pass of the G-lane kernel owns (GRID_CAP blocks of 256 / G rows), two entries each, F = 40"""
    n = GRID_CAP * (256 // G) + 37
    rs = np.random.RandomState(5 + G)
    return np.arange(n + 1, dtype=np.int64) * 2, rs.randint(0, 40, 2 * n).astype(np.int32), _values(rs, 2 * n)


# ---------------------------------------------------------------- the kernel's order, in float32 NumPy
def _fma32(a, b, c):
    """fmaf through float64: the product of two float32 is exact there, the sum rounds once and then once more"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F4)


def kernel_f32(mu, Wt, V, indptr, indices, data):
    """k_fm_forward_bf16 on V as given (float32 values that are exactly bf16: what widening the snapshot yields): G lanes
    per row, lane l owns elements 8 l .. 8 l + 7 of the padded row; per entry in CSR order xv = x * v, s += xv,
    q = fmaf(xv, xv, q), lin = fmaf(x, w, lin); then per lane sum_e (s_e^2 - q_e) over e ascending, the lanes past DP / 8
    replaced by 0, a butterfly over the G lanes, y = (mu + lin) + 0.5 * acc.  It differs from k_fm_forward's order only in
    the lane geometry.  (The entries the four-at-a-time walk pads a row with carry x = 0 and change nothing: not restated.)"""
    mu, Wt, V = F4(mu), np.asarray(Wt, F4), np.asarray(V, F4)
    D = V.shape[1]
    DP, G = bf16.row_stride(D), bf16.lanes(D)
    Vp = np.zeros((V.shape[0], G * 8), F4)                 # pads +0
    Vp[:, :D] = V
    Vp[:, DP:] = np.tile(Vp[:, :8], (1, (G * 8 - DP) // 8))   # a spare lane loads the row's first fragment
    live = np.arange(G) * 8 < DP
    n = len(indptr) - 1
    y = np.empty(n, F4)
    for r in range(n):
        s, q, lin = np.zeros(G * 8, F4), np.zeros(G * 8, F4), F4(0)
        for p in range(indptr[r], indptr[r + 1]):
            x, f = F4(data[p]), indices[p]
            xv = x * Vp[f]
            s = s + xv
            q = _fma32(xv, xv, q)
            lin = _fma32(x, Wt[f], lin)
        t = (s * s - q).reshape(G, 8)
        acc = np.zeros(G, F4)
        for e in range(8):
            acc = acc + t[:, e]
        acc = np.where(live, acc, F4(0))
        o = G // 2
        while o >= 1:
            acc = acc + acc[np.arange(G) ^ o]
            o //= 2
        y[r] = (mu + lin) + F4(0.5) * acc[0]
    return y


# ---------------------------------------------------------------- what rounding V to bf16 may move
def quantisation_bound(mu, Wt, V, indptr, indices, data):
    """per row: 2^-9 sum_d (|s_d| A_d + q_d) + 2^-19 sum_d (A_d^2 + q_d), with s, A of fm_ref.forward_terms on the float32
    V and q_d = sum_j (x v_jd)^2.  With every element moved by 2^-9 of itself, s_d moves by at most 2^-9 A_d and
    0.5 s_d^2 by |s_d| 2^-9 A_d + 0.5 (2^-9 A_d)^2; each (x v)^2 by (2^-8 + 2^-18) of itself, and 0.5 q_d by half of that
    sum.  Round to nearest moves a single bf16 element by up to 2^-8 of itself (8 significand bits), twice that: the
    statement is not a worst-case bound but one for rows that sum several independent roundings, and a row of one entry
    is exact whatever V (s^2 = q).  tests/test_fm_bf16_host.py runs it in float64 on the GPU test's own inputs and prints
    the fraction of the first term they reach.  Returns (first term, second term)."""
    t = FR.forward_terms(mu, Wt, V, indptr, indices, data)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    xv = np.asarray(data, np.float64)[:, None] * np.asarray(V, np.float64)[np.asarray(indices, np.int64)]
    Q = R.seg_sum(xv * xv, rows, len(indptr) - 1)
    S, A = t["S"], t["A"]
    return 2.0 ** -9 * np.sum(np.abs(S) * A + Q, axis=1), 2.0 ** -19 * np.sum(A * A + Q, axis=1)


def float32_allowance(mu, Wt, V, indptr, indices, data):
    """per row: limit x eps32 x X_r, the distance fm_ref.forward_excess allows between a float32 forward on these tables
    and float64"""
    t = FR.forward_terms(mu, Wt, V, indptr, indices, data)
    lim = R.limit_from(R.ratio(FR.f32_fm(mu, Wt, V, indptr, indices, data)["y"], t["y"], t["X"], t["nnz"]))
    return np.where(t["nnz"] <= R.LONG_RUN, lim["short"], lim["long"]) * R.EPS32 * t["X"]


# ---------------------------------------------------------------- dyadic inputs: every product and sum exact
def dyadic(rs, shape, step):
    return (rs.randint(-int(1 / step), int(1 / step) + 1, shape) * step).astype(F4)


@functools.lru_cache(maxsize=None)
def dyadic_model(D):
    """mu a multiple of 1/4, W multiples of 1/4 and V of 1/4 in [-1, 1]"""
    rs = np.random.RandomState(31 + D)
    return F4(0.25), dyadic(rs, F, .25), dyadic(rs, (F, D), .25)


@functools.lru_cache(maxsize=None)
def dyadic_design():
    """the rows of ``design`` with values that are multiples of 1/2 in [-2, 2]"""
    indptr, indices, data = design()
    rs = np.random.RandomState(3)
    vals = (rs.randint(-4, 5, data.size) * 0.5).astype(F4)
    vals[data == 0] = 0
    return indptr, indices, vals


@functools.lru_cache(maxsize=None)
def topk_tables(D, users=40, items=500):
    """bf16_topk_cases.dyadic_tables-style V (multiples of 1/8) and W (of 1/4) over users + items features, users first:
    the layout of FmModel.get_ranking"""
    from tests import bf16_topk_cases as TC
    rs = np.random.RandomState(10 + D)
    nf = users + items
    return dict(mu=F4(0.25), W=TC.dyadic(rs, nf, .25), V=TC.dyadic(rs, (nf, D), .125), users=users, items=items)


def dyadic_faults(mu, Wt, V, indptr, indices, data):
    """the names of the exactness properties the inputs break (empty: float32 arithmetic in any order, fused or not, gives
    the float64 prediction).  x v is a multiple of 1/8, so every partial sum of s_d is one, bounded by A_d = sum |x v|;
    s_d^2 (at most A_d^2), the partial sums of q_d and s_d^2 - q_d are multiples of 1/64, and every partial sum of those
    over d is bounded by T = sum_d (s_d^2 + q_d); x w, mu and their sums are multiples of 1/8 bounded by
    L = |mu| + sum |x w|; the prediction and its two halves are multiples of 1/128 bounded by L + T / 2."""
    faults = []
    V, Wt, data = np.asarray(V, np.float64), np.asarray(Wt, np.float64), np.asarray(data, np.float64)
    if not np.array_equal(bf16.round_trip(V.astype(F4)), V.astype(F4)):
        faults.append("rows are bf16-exact")
    if not (np.array_equal(V * 4, np.rint(V * 4)) and np.abs(V).max() <= 1 and np.array_equal(Wt * 4, np.rint(Wt * 4))
            and np.abs(Wt).max() <= 1 and float(mu) * 4 == round(float(mu) * 4)):
        faults.append("tables are multiples of 1/4 in [-1, 1]")
    if not (np.array_equal(data * 2, np.rint(data * 2)) and np.abs(data).max() <= 2):
        faults.append("values are multiples of 1/2 in [-2, 2]")
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    xv = data[:, None] * V[np.asarray(indices, np.int64)]
    S, A, Q = R.seg_sum(xv, rows, n), R.seg_sum(np.abs(xv), rows, n), R.seg_sum(xv * xv, rows, n)
    if not (A * A).max() * 64 < 2 ** 24:
        faults.append("s_d^2 is a multiple of 1/64 below 2^18")
    T = np.sum(S * S + Q, axis=1)
    L = abs(float(mu)) + R.seg_sum(np.abs(data * Wt[np.asarray(indices, np.int64)]), rows, n)
    if not (L + T).max() * 128 < 2 ** 24:
        faults.append("every partial sum is a multiple of 1/128 below 2^17")
    return faults
