"""Shared inputs of tests/test_fm_fit_host.py and tests/test_gpu_fm_fit.py: the reference of the device's minibatch gather
(scipy's ``X[ids]`` / ``y[ids]``), one small row store and the id batches drawn from it.

The store: F = 400 features, N = 701 rows of 0 .. 9 entries, one row of 70 (longer than a wave) and one of 300; empty rows at
0, N - 1 and in the middle; count-valued, negative and fractional values; features no row holds.  The batches are the
smallest that reach every path of the gather: sub-wave lane groups of every width, the whole-wave loop over a long row, the
scan's 256-row rounds and its chunk boundary, duplicates, both ends of the store and a batch with no entry at all."""
import functools

import numpy as np
import scipy.sparse as sp

F, N = 400, 701
LONG_ROW, LONG_LEN = 6, 70                # a row longer than a wave
HUGE_ROW, HUGE_LEN = 333, 300
EMPTY_ROWS = (0, 350, N - 1)
UNTOUCHED = 20                            # features F - 1 - UNTOUCHED .. F - 2 are in no row
SCAN_CHUNK = 2048                         # csrc/fm_fit.h FM_SCAN_CHUNK: batch rows per block of the length scan
WIDE_ROUNDS = 4                           # csrc/fm_fit.h FM_WIDE_ROUNDS


def gather_rows_ref(x, y, ids):
    """(X[ids], y[ids]): rows in id order, entries in stored order, duplicates repeated, empty rows empty"""
    ids = np.asarray(ids, np.int64)
    return x[ids], np.asarray(y)[ids]


def group_of(n_rows, nnz):
    """lanes per row of the copy kernel (csrc/fm_fit.hip fm_gather_group): the power of two in [4, 64] covering the mean row"""
    mean, g = -(-nnz // n_rows), 4
    while g < 64 and g < mean:
        g *= 2
    return g


def make_store(seed, n=N, positives=0.5, targets="binary"):
    """(csr [n, F], y [n]) with the rows described above (the special rows only when n == N)"""
    rs = np.random.RandomState(seed)
    cold = F - 1 - UNTOUCHED
    lens = rs.randint(0, 10, n)
    if n == N:
        lens[:12] = (0, 1, 2, 3, 4, 5, LONG_LEN, 6, 7, 8, 9, 1)
        lens[HUGE_ROW] = HUGE_LEN
        for r in EMPTY_ROWS:
            lens[r] = 0
    rows = []
    for r in range(n):
        k = int(lens[r])
        cols = rs.choice(cold, k, replace=False) if k > 9 else rs.randint(0, cold, k)
        vals = rs.randint(1, 4, k).astype(np.float32)
        vals = np.where(rs.rand(k) < 0.33, rs.normal(0, 1, k), vals).astype(np.float32)
        if k > 9:
            vals *= np.float32(0.25)                       # the long rows' predictions stay of order one
        rows.append((cols, vals))
    if n == N:
        rows[11] = (np.array([F - 1]), np.array([2.0], np.float32))          # the last feature
        rows[1] = (np.array([0]), np.array([-1.5], np.float32))              # the first
    indptr = np.concatenate(([0], np.cumsum([len(c) for c, _ in rows]))).astype(np.int64)
    indices = np.concatenate([c for c, _ in rows]).astype(np.int32)
    data = np.concatenate([v for _, v in rows]).astype(np.float32)
    x = sp.csr_matrix((data, indices, indptr), shape=(n, F))
    y = (rs.rand(n) < positives).astype(np.float32) if targets == "binary" else rs.normal(0, 1, n).astype(np.float32)
    if n == N:
        ln = np.diff(x.indptr)
        assert set(range(10)) <= set(ln.tolist()) and ln[LONG_ROW] == LONG_LEN and ln[HUGE_ROW] == HUGE_LEN
        assert all(ln[r] == 0 for r in EMPTY_ROWS)
        cnt = np.bincount(indices, minlength=F)
        assert cnt[0] and cnt[F - 1] and (cnt == 0).sum() >= UNTOUCHED
        assert (data < 0).any() and (data != np.round(data)).any() and (data == np.round(data)).any()
    return x, y


@functools.lru_cache(maxsize=None)
def store(which="train"):
    """the train store (binary targets) and a second, different store of the same shape used as the eval store"""
    x, y = make_store(11 if which == "train" else 23)
    # the reference itself: duplicates are repeated rows, entries keep their stored order, empty rows stay empty
    ids = np.array([LONG_ROW, 0, 9, 9, N - 1])
    gx, gy = gather_rows_ref(x, y, ids)
    lo, hi = x.indptr[LONG_ROW], x.indptr[LONG_ROW + 1]
    l9 = x.indptr[10] - x.indptr[9]
    assert gx.shape == (5, F) and np.array_equal(gy, y[ids]) and np.array_equal(np.diff(gx.indptr), [LONG_LEN, 0, l9, l9, 0])
    assert np.array_equal(gx.indices[:LONG_LEN], x.indices[lo:hi]) and np.array_equal(gx.data[:LONG_LEN], x.data[lo:hi])
    return x, y


@functools.lru_cache(maxsize=None)
def batches():
    """name -> ids (int64), every id in [0, N)"""
    rs = np.random.RandomState(5)
    ln = np.diff(store("train")[0].indptr)
    ln2 = np.diff(store("eval")[0].indptr)
    short = np.flatnonzero((ln <= 3) & (ln2 <= 3))
    b = {
        "B1": np.array([17]),
        "B1-huge": np.array([HUGE_ROW]),
        "B63": rs.randint(0, N, 63),
        "B64": rs.randint(0, N, 64),
        "B257": np.concatenate((rs.randint(0, N, 255), [LONG_ROW, HUGE_ROW])),        # long rows among lane groups of 8
        "repeat-one": np.full(33, 9),
        "repeat-long": np.full(5, LONG_ROW),
        "ends": np.array([N - 1, 0, 5, N - 1, 0, 10]),
        "empty-only": np.array(EMPTY_ROWS * 3),
        "above-a-chunk": rs.randint(0, N, SCAN_CHUNK + 1),
        "two-chunks-and-a-bit": rs.randint(0, N, 2 * SCAN_CHUNK + 300),
        "group4": rs.choice(short, 40),                                               # mean row <= 4
        "group4-wide": np.concatenate((rs.choice(short, 60), [LONG_ROW])),            # ... and a row for the whole wave
        "group16": np.concatenate((np.full(12, 10), [LONG_ROW])),                     # mean row in (8, 16]
        "group32": np.concatenate((np.full(4, 10), np.full(2, LONG_ROW))),            # mean row in (16, 32]
        "group64": np.array([HUGE_ROW, 3, LONG_ROW]),
    }
    b = {k: np.asarray(v, np.int64) for k, v in b.items()}
    want = {"group4": 4, "group4-wide": 4, "B257": 8, "group16": 16, "group32": 32, "group64": 64, "B1-huge": 64}
    for name, g in want.items():
        for l in (ln, ln2):
            assert group_of(b[name].size, int(l[b[name]].sum())) == g, (name, g)
    # a row longer than WIDE_ROUNDS turns of its lane group, in a batch of lane groups of 4, 8 and 16
    for name, g in (("group4-wide", 4), ("B257", 8), ("group16", 16)):
        assert ln[b[name]].max() > WIDE_ROUNDS * g
    assert int(ln[b["empty-only"]].sum()) == 0 == int(ln2[b["empty-only"]].sum())
    return b


def train_ids(batch=64, seed=3):
    """six steps' ids [6 * batch]: random draws; the store's ends and long rows; one id repeated; empty rows only; random"""
    rs = np.random.RandomState(seed)
    steps = [rs.randint(0, N, batch) for _ in range(6)]
    steps[1][:4] = (0, N - 1, LONG_ROW, HUGE_ROW)
    steps[2][:] = LONG_ROW
    steps[3] = np.asarray(EMPTY_ROWS)[rs.randint(0, len(EMPTY_ROWS), batch)]
    return np.concatenate(steps).astype(np.int64)
