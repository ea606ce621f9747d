"""The cases of tests/test_gpu_fm_step.py as plain data, with their seeded inputs: shared with the host tests
(tests/test_fm_ref_host.py runs a float32 stand-in for the device through the same checks on every case; the width guard
of tests/test_width_coverage.py reads the width list they are built from).

Every ordinary case holds, in both of its steps: an empty row; rows of 1, 3, 4, 5 and 9 entries; a row of 70 entries (the
forward walks a row four entries at a time and writes the backward's records with stride G <= 64); a row with one entry
(s_r - x V_j = 0: its V gradient is lam V_j alone); a column twice in one row; an explicit zero; negative and fractional
values; features 0 and F - 1; features no row touches; hot features whose runs exceed LONG_RUN and are cut across the
reduce's pieces, and short runs left whole; n no multiple of 256 / G."""
import functools
import os
import re
import zlib

import numpy as np
import scipy.sparse as sp

from oracle import svd_oracle as so
from tests import step_ref as R
from tests import widths as W

SGD_LR = 2.0 ** -10                       # a power of two (the gradient is read back as (w - w') / lr)
ADAM_LR, LAM = 0.002, 0.01
PAIRS = (("mse", "sgd"), ("nll", "sgd"), ("mse", "adam"), ("nll", "adam"))
LONG_ROW = 70
UNTOUCHED = 20                            # features F - 1 - UNTOUCHED .. F - 2 are in no row

_CASES = []


def _case(D, loss, opt, F=400, n=701, kind="edges"):
    c = dict(D=D, loss=loss, opt=opt, F=F, n=n, kind=kind)
    c["id"] = "%s-F%d-D%d-n%d-%s_%s" % (kind, F, D, n, loss, opt)
    if c["id"] not in {x["id"] for x in _CASES}:
        _CASES.append(c)


# one width per (G, VEC, full width); loss and optimiser rotate
for _k, _d in enumerate(W.FM_STEP):
    _case(_d, ("mse", "nll")[_k % 2], ("sgd", "adam")[(_k >> 1) % 2], F=(300, 400, 600)[_k % 3])
# every (loss, optimiser) pair at a full and at a partial width
for _d in (64, 100):
    for _l, _o in PAIRS:
        _case(_d, _l, _o)
# every row empty: only mu and its slots move
_case(16, "nll", "adam", kind="empty")
_case(13, "mse", "sgd", kind="empty")
# the training forward's block-stride loop: G = 64 puts 4 rows in a block, 4096 blocks at the most
_case(256, "nll", "adam", F=40, n=4096 * 4 + 37, kind="stride")

CASES = tuple(_CASES)
assert len({c["id"] for c in CASES}) == len(CASES)


def seed_of(case):
    return zlib.crc32(case["id"].encode()) & 0x7fffffff


def geometry(D):
    """(G, VEC): csrc/svd_kernels.h geometry"""
    vec = 4 if D % 4 == 0 else 1
    lanes, g = -(-D // vec), 4
    while g < lanes:
        g *= 2
    return g, vec


def piece_len(G):
    """entries of the sorted order one k_seg_reduce block owns, read from the kernel's source"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tf-recomm_amd", "csrc", "svd_kernels.hip")).read()
    threads = re.search(r"constexpr int EPB = (\d+) / G;", src)
    assert threads, "k_seg_reduce no longer states its piece length as EPB = <threads> / G"
    return int(threads.group(1)) // G


def hyper_of(case):
    return (ADAM_LR if case["opt"] == "adam" else SGD_LR), LAM


def tables_of(case):
    rs = np.random.RandomState(seed_of(case))
    F, D = case["F"], case["D"]
    return dict(mu=np.float32(0.1), W=rs.normal(0, 0.1, F).astype(np.float32),
                V=rs.normal(0, 0.1 / np.sqrt(max(D, 16) / 16), (F, D)).astype(np.float32))


def _values(rs, k):
    """counts 1..3, a third of them replaced by negative and fractional values"""
    v = rs.randint(1, 4, k).astype(np.float32)
    return np.where(rs.rand(k) < 0.33, rs.normal(0, 1, k), v).astype(np.float32)


def _design(case, s):
    F, n, kind = case["F"], case["n"], case["kind"]
    rs = np.random.RandomState((seed_of(case) + 7919 * (s + 1)) & 0x7fffffff)
    if kind == "empty":
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    if kind == "stride":
        indptr = np.arange(n + 1, dtype=np.int64) * 2
        return indptr, rs.randint(0, F, 2 * n).astype(np.int32), _values(rs, 2 * n)
    cold = F - 1 - UNTOUCHED                              # ordinary draws come from [0, cold)
    hot = (0, cold // 2 + s, cold - 1)                    # on a half, a fifth and an eighth of the rows
    lens = rs.randint(1, 10, n)
    lens[:8] = (0, 1, 3, 4, 5, 9, LONG_ROW, 1)
    rows = []
    for r in range(n):
        k = int(lens[r])
        cols, vals = rs.randint(0, cold, k), _values(rs, k)
        if r == 6:
            cols = rs.choice(cold, k, replace=False)
        elif r == 8:                                      # a column twice in one row
            cols, vals = np.array([7, 7, 9]), np.array([2.0, -0.75, 1.0], np.float32)
        elif r == 9:                                      # an explicit zero
            cols, vals = np.array([11, 12, 13]), np.array([1.0, 0.0, 3.0], np.float32)
        elif r == 10:                                     # both ends of the table
            cols, vals = np.array([F - 1, 0, 5, F - 1 - UNTOUCHED - 1]), np.array([1.0, 2.0, -1.5, 0.25], np.float32)
        elif r > 10:
            p = rs.rand()
            cols[0] = hot[0] if p < 0.5 else hot[1] if p < 0.7 else hot[2] if p < 0.82 else cols[0]
        rows.append((cols, vals))
    indptr = np.concatenate(([0], np.cumsum([len(c) for c, _ in rows]))).astype(np.int64)
    indices = np.concatenate([c for c, _ in rows]).astype(np.int32)
    data = np.concatenate([v for _, v in rows]).astype(np.float32)
    _assert_edges(case, indptr, indices, data)
    return indptr, indices, data


def _assert_edges(case, indptr, indices, data):
    F, n = case["F"], case["n"]
    G, _ = geometry(case["D"])
    lens = np.diff(indptr)
    assert {0, 1, 3, 4, 5, 9}.issubset(set(lens.tolist())) and lens.max() > 64 and n % (256 // G)
    assert (data == 0).any() and (data < 0).any() and (data != np.round(data)).any()
    cnt = np.bincount(indices, minlength=F)
    assert cnt[0] and cnt[F - 1] and (cnt == 0).sum() >= UNTOUCHED
    assert any(np.unique(indices[indptr[r]:indptr[r + 1]]).size < lens[r] for r in range(n))
    # the runs of the sorted order against the reduce's pieces: a long run cut across pieces, a short run left whole
    piece = piece_len(G)
    ends = np.cumsum(cnt)
    first, last = (ends - cnt) // piece, (ends - 1) // piece
    cut = (cnt > 0) & (first != last)
    assert (cut & (cnt > R.LONG_RUN)).any(), "%s: no run above LONG_RUN is cut across the reduce's pieces" % case["id"]
    assert ((cnt > 0) & ~cut & (cnt <= R.LONG_RUN)).any(), "%s: no short run is left whole" % case["id"]


@functools.lru_cache(maxsize=None)
def _inputs(case_id):
    case = [c for c in CASES if c["id"] == case_id][0]
    steps = []
    for s in range(2):
        rs = np.random.RandomState((seed_of(case) + 104729 * (s + 1)) & 0x7fffffff)
        n = case["n"]
        y = (rs.rand(n) < 0.5).astype(np.float32) if case["loss"] == "nll" else rs.normal(0, 1, n).astype(np.float32)
        steps.append((_design(case, s), y))
    # the condition on the float64 reference that makes a per-row check mean something: nothing diverges.  max |V| and
    # max |W| after both steps stay within twice their initial values
    t = tables_of(case)
    lr, lam = hyper_of(case)
    mu, Wt, V = np.float64(t["mu"]), t["W"].astype(np.float64), t["V"].astype(np.float64)
    state = so.fm_adam_state(case["F"], case["D"]) if case["opt"] == "adam" else None
    for (indptr, indices, data), y in steps:
        _, _, mu = so.fm_train_step(mu, Wt, V, indptr, indices.astype(np.int64), data.astype(np.float64), y.astype(np.float64),
                                    lr, lam, case["loss"], case["opt"], state)
    assert np.abs(V).max() <= 2 * np.abs(t["V"]).max() and np.abs(Wt).max() <= 2 * np.abs(t["W"]).max(), \
        "%s: the float64 reference leaves its initial scale" % case["id"]
    return tuple(steps)


def batch_of(case, s):
    """((indptr, indices, data), y) of step s"""
    return _inputs(case["id"])[s]


def as_csr(csr, F):
    """the scipy matrix ``FmModel.train_step`` takes - built from the three arrays, so that duplicate columns, explicit zeros
    and the entries' order stay as they are"""
    indptr, indices, data = csr
    return sp.csr_matrix((data, indices, indptr), shape=(indptr.size - 1, F))
