"""Cases for folding new users and items into an implicit ALS (tests/test_ials_fold_host.py, tests/test_gpu_ials_fold.py;
include/tfrecomm.h tfr_ials_fold_in).

A case is a dict of tests/ials_cases.py (the resident user x item CSR with the tables X, Y, built by its ``_case``) with, on
top of it, the lists the model has never seen:

    new[0]    (ptr, ids, vals, ni): item lists of new users          new[1]    (ptr, ids, vals, nu): user lists of new items
    start[0], start[1]             [n, d] uniform in [0, 1): the non-zero conjugate-gradient starts
    steps                          0 on the Cholesky path, else the conjugate-gradient steps of the case

``new[side]`` has the layout of ``ials_ref.lists(case, side)``, so every restatement takes it as it is.  Tables stay small
(150 users, 200 items): what can go wrong in a fold-in depends on the width, on each list's length and on the chunk size.

Resident data: users 0 .. 7 hold 0, 1, 5, 31, chunk + 1, 2 chunk + 1, 33 and 64 items; the next chunk + 10 users all hold
item 0, which is then the one chunked item (two chunks); the last item has no user.  New lists: one per length of
``lengths(chunk)`` - every tile edge, and both sides of one chunk and of two - drawn from all partners, so they also hold
partners the resident lists never touch.
"""
import numpy as np

from tests import ials_cases as C

NU, NI = 150, 200
CHOL_WIDTHS = (1, 17, 33, 64)                              # slot edges of ials_cases.WIDTHS: 1, 2, 5 and 16 live slots
CHUNKS = (32, 64)
CG_WIDTHS = (33, 128, 256)                                 # 1, 2 and 4 components per lane
CG_STEPS = 3
CONV_WIDTH = 33                                            # 3 d steps against the exact minimiser (ials_cg_cases.CONV_WIDTHS)


def lengths(chunk):
    return C.TILE_LENGTHS + (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)


def _new_lists(rs, chunk, n_other):
    rows = [np.sort(rs.choice(n_other, n, replace=False)) for n in lengths(chunk)]
    ptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    ids = np.concatenate(rows).astype(np.int32)
    return ptr, ids, np.ascontiguousarray(C._values(rs, ids.size), np.float64), n_other


def fold_case(d, chunk, steps=0):
    rs = np.random.RandomState(9000 + 1000 * (steps > 0) + 10 * d + chunk // 32)
    inner = np.arange(1, NI - 1)                           # item 0 is the chunked one, item NI - 1 has no user
    rows = [rs.choice(inner, n, replace=False) for n in (0, 1, 5, 31, chunk + 1, 2 * chunk + 1, 33, 64)]
    rows += [np.concatenate(([0], rs.choice(inner, 3, replace=False))) for _ in range(chunk + 10)]
    rows += [rs.choice(inner, 4, replace=False) for _ in range(NU - len(rows))]
    name = "fold-%s-d%d-chunk%d" % ("cg%d" % steps if steps else "chol", d, chunk)
    c = C._case(name, d, 0.1, 40.0, chunk, NU, NI, rows, rs)
    new = (_new_lists(rs, chunk, NI), _new_lists(rs, chunk, NU))
    n = len(lengths(chunk))
    return dict(c, steps=steps, new=new, start=(rs.uniform(0.0, 1.0, (n, d)), rs.uniform(0.0, 1.0, (n, d))))


def csr(lst):
    """a (ptr, ids, vals, n_other) list set as the scipy matrix the Python methods take"""
    import scipy.sparse as sp
    ptr, ids, vals, n_other = lst
    return sp.csr_matrix((vals, ids, ptr), shape=(ptr.size - 1, n_other))


def take(lst, rows):
    """the lists ``rows`` of a list set, in that order"""
    ptr, ids, vals, n_other = lst
    sel = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = np.concatenate(([0], np.cumsum([ptr[r + 1] - ptr[r] for r in rows]))).astype(np.int64)
    return out, np.ascontiguousarray(ids[sel]), np.ascontiguousarray(vals[sel]), n_other


CHOL_CASES = [fold_case(d, ch) for d in CHOL_WIDTHS for ch in CHUNKS]
CG_CASES = [fold_case(d, 32, CG_STEPS) for d in CG_WIDTHS]
CONV_CASE = dict(fold_case(CONV_WIDTH, 32, 3 * CONV_WIDTH), id="fold-conv-d%d" % CONV_WIDTH)
CASES = CHOL_CASES + CG_CASES + [CONV_CASE]
BY_ID = {c["id"]: c for c in CASES}
