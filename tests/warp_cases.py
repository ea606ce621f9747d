"""The cases of tests/test_gpu_warp.py as plain data with their seeded inputs, shared with tests/test_warp_host.py (which
checks on the CPU that the inputs reach what they were built for, from the reference alone).

``EXACT``   the search on tables whose every product and partial sum is exact in float32 in any order (entries multiples of
            1/8 in [-2, 2], biases multiples of 1/8): the device's negatives and trial counts must equal the float64
            reference's.  ``random`` worlds draw the tables; ``planted`` worlds decide by the item biases alone (a large
            catalogue) and ``planted_rows`` worlds by one-hot item rows (a small one, D > I) where each triple's violator
            lies, one triple per position of the candidate list.
``RANDOM``  normal tables (U 300, I 200, B 700): decisions are held outside the rounding band only.
``STEP``    BPR's run-edge batches (tests/bpr_cases.py) with a margin: given negatives that mix g = -w and g = 0 in a user
            run, and searched ones that mix live and skipped triples, a run of skipped triples only and an item seen only
            in skipped triples."""
import functools

import numpy as np

from tests import bpr_cases as BC
from tests import bpr_ref as BR
from tests import warp_ref as WR
from tests import widths as W

GROUP = 4                                  # csrc/warp.h WARP_GROUP
SEED, STEP = 2024, 5
ROW_LENGTHS = (0, 1, 63, 64, 65)           # positives rows around the binary search's powers of two
INF = float("inf")

_EXACT = []


def _exact(D, item_abs=False, I=200, attempts=16, margin=1.0, kind="random"):
    c = dict(D=D, item_abs=item_abs, I=I, attempts=attempts, margin=margin, kind=kind)
    c["id"] = "%s-D%d%s-I%d-a%d-m%s" % (kind, D, "-abs" if item_abs else "", I, attempts, margin)
    _EXACT.append(c)


for _d in W.BPR:
    for _abs in (False, True):
        _exact(_d, _abs)
for _a in (1, 64):
    _exact(16, attempts=_a)
for _m in (0.0, INF, -INF):
    _exact(33, margin=_m)
for _i in (2, 3, 65):                      # (I - 1) // N reaches 1: the weight 0
    _exact(16, I=_i, margin=INF)
    _exact(16, I=_i)
for _d, _i, _a in ((3, 2, 16), (4, 3, 16), (68, 65, 64)):            # N reaches past (I - 1) / 2: the weight 0
    _exact(_d, I=_i, attempts=_a, kind="planted_rows")
_exact(16, I=70000, kind="planted")        # the candidate product (r >> 32) * I passes 16 bits of I
_exact(16, I=70000, attempts=64, kind="planted")
_exact(100, item_abs=True, I=70000, attempts=16, kind="random")
EXACT = tuple(_EXACT)
assert len({c["id"] for c in EXACT}) == len(EXACT)


def _eighths(rs, *shape):
    return (rs.randint(-16, 17, shape) / 8.0).astype(np.float32)


def _csr(rows):
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    items = np.concatenate([np.asarray(r, np.int64) for r in rows]) if rows else np.zeros(0, np.int64)
    return indptr, items.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _exact_world(case_id):
    case = [c for c in EXACT if c["id"] == case_id][0]
    D, I, A = case["D"], case["I"], case["attempts"]
    rs = np.random.RandomState(BC.seed_of(case))
    if case["kind"] == "planted_rows":
        # one user per triple; item c is the one-hot row e_{1+c} with bias 0, the positive item 0 has bias 2 and Q[0, 0] = 1,
        # P[u, 0] = P[u, 1] = 0: x = 2 - P[u, 1 + c].  P[u, 1 + c] = 2 makes c a violator of margin 1 for this user alone
        assert D > I
        B = A + GROUP + 3
        c = BR.candidates(SEED, STEP, B, I, A).astype(np.int64)
        P = np.zeros((B, D), np.float32)
        rows = []
        for b in range(B):
            if c[b, b % A] != 0:
                P[b, 1 + c[b, b % A]] = 2.0
            rows.append(sorted({0, int(c[b, 1])} if b % 3 == 2 and c[b, 1] != c[b, b % A] else {0}))
        Q = np.zeros((I, D), np.float32)
        Q[np.arange(I), 1 + np.arange(I)] = 1.0
        Q[0] = 0.0
        Q[0, 0] = 1.0
        bi = np.zeros(I, np.float32)
        bi[0] = 2.0
        t = dict(mu=np.float32(0.25), bu=_eighths(rs, B), bi=bi, P=P, Q=Q)
        return dict(U=B, t=t, pos=_csr(rows), u=np.arange(B, dtype=np.int32), i=np.zeros(B, np.int32))
    if case["kind"] == "planted":
        # one user per triple, P[u] = 0: x = bi[i] - bi[c].  The positive is item 0 (bi = 2, a positive of every user, so
        # never counted); a candidate with bi = 2 violates margin 1 (x = 0), one with bi = 0 does not (x = 2).  Triple b
        # plants its violator at candidate b % attempts; every third triple makes candidate 1 a positive of its user (N < t + 1)
        B = A + GROUP + 3
        c = BR.candidates(SEED, STEP, B, I, A).astype(np.int64)
        bi = np.zeros(I, np.float32)
        bi[0] = 2.0
        rows = []
        for b in range(B):
            bi[c[b, b % A]] = 2.0
            rows.append(sorted({0, int(c[b, 1])} if b % 3 == 2 and A > 1 else {0}))
        P = np.zeros((B, D), np.float32)
        u, i = np.arange(B), np.zeros(B, np.int64)
        U = B
    else:
        U = len(ROW_LENGTHS) + 8
        B = 203                                           # not a multiple of the four waves of a block
        rows = [np.sort(rs.choice(I, min(n, I), replace=False)) for n in ROW_LENGTHS]
        rows += [np.delete(np.arange(I), rs.randint(I)), np.arange(I)]           # every item but one; every item
        rows += [np.sort(rs.choice(I, rs.randint(1, min(I, 10) + 1), replace=False)) for _ in range(U - len(rows))]
        P, bi = _eighths(rs, U, D), _eighths(rs, I)
        u = np.concatenate((np.arange(U), rs.randint(0, U, B - U)))
        i = rs.randint(0, I, B)
    Q = _eighths(rs, I, D)
    if case["kind"] == "planted":                         # Q'[i] - Q'[j] = 1 in feature 0: under SGD with lr 1, lam 0 and
        Q[:, 0] = 0.0                                     # P[u] = 0 the step leaves the triple's weight there, P'[u, 0] = w
        Q[0, 0] = 1.0
    t = dict(mu=np.float32(0.25), bu=_eighths(rs, U), bi=bi, P=P, Q=Q)
    return dict(U=U, t=t, pos=_csr(rows), u=u.astype(np.int32), i=i.astype(np.int32))


def exact_world(case):
    """dict(U, t = the five tables, pos = (indptr, items), u, i)"""
    return _exact_world(case["id"])


def tid_tables(t):
    return {BR.BI: t["bi"], BR.PF: t["P"], BR.QF: t["Q"]}


@functools.lru_cache(maxsize=None)
def _exact_reference(case_id):
    case = [c for c in EXACT if c["id"] == case_id][0]
    w = exact_world(case)
    return WR.examine(tid_tables(w["t"]), *w["pos"], w["u"], w["i"], case["margin"], seed=SEED, step=STEP,
                      attempts=case["attempts"], item_abs=case["item_abs"])


def exact_reference(case):
    """``warp_ref.examine`` of the case: computed once, shared, not to be written to"""
    return _exact_reference(case["id"])


# ----------------------------------------------------------------------------- random tables
RANDOM = tuple(dict(id="D%d%s-m%s" % (D, "-abs" if a else "", m), D=D, item_abs=a, margin=m, attempts=16)
               for D, a, m in ((16, False, 1.0), (100, True, 0.0), (256, False, 1.0)))
R_U, R_I, R_B = 300, 200, 700
BAND_CAP = 0.01                            # at most this share of the triples may have a candidate in the rounding band


@functools.lru_cache(maxsize=None)
def _random_world(case_id):
    case = [c for c in RANDOM if c["id"] == case_id][0]
    D = case["D"]
    rs = np.random.RandomState(BC.seed_of(case))
    scale = 0.5 / np.sqrt(max(D, 16) / 16)
    f = lambda *s: rs.normal(0, scale, s).astype(np.float32)
    t = dict(mu=np.float32(0.2), bu=f(R_U), bi=f(R_I), P=f(R_U, D), Q=f(R_I, D))
    rows = [np.sort(rs.choice(R_I, rs.randint(1, 40), replace=False)) for _ in range(R_U)]
    u = rs.randint(0, R_U, R_B)
    i = np.array([rs.choice(rows[x]) for x in u])
    return dict(U=R_U, t=t, pos=_csr(rows), u=u.astype(np.int32), i=i.astype(np.int32))


def random_world(case):
    return _random_world(case["id"])


@functools.lru_cache(maxsize=None)
def _random_reference(case_id):
    case = [c for c in RANDOM if c["id"] == case_id][0]
    w = random_world(case)
    return WR.examine(tid_tables(w["t"]), *w["pos"], w["u"], w["i"], case["margin"], seed=SEED, step=STEP,
                      attempts=case["attempts"], item_abs=case["item_abs"])


def random_reference(case):
    return _random_reference(case["id"])


# ----------------------------------------------------------------------------- the step per row
STEP_CASES = BC.CASES


def margin_of(case):
    """skip cases search with margin 0 and one attempt: about half the open candidates do not violate, so live and skipped
    triples share user runs.  edges cases give the negatives: margin 0 mixes g = -w and g = 0, margin 1 is mostly g = -w"""
    if case["kind"] == "skip":
        return 0.0
    return (0.0, 1.0)[BC.CASES.index(case) % 2]
