"""The cases of tests/test_gpu_bpr_step.py as plain data, with their seeded inputs: shared with the host tests
(tests/test_bpr_step_ref_host.py runs a float32 stand-in for the device through the same checks on every case).

``edges`` cases give the negatives: user runs and item runs of the lengths the run-end windows are built around, the
hazard chain, j == i, an exact zero in Q.  ``skip`` cases let the sampler draw them (one attempt), with a user whose
positives are every item and one whose positives are half of them; tests/bpr_ref.py's sampler says here what the device
will draw, and the device test holds the drawn negatives against it."""
import functools
import zlib

import numpy as np

from tests import bpr_ref as BR
from tests import widths as W

SGD_LR = 2.0 ** -10                       # a power of two (the gradient is read back as (w - w') / lr)
ADAM_LR, LAM = 3e-3, 0.02
WAVES = 4                                 # csrc/bpr.h BPR_WAVES
U, I = 400, 300
USER_RUNS = (1, 31, 32, 33, 64, 65)       # triples: 2, 62, 64, 66, 128 and 130 keys of the sorted user column
ITEM_RUNS = (1, 63, 64, 65, 128, 129)     # occurrences, both roles
RUN_USER = 10 + np.arange(len(USER_RUNS))
HAZARD_USER, N_HAZARD = 7, 40
SINGLES = np.arange(20, 170)
TAIL_USER = U - 1
RUN_ITEM = 280 + np.arange(len(ITEM_RUNS))
ZERO_ITEM = int(RUN_ITEM[1])
RAND_ITEMS = np.arange(20, 250)           # items 250..279 are in no triple
S_U, S_I, S_B, FULL, HALF, SEED = 60, 40, 401, 3, 5, 12345     # the skip cases' world

_CASES = []


def _case(D, kind="edges", tail=0, frozen=0, hyper2=None, opt=None):
    x = len(_CASES)
    c = dict(D=D, kind=kind, tail=tail, frozen=frozen, hyper2=hyper2, item_abs=bool(x & 1), reg_bias=bool((x >> 1) & 1),
             opt=opt or ("adam", "sgd")[(x // 2 + x // 4) % 2])
    c["U"], c["I"] = (S_U, S_I) if kind == "skip" else (U, I)
    c["id"] = "%s-D%d-%s%s%s%s%s%s" % (kind, D, c["opt"], "-abs" if c["item_abs"] else "", "-rb" if c["reg_bias"] else "",
                                     "-tail%d" % tail if tail else "", "-frozen%d" % frozen if frozen else "", "-hyper" if hyper2 else "")
    _CASES.append(c)


for _d in W.BPR:
    _case(_d)
_case(64, tail=33)                        # the last run of the sorted user column: 66 and 130 keys end at n
_case(100, tail=65)
_case(16, kind="skip", opt="adam")
_case(33, kind="skip", opt="sgd")
for _bit in (BR.BI, BR.PF, BR.QF):
    _case(16, frozen=1 << _bit, opt="adam")
_case(64, hyper2=(1e-3, 0.07), opt="adam")
_case(100, hyper2=(2.0 ** -12, 0.07), opt="sgd")

CASES = tuple(_CASES)
assert len({c["id"] for c in CASES}) == len(CASES)


def seed_of(case):
    return zlib.crc32(case["id"].encode()) & 0x7fffffff


def hyper_of(case, s):
    if s >= 1 and case["hyper2"]:
        return case["hyper2"]
    return (ADAM_LR if case["opt"] == "adam" else SGD_LR), LAM


def tables_of(case):
    D, nu, ni = case["D"], case["U"], case["I"]
    rs = np.random.RandomState(seed_of(case))
    scale = 0.3 / np.sqrt(max(D, 16) / 16)
    f = lambda *s: rs.normal(0, scale, s).astype(np.float32)
    t = dict(mu=np.float32(0.2), bu=f(nu), bi=f(ni), P=f(nu, D), Q=f(ni, D))
    z = ZERO_ITEM if case["kind"] == "edges" else 7
    t["Q"][z, 0] = 0.0
    t["Q"][z, D - 1] = 0.0
    return t


@functools.lru_cache(maxsize=None)
def positives(kind):
    """(indptr, items) for set_positives"""
    rs = np.random.RandomState(99)
    if kind == "skip":                    # item 0 is a positive of every user: never drawn as a negative
        rows = [np.concatenate(([0], np.sort(rs.choice(np.arange(1, S_I), rs.randint(1, 6), replace=False)))) for _ in range(S_U)]
        rows[FULL] = np.arange(S_I)
        rows[HALF] = np.arange(S_I // 2)
    else:
        rows = [np.sort(rs.choice(I, rs.randint(1, 10), replace=False)) for _ in range(U)]
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def _edges_batch(case, s):
    rs = np.random.RandomState((seed_of(case) + 7919 * (s + 1)) & 0x7fffffff)
    tail = case["tail"] or 1
    u = np.concatenate([np.repeat(RUN_USER, USER_RUNS), SINGLES, np.repeat(TAIL_USER, tail)])
    while (u.size + N_HAZARD) % WAVES != 1:              # B = 1 mod 4: the last block has one wave of work
        u = np.concatenate((u, [SINGLES[-1] + 1 + u.size % 7]))
    u = rs.permutation(u)
    n = u.size
    i, j = rs.choice(RAND_ITEMS, n), rs.choice(RAND_ITEMS, n)
    slots = rs.permutation(2 * n)[:sum(ITEM_RUNS)]       # occurrence slots of the designated items, either role
    flat = np.stack((i, j), axis=1).reshape(-1)
    flat[slots] = np.repeat(RUN_ITEM, ITEM_RUNS)
    i, j = flat.reshape(n, 2)[:, 0], flat.reshape(n, 2)[:, 1]
    k = np.arange(N_HAZARD)                               # tests/test_gpu_bpr.py hazard_batch: j of triple k is i of triple k + 1
    hi, hj = k % 13, (k + 1) % 13
    hj[-1] = hi[-1]                                       # an explicit j == i
    u = np.concatenate((np.full(N_HAZARD, HAZARD_USER), u))
    i, j = np.concatenate((hi, i)), np.concatenate((hj, j))
    nu = np.bincount(u, minlength=U)
    assert set(USER_RUNS) <= set(nu.tolist()) and u.max() == TAIL_USER and nu[TAIL_USER] == tail
    both = np.bincount(np.concatenate((i, j)), minlength=I)
    assert np.array_equal(both[RUN_ITEM], ITEM_RUNS)
    for it in RUN_ITEM[1:]:
        assert (i == it).any() and (j == it).any(), "item %d occurs in one role only" % it
    assert (i == j).any() and np.array_equal(j[:N_HAZARD - 2], i[1:N_HAZARD - 1]) and u.size % WAVES == 1
    assert both[250:280].sum() == 0
    return u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)


def _skip_batch(case, s):
    """(u, i, the negatives the device will draw at step s)"""
    rs = np.random.RandomState((seed_of(case) + 7919 * (s + 1)) & 0x7fffffff)
    u = rs.randint(0, S_U, S_B)
    u[(u == FULL) | (u == HALF)] = 4
    i = rs.randint(1, S_I, S_B)
    u[:5], i[:5] = FULL, 0
    u[5:45] = HALF
    indptr, items = positives("skip")
    j = BR.sample(indptr, items, u, S_I, SEED, s, 1)
    assert np.all(j[u == FULL] < 0), "a user run of skipped triples only"
    h = j[u == HALF] >= 0
    live = np.flatnonzero(h)
    assert live.size >= 2 and not h[live[0]:live[-1]].all(), "no skipped triple inside a run of live ones"
    keep = j >= 0
    assert (i == 0).any() and not (i[keep] == 0).any() and not (j == 0).any(), "item 0 occurs in skipped triples only"
    assert keep.sum() > S_B // 2 and u.size % WAVES == 1
    assert 7 in i[keep] or 7 in j[keep]
    return u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _inputs(case_id):
    case = [c for c in CASES if c["id"] == case_id][0]
    return tuple((_skip_batch if case["kind"] == "skip" else _edges_batch)(case, s) for s in range(2))


def batch_of(case, s):
    """(u, i, j) of step s; in a skip case j is what the sampler draws (the device is given none)"""
    return _inputs(case["id"])[s]
