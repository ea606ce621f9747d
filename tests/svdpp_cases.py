"""The cases of tests/test_gpu_svdpp_step.py as plain data, with their seeded inputs: shared with the host tests
(tests/test_svdpp_step_ref_host.py runs a float32 stand-in for the device through the same checks on every case).

One world of implicit sets serves every case.  Users 0..299 are in every batch (ACT), users 300..599 in none (INA), so a
column of NT can be given any length with all, none or half of its users active; GA holds three users per |N(u)| of
NSET (in both steps, in step 0 only, in step 1 only) whose sets are drawn from filler items; HI are active users with ids
above INA (the last lane of a window); the highest user and the highest item end the two sorted columns of the batch.
``_assert_edges`` holds every edge the kernels are built around against what was really built."""
import functools
import zlib

import numpy as np

from tests import widths as W

SGD_LR = 2.0 ** -10                       # a power of two (the gradient is read back as (w - w') / lr)
ADAM_LR, LAM = 3e-3, 0.02
PIECE, WAVES = 128, 4                     # csrc/svdpp.h PP_PIECE, PP_WAVES
NSET = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257)
RUNS = (1, 2, 63, 64, 65, 66, 128, 129)
MU, BU, BI, P, Q, Y = 0, 1, 2, 3, 4, 5

N_ACT, N_INA = 300, 300
ACT = np.arange(N_ACT)
INA = np.arange(N_ACT, N_ACT + N_INA)
GA0 = N_ACT + N_INA                       # GA[x, k]: |N(u)| = NSET[x]; k = 0 both steps, 1 step 0 only, 2 step 1 only
GA = GA0 + np.arange(3 * len(NSET)).reshape(len(NSET), 3)
HI = GA0 + 3 * len(NSET) + np.arange(7)
T_USER = (HI[-1] + 1, HI[-1] + 2)         # a user of step 0 only and one of step 1 only, each alone in a column
TAIL_USER = HI[-1] + 3
U = int(TAIL_USER) + 1

COLS = {}                                 # (L, kind) -> item
for _L in NSET:
    for _kind in ("all", "none", "mixed"):
        if _L == 0 and _kind != "all" or _L == 1 and _kind == "mixed":
            continue
        COLS[_L, _kind] = len(COLS)
W0, W63, WGAP, T_ITEM0, T_ITEM1 = (len(COLS) + k for k in range(5))
F0, N_FILL = len(COLS) + 5, 260           # filler items: the sets of GA, HI, T_USER and TAIL_USER
RUN_ITEM = F0 + 10 + np.arange(len(RUNS))  # the items whose batch runs have the lengths RUNS
ZERO_ITEM = int(RUN_ITEM[1])              # a touched item row (a run of 2) with exact zeros in Q
Q_ITEM = (F0 + 30, F0 + 31)               # an item row of step 0 only, and one of step 1 only
RAND_ITEMS = np.arange(F0 + 40, F0 + N_FILL)
TAIL_ITEM = F0 + N_FILL
I = TAIL_ITEM + 1
RUN_USER = ACT[10:10 + len(RUNS)]
PAD_USER = int(ACT[20])

_CASES = []


def _case(D, kind="edges", tail=0, frozen=0, hyper2=None, opt=None):
    x = len(_CASES)
    c = dict(D=D, kind=kind, tail=tail, frozen=frozen, hyper2=hyper2, loss=("mse", "nll")[x % 2], item_abs=bool((x >> 1) & 1),
             reg_bias=bool((x >> 2) & 1), opt=opt or ("adam", "sgd")[(x // 2 + x // 4) % 2])
    c["id"] = "%s-D%d-%s_%s%s%s%s%s%s" % (kind, D, c["loss"], c["opt"], "-abs" if c["item_abs"] else "", "-rb" if c["reg_bias"] else "",
                                        "-tail%d" % tail if tail else "", "-frozen%d" % frozen if frozen else "",
                                        "-hyper" if hyper2 else "")
    _CASES.append(c)


for _d in tuple(W.SVDPP) + (1, 5, 16):    # every NJ, last register full and partial, and the narrow rows
    _case(_d)
_case(64, tail=65)                        # the highest ids' runs reach the end of the sorted columns: e < n ends the window
_case(100, tail=129)
_case(64, kind="one")                     # B = 1
_case(33, kind="oneuser", opt="adam")     # a batch of one user
_case(132, kind="oneuser", opt="sgd")
for _bit in range(6):                     # each frozen bit alone, and P with Q
    _case(16, frozen=1 << _bit, opt="adam")
_case(16, frozen=(1 << P) | (1 << Q), opt="adam")
_case(64, hyper2=(1e-3, 0.07), opt="adam")
_case(100, hyper2=(2.0 ** -12, 0.07), opt="sgd")

CASES = tuple(_CASES)
assert len({c["id"] for c in CASES}) == len(CASES)


def seed_of(case):
    return zlib.crc32(case["id"].encode()) & 0x7fffffff


def hyper_of(case, s):
    """(lr, reg) in force at step s"""
    if s >= 1 and case["hyper2"]:
        return case["hyper2"]
    return (ADAM_LR if case["opt"] == "adam" else SGD_LR), LAM


@functools.lru_cache(maxsize=None)
def implicit():
    """(indptr int64 [U + 1], items int32): N(u) of the world, rows strictly increasing"""
    rs = np.random.RandomState(20240)
    fill = np.arange(F0, F0 + N_FILL)
    rows = [[] for _ in range(U)]
    for (L, kind), item in COLS.items():
        na = L if kind == "all" else 0 if kind == "none" else L // 2
        for a in ACT[:na]:
            rows[a].append(item)
        for b in INA[:L - na]:
            rows[b].append(item)
    rows[ACT[5]].append(W0)               # lane 0 active, 63 inactive users above it
    for b in INA[:63]:
        rows[b] += [W0, W63]              # 63 inactive users, then HI[0] in lane 63
    rows[HI[0]].append(W63)
    for a in ACT[:PIECE]:                 # a piece of active users, a piece of inactive ones, then three active users
        rows[a].append(WGAP)
    for b in INA[:PIECE]:
        rows[b].append(WGAP)
    for h in HI[:3]:
        rows[h].append(WGAP)
    rows[T_USER[0]].append(T_ITEM0)
    rows[T_USER[1]].append(T_ITEM1)
    for x, L in enumerate(NSET):
        for k in range(3):
            rows[GA[x, k]] += list(rs.choice(fill, L, replace=False))
    for h in tuple(HI) + T_USER + (TAIL_USER,):
        rows[h] += list(rs.choice(fill, 3, replace=False))
    rows = [np.unique(np.asarray(r_, np.int64)) for r_ in rows]
    indptr = np.concatenate(([0], np.cumsum([r_.size for r_ in rows]))).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def tables_of(case):
    D = case["D"]
    rs = np.random.RandomState(seed_of(case))
    scale = 0.3 / np.sqrt(max(D, 16) / 16)
    f = lambda *s: rs.normal(0, scale, s).astype(np.float32)
    t = dict(mu=np.float32(0.2), bu=f(U), bi=f(I), P=f(U, D), Q=f(I, D), Y=f(I, D))
    t["Q"][ZERO_ITEM, 0] = 0.0
    t["Q"][ZERO_ITEM, D - 1] = 0.0
    return t


def _batch(case, s):
    rs = np.random.RandomState((seed_of(case) + 7919 * (s + 1)) & 0x7fffffff)
    kind, tail = case["kind"], case["tail"]
    if kind == "one":
        u, i = np.array([GA[NSET.index(65), 0]]), np.array([ZERO_ITEM + s])
    elif kind == "oneuser":
        u = np.full(131, GA[NSET.index(129), 0])
        i = rs.choice(RAND_ITEMS, u.size)
        i[:2] = ZERO_ITEM
    else:
        cnt = np.zeros(U, np.int64)
        cnt[ACT] = 1
        cnt[RUN_USER] = RUNS
        cnt[GA[:, 0]] = 1
        cnt[GA[:, 1 + s]] = 1
        cnt[HI] = 1
        cnt[T_USER[s]] = 1
        cnt[TAIL_USER] = tail or 1
        while cnt.sum() % WAVES != 1:                    # B = 1 mod 4: the last block has one wave of work
            cnt[PAD_USER] += 1
        u = rs.permutation(np.repeat(np.arange(U), cnt))
        forced = np.concatenate([np.repeat(RUN_ITEM, RUNS), np.repeat(TAIL_ITEM, tail or 1), [Q_ITEM[s]]])
        i = rs.permutation(np.concatenate((forced, rs.choice(RAND_ITEMS, u.size - forced.size))))
    r = (rs.rand(u.size) < 0.5) if case["loss"] == "nll" else rs.randint(1, 6, u.size)
    return u.astype(np.int32), i.astype(np.int32), r.astype(np.float32)


def transpose(indptr, items):
    """NT as the library builds it: the users of each item, ascending"""
    rowof = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    order = np.argsort(items, kind="stable")
    tip = np.concatenate(([0], np.cumsum(np.bincount(items, minlength=I)))).astype(np.int64)
    return tip, rowof[order].astype(np.int32)


def _assert_edges(case, batches):
    indptr, items = implicit()
    tip, tusers = transpose(indptr, items)
    nlen, clen = np.diff(indptr), np.diff(tip)
    ty = []
    for s, (u, i, _) in enumerate(batches):
        who = "%s step %d: " % (case["id"], s)
        act = np.zeros(U, bool)
        act[u] = True
        assert set(NSET) <= set(nlen[act].tolist()), who + "|N(u)| over the active users"
        assert act[GA[0]].any() and nlen[GA[0, 0]] == 0, who + "an active user with an empty N(u)"
        frac = np.array([act[tusers[tip[j]:tip[j + 1]]].mean() if clen[j] else -1.0 for j in range(I)])
        for L in NSET:
            for kind, ok in (("all", frac == 1), ("none", frac == 0), ("mixed", (frac > 0) & (frac < 1))):
                if (L, kind) in COLS:
                    assert ((clen == L) & (ok | (L == 0))).any(), who + "no column of %d users, %s active" % (L, kind)
        wins, gap = set(), False
        for j in range(I):
            a = act[tusers[tip[j]:tip[j + 1]]]
            pieces = [a[k:k + PIECE] for k in range(0, a.size, PIECE)]
            for p in pieces:
                for k in range(0, p.size, 64):
                    if p[k:k + 64].size == 64:
                        wins.add(p[k:k + 64].tobytes())
            some = [bool(p.any()) for p in pieces]
            gap = gap or any(some[k] and not some[k + 1] and any(some[k + 2:]) for k in range(len(some) - 2))
        lane = lambda *on: np.isin(np.arange(64), on).tobytes()
        assert lane(0) in wins and lane(63) in wins and np.ones(64, bool).tobytes() in wins, who + "the 64-user windows"
        assert gap, who + "no piece without an active user between two that have some"
        assert (frac == 0).any()
        nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
        assert set(RUNS) <= set(nu.tolist()) and set(RUNS) <= set(ni.tolist()), who + "run lengths"
        assert u.max() == TAIL_USER and i.max() == TAIL_ITEM
        if case["tail"]:
            assert nu[TAIL_USER] == case["tail"] and ni[TAIL_ITEM] == case["tail"], who + "the last runs"
        assert u.size % WAVES == 1
        assert ni[ZERO_ITEM] == 2
        t = np.zeros(I, bool)
        for uu in np.flatnonzero(act):
            t[items[indptr[uu]:indptr[uu + 1]]] = True
        ty.append((act, ni > 0, t))
    for a, b in zip(*ty):                                 # rows of step 0 only, of step 1 only, of both: P, Q and Y
        assert (a & ~b).any() and (~a & b).any() and (a & b).any() and (~a & ~b).any()
    assert ty[0][2][T_ITEM0] and not ty[1][2][T_ITEM0] and ty[1][2][T_ITEM1] and not ty[0][2][T_ITEM1]


@functools.lru_cache(maxsize=None)
def _inputs(case_id):
    case = [c for c in CASES if c["id"] == case_id][0]
    batches = tuple(_batch(case, s) for s in range(2))
    t = tables_of(case)
    assert (t["Q"][ZERO_ITEM] == 0).any() and all(ZERO_ITEM in b[1] or case["kind"] == "one" for b in batches)
    if case["kind"] == "edges":
        _assert_edges(case, batches)
    elif case["kind"] == "one":
        assert all(b[0].size == 1 for b in batches)
    else:
        assert all(np.unique(b[0]).size == 1 and b[0].size % WAVES for b in batches)
    return batches


def batch_of(case, s):
    """(u, i, r) of step s"""
    return _inputs(case["id"])[s]
