"""The cases of tests/test_gpu_shard_stages.py and tests/test_gpu_dp_stages.py as plain data, with their seeded inputs:
shared with the host tests (tests/test_shard_stages_host.py runs the same list through the in-process world on the CPU;
the width guards of tests/test_width_coverage.py read the two width lists they are built from)."""
import numpy as np

from tests import step_cases as S
from tests import widths as W
from tests.util import dup_heavy_ids, rand_tables

OPTS = (S.ADAM_TF1, S.ADAM_LAZY, S.SGD)
_CASES = []


def _case(world, U, I, D, B, opt, ids="dup", form="route", frozen=0, hyper2=None, presort=False):
    x = len(_CASES)                       # loss form and flags rotate as in step_cases._case
    c = dict(world=world, U=U, I=I, D=D, B=B, opt=opt[0], mode=opt[1], loss=("mse", "nll")[x % 2], item_abs=bool((x >> 1) & 1),
             reg_bias=bool((x >> 2) & 1), ids=ids, form=form, frozen=frozen, hyper2=hyper2, presort=presort, sample=None)
    c["id"] = "w%d-U%d-I%d-D%d-B%d-%s_%s-%s-%s%s%s%s" % (world, U, I, D, B, opt[0], opt[1], ids, form, "-frozen%d" % frozen if frozen else "",
                                                      "-hyper" if hyper2 else "", "-presort" if presort else "")
    _CASES.append(c)


# every (G, VEC, full width) class; worlds 1..4 and the three optimisers rotate; row counts that do not divide by the world
for _k, _d in enumerate(W.SHARD):
    _case(1 + _k % 4, 301, 203, _d, 1500, OPTS[_k % 3])
# a rank that owns no rows (I, then U, smaller than the world: per = 1, the last ranks stay empty)
_case(4, 50, 3, 16, 400, S.ADAM_LAZY)
_case(4, 3, 50, 13, 400, S.ADAM_TF1)
# a rank that owns rows and receives no sample: every user id lies in ranks 0 and 1's blocks
_case(3, 300, 200, 28, 600, S.SGD, ids="low_users")
# hot: one item on half of the batch - on some rank slots written whole by the reduce AND slots cut by a block boundary
_case(2, 400, 300, 128, 3000, S.ADAM_LAZY, ids="hot")
_case(3, 400, 300, 64, 3000, S.ADAM_TF1, ids="hot")
_case(4, 400, 300, 7, 4000, S.SGD, ids="hot")
_case(2, 400, 300, 100, 2000, S.SGD, ids="hot", presort=True)
# one item only: every rank asks one owner for one row
_case(3, 200, 100, 36, 900, S.ADAM_LAZY, ids="one_item")
_case(2, 200, 100, 31, 900, S.ADAM_TF1, ids="one_item")
# the routing forms that fill R.r / R.u from the store: the global batch as store rows, and pre-split batches
_case(3, 301, 203, 64, 1500, S.ADAM_LAZY, form="route_ids")
_case(3, 301, 203, 12, 1500, S.ADAM_TF1, form="recs")
_case(2, 301, 203, 61, 1500, S.SGD, form="recs", presort=True)
# frozen sides, set_hyper between the two steps (on every rank)
_case(2, 301, 203, 64, 1500, S.ADAM_TF1, frozen=S.FROZEN_ITEM_SIDE)
_case(3, 301, 203, 32, 1500, S.ADAM_LAZY, frozen=S.FROZEN_USER_SIDE)
_case(2, 301, 203, 64, 1500, S.ADAM_TF1, hyper2=(1e-3, 0.07))
_case(3, 301, 203, 13, 1500, S.ADAM_LAZY, hyper2=(1e-3, 0.07))
_case(4, 301, 203, 16, 1500, S.SGD, hyper2=(2.0 ** -12, 0.07))

CASES = tuple(_CASES)
assert len({c["id"] for c in CASES}) == len(CASES)

# bit-identical pairs (two worlds of two ranks alive at a time): forward_reduce against forward_items + reduce_users, and
# presort(req_recv) ahead of the compute stages against none
PAIR_CASES = tuple(c for c in CASES if c["world"] == 2 and not c["presort"])
# the void step: a VEC = 4 and a VEC = 1 width (the flag sits at D + 1 of a stride of D + 4, or of D + 2)
VOID_WIDTHS = (64, 6)

seed_of, hyper_of = S.seed_of, S.hyper_of


def tables_of(case):
    D = case["D"]
    return rand_tables(np.random.RandomState(seed_of(case)), case["U"], case["I"], D, scale=0.3 / np.sqrt(max(D, 16) / 16))


def batch_of(case, s):
    """(u, i, r) of the global batch of step s"""
    U, I, B, kind = case["U"], case["I"], case["B"], case["ids"]
    rs = np.random.RandomState((seed_of(case) + 7919 * (s + 1)) & 0x7fffffff)
    u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    if kind == "hot":                     # as step_cases.batch_of: one item on half of the batch, one user on a third of it
        u, i = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
        i[rs.rand(B) < 0.5] = (I // 3 + s) % I
        u[rs.rand(B) < 0.33] = (U // 5 - s) % U
    elif kind == "uniform":               # no case; what a hot case must not degrade to (tests/test_shard_stages_host.py)
        u, i = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
    elif kind == "one_item":
        i = np.full(B, I // 2, np.int32)
    elif kind == "low_users":
        u = (u % (2 * -(-U // case["world"]))).astype(np.int32)
    elif kind != "dup":
        raise ValueError(kind)
    r = (rs.rand(B) < 0.5).astype(np.float32) if case["loss"] == "nll" else rs.randint(1, 6, B).astype(np.float32)
    return u, i, r


# ----------------------------------------------------------------------------- data parallel
_DP = []


def _dp_case(path, U, I, D, B, opt, form):
    x = len(_DP)
    c = dict(path=path, U=U, I=I, D=D, B=B, opt=opt[0], mode=opt[1], loss=("mse", "nll")[x % 2], item_abs=bool((x >> 1) & 1),
             reg_bias=bool((x >> 2) & 1), form=form, ids="dup")
    c["id"] = "dp-%s-U%d-I%d-D%d-B%d-%s_%s-%s" % (path, U, I, D, B, opt[0], opt[1], form)
    _DP.append(c)


# B is one replica's half of the global batch.  Tile path: both tables at most 16384 rows, B at most 16 tiles; sort path: a
# table above 16384 rows.  The tile cases run k_dense_tiles at 4, 8, 10, 12 and 16 tiles.  Optimiser and batch form alternate out of step with each other.
for _k, _d in enumerate(W.DP):
    _dp_case("tiles", 300, 200, _d, (700, 5000, 9500, 12000, 16000)[_k % 5], (S.ADAM_TF1, S.SGD)[_k % 2], ("columns", "store")[(_k // 2) % 2])
for _k, _d in enumerate(W.DP):
    _dp_case("sort", 16384 + 77, 300, _d, 1500, (S.SGD, S.ADAM_TF1)[_k % 2], ("store", "columns")[(_k // 2) % 2])
DP_CASES = tuple(_DP)
assert len({c["id"] for c in DP_CASES}) == len(DP_CASES)


def dp_batch_of(case, s):
    """the global batch of step s: two halves of B"""
    U, I, B = case["U"], case["I"], 2 * case["B"]
    rs = np.random.RandomState((seed_of(case) + 7919 * (s + 1)) & 0x7fffffff)
    u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    r = (rs.rand(B) < 0.5).astype(np.float32) if case["loss"] == "nll" else rs.randint(1, 6, B).astype(np.float32)
    return u, i, r
