"""The cases of tests/test_gpu_step_gradients.py as plain data, with their seeded inputs: shared with the host tests
(tests/test_step_ref_host.py runs the float32 oracle on the small ones; the path-coverage guard reads the list).

A case names the step path it was written for (``path``); the GPU test holds ``kernel_plan`` against it and the guard
holds the restated dispatch rule against it, so a case cannot migrate to another path unnoticed."""
import zlib

import numpy as np

from tests.util import dup_heavy_ids, rand_tables

ADAM_TF1, ADAM_LAZY, SGD = ("adam", "tf1"), ("adam", "lazy"), ("sgd", "tf1")
SGD_LR = 2.0 ** -10                       # a power of two (the gradient is read back as (w - w') / lr), small enough for hot rows
ADAM_LR, REG = 3e-3, 0.02
MU, BU, BI, P, Q = 0, 1, 2, 3, 4          # include/tfrecomm.h
FROZEN_ITEM_SIDE = (1 << MU) | (1 << BI) | (1 << Q)
FROZEN_USER_SIDE = (1 << BU) | (1 << P)

_CASES = []


def _case(path, U, I, D, B, opt, ids="dup", frozen=0, hyper2=None, sample=None, item_abs=None, tables="rand"):
    x = len(_CASES)                       # loss form and flags rotate as in test_gpu_parity._rotation
    c = dict(path=path, U=U, I=I, D=D, B=B, opt=opt[0], mode=opt[1], loss=("mse", "nll")[x % 2],
             item_abs=bool((x >> 1) & 1) if item_abs is None else item_abs,
             reg_bias=bool((x >> 2) & 1), ids=ids, frozen=frozen, hyper2=hyper2, sample=sample, tables=tables)
    c["id"] = "%s-U%d-I%d-D%d-B%d-%s_%s-%s%s%s%s" % (path, U, I, D, B, opt[0], opt[1], ids, "-frozen%d" % frozen if frozen else "",
                                                "-hyper" if hyper2 else "", "-" + tables if tables != "rand" else "")
    _CASES.append(c)


# k_tile_step + k_dense_tiles<.., 4 / 8 / 10 / 12 / 16>
for _o in (ADAM_TF1, ADAM_LAZY, SGD):
    _case("tiles4", 500, 300, 64, 700, _o)
_case("tiles10", 6040, 3952, 64, 10000, ADAM_TF1)                    # the headline configuration
_case("tiles8", 6040, 3952, 64, 8000, ADAM_LAZY)
_case("tiles12", 6040, 3952, 32, 12288, SGD)
_case("tiles16", 6040, 3952, 128, 12289, ADAM_LAZY)
_case("tiles16", 16384, 500, 128, 16384, SGD)                        # a full 16384-row table
_case("tiles4", 6040, 3952, 15, 1000, ADAM_TF1)                      # VEC = 1 rows
# the same path on constructed runs: 1, 2, 15, 16 waves of a piece, pieces across tiles (tests/test_gpu_tile_pieces._batch)
_case("tiles4", 3000, 2000, 64, 3 * 1024 + 500, ADAM_TF1, ids="runs")
_case("tiles4", 3000, 2000, 64, 3 * 1024 + 500, SGD, ids="runs")
_case("tiles10", 6040, 3952, 64, 10000, ADAM_LAZY, ids="runs")
# k_front + k_csort_scan/scatter: the first B past the tile path; several csort tiles
_case("csort", 6040, 3952, 32, 16385, ADAM_TF1)
_case("csort", 6040, 3952, 32, 16385, SGD)
_case("csort", 6040, 3952, 64, 65536, ADAM_LAZY, sample=2000)
# small tables, B past csort_eligible: small_tables is true while csort_path is false
_case("tf1_small", 6040, 3952, 64, 300000, ADAM_TF1, sample=2000)
_case("fused_small", 6040, 3952, 64, 300000, ADAM_LAZY, sample=2000)
# radix sort + k_adam_dense: one side small and one big, both big
for _d in (12, 64, 100):
    _case("tf1_big", 16384 + 77, 300, _d, 3000, ADAM_TF1)
_case("tf1_big", 20000, 17000, 32, 5000, ADAM_TF1)
# radix sort + fused k_seg_reduce + k_apply_rows: three-round (D = 128, 16) and general (D = 20) load form, hot rows cut
# into hundreds of pieces, ragged and single-entry batches
_case("fused_big", 40000, 30000, 128, 20000, ADAM_LAZY, ids="hot")
_case("fused_big", 40000, 30000, 128, 20000, SGD, ids="hot")
_case("fused_big", 40000, 30000, 20, 20000, ADAM_LAZY, ids="hot")
_case("fused_big", 70000, 20000, 16, 1057, SGD)
_case("fused_big", 40000, 30000, 128, 1, ADAM_LAZY)
# two-table form: the second step re-touches the item rows of the first
_case("fused_big", 40000, 30000, 64, 20000, ADAM_LAZY, ids="retouch")
_case("fused_big", 40000, 30000, 64, 20000, SGD, ids="retouch")
# the longest possible runs
for _o in (ADAM_TF1, ADAM_LAZY, SGD):
    _case("tiles8", 10, 10, 64, 5000, _o, ids="same")
_case("tiles10", 3, 2, 64, 9000, ADAM_LAZY)
_case("tiles10", 3, 2, 64, 9000, ADAM_TF1)
# frozen tables, one case per path
_case("tiles4", 500, 300, 64, 700, ADAM_TF1, frozen=FROZEN_ITEM_SIDE)
_case("csort", 6040, 3952, 32, 16385, ADAM_LAZY, frozen=FROZEN_USER_SIDE)
_case("tf1_big", 16384 + 77, 300, 12, 3000, ADAM_TF1, frozen=FROZEN_ITEM_SIDE)
_case("fused_big", 70000, 20000, 16, 1057, ADAM_LAZY, frozen=FROZEN_USER_SIDE)
# set_hyper between the two steps: the second step's gradient carries reg2, its alpha (or the SGD step) lr2
_case("tiles4", 500, 300, 64, 700, ADAM_TF1, hyper2=(1e-3, 0.07))
_case("tiles4", 500, 300, 64, 700, SGD, hyper2=(2.0 ** -12, 0.07))
_case("fused_big", 70000, 20000, 16, 1057, ADAM_LAZY, hyper2=(1e-3, 0.07))
_case("fused_big", 70000, 20000, 16, 1057, SGD, hyper2=(2.0 ** -12, 0.07))
# exact zeros in Q under item_abs (d|q|/dq = sign(q), sign(0) = 0: svd_kernels.hip k_tile_step, k_seg_reduce), planted by
# ``tables_of`` in rows both steps touch; the tile path at VEC = 4 and VEC = 1, the three-round and the general load form
_case("tiles4", 500, 300, 64, 700, ADAM_TF1, item_abs=True, tables="zeros")
_case("tiles4", 500, 300, 15, 700, SGD, item_abs=True, tables="zeros")
_case("csort", 6040, 3952, 32, 16385, ADAM_LAZY, item_abs=True, tables="zeros")
_case("tf1_big", 16384 + 77, 300, 12, 3000, ADAM_TF1, item_abs=True, tables="zeros")
_case("fused_big", 70000, 20000, 16, 1057, SGD, item_abs=True, tables="zeros")
_case("fused_big", 40000, 30000, 20, 20000, ADAM_LAZY, ids="hot", item_abs=True, tables="zeros")

CASES = tuple(_CASES)
assert len({c["id"] for c in CASES}) == len(CASES)


def seed_of(case):
    return zlib.crc32(case["id"].encode()) & 0x7fffffff


def tables_of(case):
    D = case["D"]
    t = rand_tables(np.random.RandomState(seed_of(case)), case["U"], case["I"], D, scale=0.3 / np.sqrt(max(D, 16) / 16))
    if case["tables"] == "zeros":
        for row, cols, vals in zero_plan(case):
            t["Q"][row, cols] = vals
    return t


def zero_plan(case):
    """[(Q row, columns, values)] of the planted zeros: a hot row and a once-seen row carry +0.0 and -0.0 at columns 0
    and D - 1, one 4-column fragment all zero and one partly zero; a third row is zero altogether.  All three rows occur
    in both steps' batches (asserted)."""
    D, I = case["D"], case["I"]
    assert D >= 12
    n0, n1 = (np.bincount(batch_of(case, s)[1], minlength=I) for s in range(2))
    both = np.minimum(n0, n1)
    hot = int(np.argmax(np.where(both > 0, n0, 0)))                     # the longest first-step run the second step meets again
    once = np.flatnonzero((n0 == 1) & (n1 >= 1))
    assert n0[hot] >= 2 and both[hot] >= 1 and once.size, (case["id"], n0[hot], once.size)
    once = int(once[np.argmin(n1[once])])
    rest = np.flatnonzero((both > 0) & (np.arange(I) != hot) & (np.arange(I) != once))
    whole = int(rest[rest.size // 2])
    pz, nz = np.float32(0.0), np.float32(-0.0)
    cols = np.array([0, D - 1, 4, 5, 6, 7, 9, 10])
    alt = np.where(np.arange(D) % 2 == 0, pz, nz).astype(np.float32)
    return [(hot, cols, np.array([pz, nz, pz, nz, nz, pz, nz, pz], np.float32)),
            (once, cols, np.array([nz, pz, nz, nz, pz, pz, pz, nz], np.float32)),
            (whole, np.arange(D), alt)]


def assert_zero_edges(case):
    """what a "zeros" case was built for holds: the planted elements are zeros of both signs, their rows are touched in
    both steps, and the float64 gradient there is exactly lam * 0"""
    from tests import step_ref
    assert case["item_abs"] and case["tables"] == "zeros"
    t = tables_of(case)
    u, i, r = batch_of(case, 0)
    G = step_ref.step_grads(t, u, i, r, case["loss"], True, case["reg_bias"], REG)[0]["Q"][0]
    touched = [np.bincount(batch_of(case, s)[1], minlength=case["I"]) for s in range(2)]
    signs = set()
    for row, cols, vals in zero_plan(case):
        assert touched[0][row] > 0 and touched[1][row] > 0, (case["id"], row)
        got = t["Q"][row, cols]
        assert np.all(got == 0) and np.array_equal(np.signbit(got), np.signbit(vals))
        signs |= set(np.signbit(got).tolist())
        assert np.all(G[row, cols] == 0), (case["id"], row, G[row, cols])
        assert np.any(G[row] != 0) or cols.size == case["D"]           # the rest of the row does move
    assert signs == {True, False}


def batch_of(case, s):
    """(u, i, r) of step s"""
    U, I, B, kind = case["U"], case["I"], case["B"], case["ids"]
    rs = np.random.RandomState((seed_of(case) + 7919 * (s + 1)) & 0x7fffffff)
    if kind == "dup":
        u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    elif kind == "runs":
        from tests.test_gpu_tile_pieces import _batch
        u, i, _, _ = _batch(rs, U, I, B)
    elif kind == "hot":                   # one item on half of the batch, one user on a third of it
        u, i = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
        i[rs.rand(B) < 0.5] = 4242 + s
        u[rs.rand(B) < 0.33] = 31000 - s
    elif kind == "retouch":               # the same 400 item rows in every step, one of them on a tenth of the batch
        hot = np.random.RandomState(seed_of(case)).randint(0, I, 400)
        u = rs.randint(0, U, B).astype(np.int32)
        i = np.where(rs.rand(B) < 0.6, hot[rs.randint(0, 400, B)], rs.randint(0, I, B)).astype(np.int32)
        i[rs.rand(B) < 0.1] = hot[0]
    elif kind == "same":
        u, i = np.full(B, 3, np.int32), np.full(B, 7, np.int32)
    else:
        raise ValueError(kind)
    r = (rs.rand(B) < 0.5).astype(np.float32) if case["loss"] == "nll" else rs.randint(1, 6, B).astype(np.float32)
    return u, i, r


def hyper_of(case, s):
    """(lr, reg) in force at step s"""
    if s >= 1 and case["hyper2"]:
        return case["hyper2"]
    return (ADAM_LR if case["opt"] == "adam" else SGD_LR), REG


# ----------------------------------------------------------------------------- the dispatch rule, restated
CSORT_TILE, CSORT_MAX_BINS, MAX_TILES, MAX_BINS_X_TILES = 1024, 16384, 16, 1 << 20      # csrc/svd_kernels.h, sort.hip, api.hip


def bits_for(rows):
    b = 1
    while (1 << b) < rows and b < 31:
        b += 1
    return b


def path_of(U, I, B, opt, mode):
    """the four-way branch of tfr_kernel_plan (csrc/api.hip): tiles_eligible, fwd_in_reduce, csort_path, else"""
    bins = 1 << max(bits_for(U), bits_for(I))
    small = bins <= CSORT_MAX_BINS
    ntiles = -(-B // CSORT_TILE)
    csort = small and bins * ntiles <= MAX_BINS_X_TILES
    tf1 = opt == "adam" and mode == "tf1"
    if csort and ntiles <= MAX_TILES:
        return "tiles%d" % (4 if ntiles <= 4 else 8 if ntiles <= 8 else 10 if ntiles <= 10 else 12 if ntiles <= 12 else 16)
    if not tf1 and not csort:
        return "fused_small" if small else "fused_big"
    if csort:
        return "csort"
    return "tf1_small" if small else "tf1_big"
