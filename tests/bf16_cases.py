"""Shared inputs of the bf16 snapshot tests (tests/test_bf16_host.py, tests/test_gpu_bf16.py)."""
import functools

import numpy as np

from tfrecomm_amd import bf16
from tests.util import rand_tables

# both ends of every lane-group size and every kind of pad (tests/test_bf16_host.py guards the list)
WIDTHS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 100, 128, 132, 200, 252, 256]

# |dot of the bf16 rows - dot of the float32 rows| <= QBOUND * sum |p||q| for normal-range values: the unit roundoff of
# round-to-nearest bf16 is 2^-8 per factor, (1 + 2^-8)^2 - 1 = 2^-7 + 2^-16
QBOUND = 2.0 ** -7 + 2.0 ** -16


def row_stride(D):
    """DP (csrc/bf16_rows.h bf16_row_stride)"""
    return 8 * -(-D // 8)


def lanes(D):
    """lanes per rating: the smallest power of two >= DP / 8 (csrc/bf16_rows.h bf16_geometry)"""
    g = 1
    while g * 8 < row_stride(D):
        g *= 2
    return g


def unroll(G):
    """ratings in flight per lane group (csrc/bf16_rows.h bf16_unroll)"""
    return min(G, 4)


def per_block(D):
    """ratings per block and grid-stride turn: 4 waves x 64 / G groups x UNR (csrc/svd_kernels.hip forward_grid at
    bf16_unroll)"""
    g = lanes(D)
    return 4 * (64 // g) * unroll(g)


EDGE_BITS = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                # +-0, +-inf
    0x3F800000, 0x3F7FFFFF, 0x3F800001,                            # 1 and its neighbours
    0x3F808000, 0x3F818000,                                        # ties: down to even, up to even
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,                # one ulp either side of a tie
    0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000, 0xFF7F7FFF,                # rounds to inf / stays finite
    0x00008000, 0x80008000, 0x00008001, 0x80008001, 0x00007FFF, 0x80007FFF,   # halves of the smallest subnormal
    0x00010000, 0x007FFFFF,                                        # smallest bf16 subnormal, largest float32 subnormal
], np.uint32)
NAN_BITS = np.array([0x7F800001, 0xFFC12345, 0x7FBFFFFF], np.uint32)


def random_values(seed=0):
    """202 000 values: N(0, 1) at scales 0.3, 1e-40 (subnormal) and 1e38 (overflow to inf at the tail)"""
    rs = np.random.RandomState(seed)
    with np.errstate(over="ignore"):
        parts = [(rs.standard_normal(n) * s).astype(np.float32) for n, s in ((100000, 0.3), (51000, 1e-40), (51000, 1e38))]
    return np.concatenate(parts)


def torch_bits(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def planted_table(rs, rows, D):
    """random [rows, D] with the edge list and the NaNs at random distinct places (rows * D >= their count)"""
    t = rs.normal(0, 0.3, (rows, D)).astype(np.float32)
    plant = np.concatenate([EDGE_BITS, NAN_BITS])
    assert t.size >= plant.size
    where = rs.permutation(t.size)[:plant.size]
    t.reshape(-1).view(np.uint32)[where] = plant
    return t


def snapshot_tables(t):
    """the tables as the snapshot holds them: rows exactly bf16, biases float32"""
    return dict(t, P=bf16.round_trip(t["P"]), Q=bf16.round_trip(t["Q"]))


def sum_abs(t, u, i):
    """sum |p||q| per pair, float64"""
    return np.einsum("bd,bd->b", np.abs(t["P"][u].astype(np.float64)), np.abs(t["Q"][i].astype(np.float64)))


# eval case: the shape of test_eval_sse_and_accuracy.  The seed was picked on the CPU so that no oracle logit of the
# round-tripped tables lies within 1e-4 of 0, where round(sigmoid(x)) may flip: the +-2 allowance hides nothing
# (tests/test_bf16_host.py checks the property).
EVAL_SHAPE = (200, 150, 15, 30001)
EVAL_SEED = 7


def eval_case(loss):
    U, I, D, N = EVAL_SHAPE
    rs = np.random.RandomState(EVAL_SEED)
    t = rand_tables(rs, U, I, D)
    u, i = rs.randint(0, U, N), rs.randint(0, I, N)
    r = (rs.rand(N) < 0.5).astype(np.float32) if loss == "nll" else rs.randint(1, 6, N).astype(np.float32)
    return t, u, i, r


# ---------------------------------------------------------------- the exact case
# One forward body serves float32 rows and snapshot rows (csrc/forward_body.h).  On these inputs every partial sum of
# the forward and of the mse evaluation is exactly representable in float32 whatever the order it is added in, so the
# float32 entries, the snapshot entries and a float64 evaluation have to agree bit for bit: P and Q are small integers
# (bf16-exact), mu, bu and bi multiples of 1/2, rates integers.  A dot product's partial sums are integers of
# magnitude <= sum |p||q| <= 9 * 64 or 4 * 256; a logit is a multiple of 1/2 below 2^11; (infer - rate)^2 is a multiple
# of 1/4, and the sizes keep 4 * (the whole batch's sum of them) below 2^24, which bounds every block's partial sums in
# every order.  exactness_faults states these properties and tests/test_bf16_host.py holds the case to them.
EXACT_TABLES = (40, 30)


def exact_case(D, item_abs, seed=None):
    """(tables, u, i, r) at B = 3 * per_block(D) + 5: four blocks, the last one with 5 ratings.  A third of the
    ratings whose logit is an integer are rated exactly that, so that n_equal counts something."""
    U, I = EXACT_TABLES
    B = 3 * per_block(D) + 5
    rs = np.random.RandomState(7000 + 2 * D + int(item_abs) if seed is None else seed)
    A = 3 if D <= 64 else 2
    t = dict(mu=np.float32(0.5 * rs.randint(-4, 5)), bu=(0.5 * rs.randint(-4, 5, U)).astype(np.float32),
             bi=(0.5 * rs.randint(-4, 5, I)).astype(np.float32),
             P=rs.randint(-A, A + 1, (U, D)).astype(np.float32), Q=rs.randint(-A, A + 1, (I, D)).astype(np.float32))
    u, i = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
    r = rs.randint(1, 6, B).astype(np.float32)
    x = exact_logits(t, u, i, item_abs)
    hit = (x == np.rint(x)) & (np.arange(B) % 3 == 0)
    r[hit] = x[hit]
    return t, u, i, r


def exact_logits(t, u, i, item_abs):
    """float64"""
    q = t["Q"][i].astype(np.float64)
    dot = np.einsum("bd,bd->b", t["P"][u].astype(np.float64), np.abs(q) if item_abs else q)
    return dot + np.float64(t["mu"]) + t["bu"][u].astype(np.float64) + t["bi"][i].astype(np.float64)


def exact_eval(t, u, i, r, item_abs):
    """(sse, n_equal) of the mse head, float64"""
    x = exact_logits(t, u, i, item_abs)
    return float(np.sum((x - r) ** 2)), int(np.sum(x == r))


def f32_logits(t, u, i, item_abs, reverse):
    """the forward in float32, one add at a time: features ascending and ((s + mu) + bu) + bi as the kernels have it,
    or features descending and the biases first"""
    q = t["Q"][i]
    prod = (t["P"][u] * (np.abs(q) if item_abs else q)).astype(np.float32)
    s = np.zeros(len(u), np.float32)
    for d in (range(prod.shape[1] - 1, -1, -1) if reverse else range(prod.shape[1])):
        s = (s + prod[:, d]).astype(np.float32)
    mu, bu, bi = np.float32(t["mu"]), t["bu"][u], t["bi"][i]
    return (s + ((bi + bu) + mu)).astype(np.float32) if reverse else (((s + mu) + bu) + bi).astype(np.float32)


def exactness_faults(t, u, i, r, item_abs):
    """the names of the exactness properties the case breaks (empty: float32 in any order == float64)"""
    faults = []
    P, Q = t["P"], t["Q"]
    if not (np.array_equal(P, np.rint(P)) and np.array_equal(Q, np.rint(Q))
            and np.array_equal(bf16.round_trip(P), P) and np.array_equal(bf16.round_trip(Q), Q)):
        faults.append("rows are bf16-exact integers")
    halves = np.concatenate([[t["mu"]], t["bu"], t["bi"]]).astype(np.float64) * 2
    if not (np.array_equal(halves, np.rint(halves)) and np.array_equal(r, np.rint(r))):
        faults.append("biases are multiples of 1/2, rates integers")
    x = exact_logits(t, u, i, item_abs)
    room = sum_abs(t, u, i) + abs(float(t["mu"])) + np.abs(t["bu"][u]) + np.abs(t["bi"][i])
    if not (2 * room < 2 ** 24).all():
        faults.append("logit partial sums fit 24 bits")
    fwd, rev = f32_logits(t, u, i, item_abs, False), f32_logits(t, u, i, item_abs, True)
    if not (np.array_equal(fwd.astype(np.float64), x) and np.array_equal(rev.astype(np.float64), x)):
        faults.append("float32 logits in two orders equal float64")
    d2 = (x - r) ** 2
    if not (np.array_equal(4 * d2, np.rint(4 * d2)) and 4 * d2.sum() < 2 ** 24):
        faults.append("squared errors are quarters and their sum fits 24 bits")
    d2f = ((fwd - r) * (fwd - r)).astype(np.float32)
    up, down = np.cumsum(d2f, dtype=np.float32)[-1], np.cumsum(d2f[::-1], dtype=np.float32)[-1]
    if not (float(up) == float(down) == float(d2.sum())):
        faults.append("float32 sse in two orders equals float64")
    return faults


@functools.lru_cache(maxsize=None)
def exact_reference(D, item_abs):
    """the case and what every entry has to return: logits as float32 (the float64 values, exactly), sse, n_equal"""
    t, u, i, r = exact_case(D, item_abs)
    sse, neq = exact_eval(t, u, i, r, item_abs)
    return t, u, i, r, exact_logits(t, u, i, item_abs).astype(np.float32), sse, neq
