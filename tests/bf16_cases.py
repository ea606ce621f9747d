"""Shared inputs of the bf16 snapshot tests (tests/test_bf16_host.py, tests/test_gpu_bf16.py)."""
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
    """ratings per block and grid-stride turn: 4 waves x 64 / G groups x UNR (csrc/bf16_rows.hip bf16_forward_grid)"""
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
