"""Shared inputs of the snapshot top-K tests (tests/test_bf16_topk_host.py, tests/test_gpu_bf16_topk.py).

The tile, restated from csrc/score_tile.h mfma_tile_dot_bf16: a snapshot row of D elements sits at a stride of
DP = 8 * ceil(D / 8) and is NF = DP / 8 fragments of 8 elements.  K-step s = 0 .. ceil(NF / 2) - 1 gives fragment 2 s + h to
the half-wave h, one v_mfma_f32_32x32x16_bf16 per step; with NF odd the upper half-wave has no fragment in the last step and
its operands are zero on both sides.  The fragments are loaded in groups of four steps ahead of their MFMAs, the last group
masked."""
import functools

import numpy as np

from tfrecomm_amd import bf16
from tests import sliced_cases as SC
from tests.topk_ref import svd_scores, topk_ref

# every (NF odd or even, K-steps of a single load group, or where the last of several groups ends) a supported width reaches
# (tests/test_bf16_topk_host.py guards the list), and both ends of the pads
WIDTHS = [1, 8, 9, 16, 17, 24, 32, 33, 48, 56, 64, 80, 88, 96, 100, 112, 120, 128, 132, 200, 252, 256]

GROUP = 4                                                  # K-steps loaded ahead of their MFMAs


def supported(D):
    """a row width the models accept (csrc/dispatch.h geometry)"""
    return 1 <= D <= 64 or (D % 4 == 0 and D <= 256)


def fragments(D):
    """NF"""
    return bf16.row_stride(D) // 8


def k_steps(D):
    return -(-fragments(D) // 2)


def tile_class(D):
    """(NF is odd: the last step's upper half-wave is zeroed, the K-steps where one load group takes them all or else where
    the last group ends)"""
    s = k_steps(D)
    return fragments(D) % 2 == 1, "%d steps, one group" % s if s <= GROUP else "last group ends at %d" % (s % GROUP)


def fragment_dot(prow, qrow, D):
    """the tile's walk over two packed rows (uint16 [DP]): the products of K-step s, half h are those of features
    16 s + 8 h .. 16 s + 8 h + 7, a missing fragment is zero on both sides; float64 sum of the widened products"""
    nf = fragments(D)
    p = bf16.from_bits(prow).astype(np.float64).reshape(nf, 8)
    q = bf16.from_bits(qrow).astype(np.float64).reshape(nf, 8)
    zero = np.zeros(8)
    acc = 0.0
    for s in range(k_steps(D)):
        for h in (0, 1):
            f = 2 * s + h
            a, b = (q[f], p[f]) if f < nf else (zero, zero)
            assert f >= nf or np.array_equal(np.arange(8 * f, 8 * f + 8), 16 * s + 8 * h + np.arange(8))
            acc += float(np.dot(a, b))
    return acc


# ---------------------------------------------------------------- dyadic tables (tests/test_gpu_topk.py make(dyad=True))
def dyadic(rs, shape, step):
    return (rs.randint(-int(1 / step), int(1 / step) + 1, shape) * step).astype(np.float32)


def dyadic_tables(rs, U, I, D):
    """the draws of tests/test_gpu_topk.py make(dyad=True), in its order"""
    return dict(mu=np.float32(0.25), bu=dyadic(rs, U, .25), bi=dyadic(rs, I, .25), P=dyadic(rs, (U, D), .125),
                Q=dyadic(rs, (I, D), .125))


def dyadic_faults(t):
    """the names of the exactness properties the tables break (empty: any summation order gives the float64 score)"""
    faults = []
    P, Q = t["P"], t["Q"]
    if not (np.array_equal(bf16.round_trip(P), P) and np.array_equal(bf16.round_trip(Q), Q)):
        faults.append("rows are bf16-exact")
    if not (np.array_equal(P * 8, np.rint(P * 8)) and np.array_equal(Q * 8, np.rint(Q * 8))
            and np.abs(P).max() <= 1 and np.abs(Q).max() <= 1):
        faults.append("rows are multiples of 1/8 in [-1, 1]")
    room = np.abs(P.astype(np.float64)).sum(1).max() * np.abs(Q.astype(np.float64)).max()
    if not room < 2 ** 9:                                  # multiples of 1/64 below 2^9: 15 bits
        faults.append("partial sums are multiples of 1/64 below 2^9")
    b = np.concatenate([[t["mu"]], t["bu"], t["bi"]]).astype(np.float64) * 4
    if not (np.array_equal(b, np.rint(b)) and np.abs(b).max() <= 4):
        faults.append("biases are multiples of 1/4 in [-1, 1]")
    return faults


# ---------------------------------------------------------------- the block's cases on round-tripped tables
@functools.lru_cache(maxsize=None)
def sliced_tables(name):
    """the tables of a case of tests/sliced_cases.py as the snapshot holds them"""
    t = SC.BY_NAME[name].tables()
    t = dict(t, P=bf16.round_trip(t["P"]), Q=bf16.round_trip(t["Q"]))
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def sliced_scores(name):
    t = sliced_tables(name)
    with np.errstate(invalid="ignore"):
        S = svd_scores(t["P"], t["Q"], t["bu"], t["bi"], t["mu"], np.arange(SC.NU))
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def sliced_reference(name):
    """(items [NU, k], scores [NU, k]) by distinct user: the contract on the round-tripped tables"""
    c = SC.BY_NAME[name]
    return topk_ref(sliced_scores(name), c.k, [c.excl_of_user(u) for u in range(SC.NU)])


def sliced_expected(name):
    rows = SC.BY_NAME[name].rows()
    wi, ws = sliced_reference(name)
    return wi[rows], ws[rows]


def sliced_scores_f64(name):
    """the same scores with every operation in float64"""
    t = sliced_tables(name)
    with np.errstate(invalid="ignore"):
        S = t["P"].astype(np.float64) @ t["Q"].astype(np.float64).T
        return ((S + np.float64(t["mu"])) + t["bu"].astype(np.float64)[:, None]) + t["bi"].astype(np.float64)[None, :]
