"""Shared pieces of the snapshot ranking and neighbours tests (tests/test_bf16_rank_host.py, tests/test_gpu_bf16_rank.py,
tests/test_gpu_bf16_neighbours.py): the inverse norms of packed snapshot rows restated in float32 NumPy, and the float64
bracket a rank on rounded scores has to fall in."""
import numpy as np

from tfrecomm_amd import bf16


def packed_ss(rows):
    """ss [R] float32 of packed rows (uint16 [R, DP], ``bf16.pack_rows``), as csrc/bf16_neighbours.hip k_row_rnorm_bf16
    states it: over every element of the row, pads included, ascending, ss = fmaf(x, x, ss) from +0 with x the widened
    element.  x * x is exact in float32 (8 + 8 significand bits), so the fmaf is one float32 multiply and one float32 add."""
    x = bf16.from_bits(np.ascontiguousarray(rows, np.uint16))
    ss = np.zeros(x.shape[0], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for f in range(x.shape[1]):
            sq = x[:, f] * x[:, f]
            assert sq.dtype == np.float32
            ss = ss + sq
    return ss


def packed_rnorm(rows):
    """rn [R] float32: 1 / sqrtf(ss), 0 where ss == 0"""
    ss = packed_ss(rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = np.float32(1) / np.sqrt(ss, dtype=np.float32)
    return np.where(ss == 0, np.float32(0), rn).astype(np.float32)


def rank_bracket(s64, elig, t, tol):
    """(lo, hi) of an eligible target t of one float64 score row: every ranking by scores within tol of s64 puts t at a
    rank in [lo, hi].  A score moved by at most tol changes a comparison only between scores closer than 2 tol."""
    lo = int(np.count_nonzero(elig & (s64 > s64[t] + 2 * tol)))
    hi = int(np.count_nonzero(elig & (s64 >= s64[t] - 2 * tol))) - 1
    return lo, hi
