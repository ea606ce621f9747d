"""The bf16 snapshot's number format and row layout, restated in NumPy (csrc/bf16_rows.h).

Element: the upper 16 bits of the float32, rounded to nearest, ties to even:
``(bits + 0x7FFF + ((bits >> 16) & 1)) >> 16`` for everything that is not a NaN - overflow past the largest finite
value rounds to +-inf, subnormals round like any other value - and ``(bits >> 16) | 0x40`` for a NaN (sign kept,
quiet, never inf).  Widening is ``bits << 16`` and exact.

Row: ``D`` elements at a stride of ``DP = 8 * ceil(D / 8)`` elements, the pad elements +0.

Geometry: the forward spreads a rating over ``lanes(D)`` lanes, the smallest power of two >= DP / 8.
"""
import numpy as np


def row_stride(D):
    return 8 * -(-int(D) // 8)


def lanes(D):
    g = 1
    while g * 8 < row_stride(D):
        g *= 2
    return g


def to_bits(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (b.astype(np.uint64) + np.uint64(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    return np.where(nan, (b >> np.uint32(16)) | np.uint32(0x40), r).astype(np.uint16)


def from_bits(h):
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_trip(x):
    """``x`` as the snapshot holds it: float32 values that are exactly bf16."""
    return from_bits(to_bits(x))


def pack_rows(table):
    """float [rows, D] -> uint16 [rows, DP], as ``SvdModel.bf16_rows`` returns them."""
    t = np.asarray(table, np.float32)
    if t.ndim != 2:
        raise ValueError("a table is [rows, D]")
    out = np.zeros((t.shape[0], row_stride(t.shape[1])), np.uint16)
    out[:, :t.shape[1]] = to_bits(t)
    return out
