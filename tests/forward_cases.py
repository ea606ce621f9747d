"""Shared inputs of the forward-path tests (tests/test_forward_paths_host.py, tests/test_gpu_forward_paths.py): what the
dispatch launches for a shape (tfr_forward_plan), the smallest user table that takes the non-temporal loads, and the exact
and the random case of tests/bf16_cases.py with their 40 user rows spread over such a table.

The rule, restated from csrc/svd_kernels.h: INFER and EVAL read the user rows by non-temporal loads (PNT) where the user
table is larger than 256 MB - stream_user_rows(U, row_bytes), row_bytes = 4 D for float32 rows and 2 DP for snapshot rows."""
import ctypes

import numpy as np

from tests import bf16_cases as BC
from tests.util import rand_tables

INFER, TRAIN, EVAL = 0, 1, 2                               # csrc/svd_kernels.h MODE_*
F32, BF16 = 0, 1                                           # tfr_forward_plan's rows
CACHE_BYTES = 256 << 20                                    # csrc/svd_kernels.h stream_user_rows
INFER_CAP, EVAL_CAP = 8192, 2048                           # csrc/svd_kernels.hip forward_grid


def geometry(D):
    """(G, VEC) of the float32 forward (csrc/svd_kernels.h geometry), as tests/test_width_coverage.py restates it"""
    vec = 4 if D % 4 == 0 else 1
    g = 4
    while g < -(-D // vec):
        g *= 2
    return g, vec


def per_block(D):
    """ratings per block and grid-stride turn of k_forward: 4 waves x 64 / G groups x 4 in flight (forward_grid)"""
    return 4 * (64 // geometry(D)[0]) * 4


def row_bytes(D, rows):
    return 4 * D if rows == F32 else 2 * BC.row_stride(D)


def pnt_rows(D, row_bytes):
    """the smallest U with U * row_bytes > 256 MB"""
    return CACHE_BYTES // row_bytes + 1


def plan_text(D, U, mode, rows, batch, buflen=128):
    """(return code, text) of tfr_forward_plan; needs no device"""
    from tfrecomm_amd import _lib as L
    buf = ctypes.create_string_buffer(max(1, buflen))
    rc = L.load().tfr_forward_plan(D, U, mode, rows, batch, buf, buflen)
    return rc, buf.value.decode()


def plan(D, U, mode, rows, batch=1):
    """(kernel name, template arguments, grid): ("k_forward", (G, VEC, MODE, 4, PNT), N) or
    ("k_forward_bf16", (G, MODE, UNR, PNT), N)"""
    rc, text = plan_text(D, U, mode, rows, batch)
    assert rc == 0, (D, U, mode, rows, batch, rc)
    kernel, grid = text.split(";grid=")
    name, args = kernel[:-1].split("<")
    return name, tuple(a == "true" if a in ("true", "false") else int(a) for a in args.split(", ")), int(grid)


def plan_pnt(D, U, mode, rows):
    return plan(D, U, mode, rows)[1][-1]


# ---------------------------------------------------------------- 40 rows of a big table
def spread_rows(U, row_bytes, n):
    """n distinct ascending rows of a U-row table: row 0, row U - 1, the rows either side of the byte offsets 2^28 (where
    the 256 MB rule turns) and 2^31 (where a 32-bit byte offset would wrap) as far as the table has them, the rest spread
    evenly"""
    assert U >= n
    rows = {0, U - 1}
    for off in (1 << 28, 1 << 31):
        k = off // row_bytes                               # the row that holds byte `off`
        rows |= {x for x in (k - 1, k, k + 1) if 0 <= x < U}
    assert len(rows) <= n
    rs = np.random.RandomState(U % (2 ** 31) + n)
    have = set(rows)
    for x in np.linspace(0, U - 1, n + 2)[1:-1].astype(np.int64).tolist():
        if len(have) < n:
            have.add(int(x))
    while len(have) < n:                                   # the even spread hit a listed row
        have.add(int(rs.randint(0, U)))
    return np.array(sorted(have), np.int64)


def embed(t, u, U, row_bytes, spread_over=None):
    """(tables of a U-row model, user ids, the rows): the case's user rows and biases at spread_rows of the table (or of
    its first spread_over rows), zeros elsewhere"""
    n, D = t["P"].shape
    pos = spread_rows(U if spread_over is None else spread_over, row_bytes, n)
    P = np.zeros((U, D), np.float32)
    P[pos] = t["P"]
    bu = np.zeros(U, np.float32)
    bu[pos] = t["bu"]
    return dict(t, P=P, bu=bu), pos[np.asarray(u)].astype(np.int32), pos


def plant_canaries(big, pos):
    """NaN in every row that follows a filled row and is not one itself.  No rating reads such a row; a load that runs
    past the end of a filled row does, and NaN times the zero on the item side's lane is NaN."""
    U = big["P"].shape[0]
    nxt = np.setdiff1d(pos + 1, pos)
    nxt = nxt[nxt < U]
    big["P"][nxt] = np.float32(np.nan)
    return nxt


def extract(big, u_big):
    """the case back out of an embedded one: (tables of the rows that a rating reads or that are not all zero, user ids
    into them, the rows)"""
    pos = np.union1d(np.flatnonzero(big["P"].any(axis=1) | (big["bu"] != 0)), u_big)
    u = np.searchsorted(pos, u_big)
    return dict(big, P=big["P"][pos], bu=big["bu"][pos]), u.astype(np.int32), pos


def embedded_faults(big, u_big, i, r, item_abs):
    """exactness_faults of an embedded case.  A row that is all zero and that no rating reads is an integer, bf16-exact
    and in no sum, so the properties are those of the other rows, taken back out of the big table."""
    t, u, _ = extract(big, u_big)
    return BC.exactness_faults(t, u, i, r, item_abs)


def exact_big_case(D, item_abs, U, row_bytes):
    """bf16_cases.exact_case on a U-row table: (tables, u, i, r, logits float32, sse, n_equal, rows)"""
    t, u, i, r, want, sse, neq = BC.exact_reference(D, item_abs)
    big, ub, pos = embed(t, u, U, row_bytes)
    return big, ub, i, r, want, sse, neq, pos


# ---------------------------------------------------------------- the random case
# 40 x 30 rand_tables rows and B ratings, binary rates under the nll head.  As in bf16_cases.eval_case the seeds were
# picked on the CPU so that no oracle logit lies within 1e-4 of 0, where round(sigmoid(x)) may flip: n_equal and the nll
# head's sse are then exact counts (tests/test_forward_paths_host.py checks the property, on the round-tripped rows too).
RANDOM_SEED = 9108
RANDOM_I = 30


def random_case(D, loss, item_abs=False, B=None):
    """(compact tables, u, i, r): user ids index the 40 compact rows; embed() puts them on a big table"""
    n = BC.EXACT_TABLES[0]
    B = max(3 * per_block(D) + 5, 301) if B is None else B
    rs = np.random.RandomState(RANDOM_SEED + 2 * D + int(item_abs))
    t = rand_tables(rs, n, RANDOM_I, D)
    u, i = rs.randint(0, n, B).astype(np.int32), rs.randint(0, RANDOM_I, B).astype(np.int32)
    r = (rs.rand(B) < 0.5).astype(np.float32) if loss == "nll" else rs.randint(1, 6, B).astype(np.float32)
    return t, u, i, r


def nll_sum(x, r):
    x = np.asarray(x, np.float64)
    return float(np.sum(np.maximum(x, 0) - x * r + np.log1p(np.exp(-np.abs(x)))))


# the grid-stride cases: one VEC = 1 and one VEC = 4 width, both at partial width and with few ratings per block
GRID_STRIDE = (61, 100)
