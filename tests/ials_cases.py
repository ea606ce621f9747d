"""Constructed implicit-feedback data for the per-entity iALS checks (tests/test_ials_ref_host.py, tests/test_gpu_ials.py).

A case is a dict: id, d, lam, alpha, chunk, nu, ni, the user x item CSR (indptr int64, items int32, vals float64: rows
strictly increasing, values positive) and the tables X [nu, d], Y [ni, d] that ``set_factors`` sets.  Everything comes from a
seeded RandomState.  Tables are uniform in [0, 1) so that b = sum c y does not cancel (the reasoning of
tests/als_step_ref.py: eps cond |x| bounds the solve, not the rounding of a cancelling right-hand side).
``swapped(case)`` is the transposed data with the two tables exchanged: every list length then lands on k_ials_fit once as
the user half and once as the item half.  CASES holds both orientations of every small case.
"""
import numpy as np

# both ends of every count of live A-entry slots ceil(d * d / 256), 1 .. 16 (csrc/ials.hip ials_accumulate), and d = 63
WIDTHS = (1, 16, 17, 22, 23, 27, 28, 32, 33, 35, 36, 39, 40, 42, 43, 45, 46, 48, 49, 50, 51, 53, 54, 55, 56, 57, 58, 59, 60,
          61, 62, 63, 64)
TILE_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65)
LONG_LENGTHS = (511, 512, 513, 1024, 1025)                 # around one and two chunks of the default 512
LONG_WIDTHS = (1, 9, 33, 64)
CHUNK_CASES = [(ch, d) for ch in (32, 64) for d in (9, 33)]
LAMBDAS = (0.1, 1e-3, 1e-6)
ALPHAS = (1.0, 40.0)
GRAM_NS = (1, 127, 128, 129, 5 * 128 + 3, 131073)          # slice edges at 128 rows; 131073 rows take slices of 160


def _values(rs, n):
    return rs.randint(1, 9, n) / 2.0                       # 0.5 .. 4.0


def _case(cid, d, lam, alpha, chunk, nu, ni, rows, rs):
    """rows: per user, an array of distinct item ids (any order)"""
    rows = [np.sort(np.asarray(r, np.int64)) for r in rows] + [np.zeros(0, np.int64)] * (nu - len(rows))
    indptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    items = np.concatenate(rows).astype(np.int32)
    return dict(id=cid, d=d, lam=lam, alpha=alpha, chunk=chunk, nu=nu, ni=ni, indptr=indptr, items=items,
                vals=np.ascontiguousarray(_values(rs, items.size), np.float64),
                X=rs.uniform(0.0, 1.0, (nu, d)), Y=rs.uniform(0.0, 1.0, (ni, d)))


def csr(case):
    import scipy.sparse as sp
    return sp.csr_matrix((case["vals"], case["items"], case["indptr"]), shape=(case["nu"], case["ni"]))


def swapped(c):
    t = csr(c).T.tocsr()
    t.sort_indices()
    return dict(c, id=c["id"] + "-swapped", nu=c["ni"], ni=c["nu"], indptr=t.indptr.astype(np.int64), items=t.indices.astype(np.int32),
                vals=np.ascontiguousarray(t.data, np.float64), X=c["Y"], Y=c["X"])


def _of_lengths(rs, lengths, ni):
    return [rs.choice(ni, n, replace=False) for n in lengths]


def widths_case(d):
    """one user per list length at every tile edge over 80 items; two further users without pairs"""
    rs = np.random.RandomState(1000 + d)
    return _case("widths-d%d" % d, d, 0.1, 40.0, 512, len(TILE_LENGTHS) + 2, 80, _of_lengths(rs, TILE_LENGTHS, 80), rs)


def long_case(d):
    """lists around one and two chunks of the default size, a short one and an empty one"""
    rs = np.random.RandomState(1500 + d)
    lengths = LONG_LENGTHS + (40, 0)
    return _case("long-d%d" % d, d, 0.1, 40.0, 512, len(lengths), 1100, _of_lengths(rs, lengths, 1100), rs)


def chunk_case(ch, d, chunk=None):
    """users around one, two and three chunks of ch, three short ones, and ch + 9 further users who all hold item 0, which is
    then the one chunked item (two chunks).  ``chunk``: the same data loaded at another chunk size."""
    rs = np.random.RandomState(2000 + 100 * ch + d)
    ni = 3 * ch + 20
    lengths = (ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch, 2 * ch + 1, 3 * ch - 1, 3 * ch, 3 * ch + 1, 1, 5, 31)
    rows = _of_lengths(rs, lengths, ni)
    for _ in range(ch + 9):
        rows.append(np.concatenate(([0], 1 + rs.choice(ni - 1, 3, replace=False))))
    c = _case("chunk%d-d%d" % (ch, d), d, 0.1, 40.0, ch, len(rows), ni, rows, rs)
    return c if chunk is None else dict(c, id=c["id"] + "-at%d" % chunk, chunk=chunk)


def conditioning(lam, alpha):
    """d = 64 with 1, 5 and 40 pairs (fewer than components: only G and the ridge make A definite) and 70 pairs"""
    rs = np.random.RandomState(4000)
    return _case("conditioning-lam%g-alpha%g" % (lam, alpha), 64, lam, alpha, 512, 5, 90, _of_lengths(rs, (1, 5, 40, 70, 0), 90), rs)


def trajectory():
    """ten iterations at d = 8, lambda = 0.1, alpha = 40 from the library's own initialisation"""
    rs = np.random.RandomState(6000)
    nu, ni = 60, 40
    c = _case("trajectory", 8, 0.1, 40.0, 512, nu, ni, _of_lengths(rs, rs.randint(3, 14, nu), ni), rs)
    init = np.random.RandomState(0)                        # ImplicitALS.init_factors(seed=0, stddev=0.01)
    return dict(c, X=init.normal(0.0, 0.01, (nu, 8)), Y=init.normal(0.0, 0.01, (ni, 8)))


def grid_entities(nu=70000, ni=300):
    """d = 5: more entities than the 65 535-block grid cap (k_ials_fit's stride loop; every tenth user empty), against a
    partner table of 300 rows; the items' lists are long and chunked at the default size"""
    rs = np.random.RandomState(5000)
    rows = [rs.choice(ni, 3, replace=False) if u % 10 else np.zeros(0, np.int64) for u in range(nu)]
    return _case("grid_entities", 5, 0.1, 40.0, 512, nu, ni, rows, rs)


def grid_chunks(nu=33000, ni=300):
    """d = 9, chunk = 32: every user holds 33 .. 40 items, two chunks each: more than 65 535 chunks (k_ials_partial's stride
    loop), the last of them one to eight entries long"""
    rs = np.random.RandomState(5001)
    rows = [rs.choice(ni, 33 + u % 8, replace=False) for u in range(nu)]
    return _case("grid_chunks", 9, 0.1, 40.0, 32, nu, ni, rows, rs)


def small_cases():
    out = [widths_case(d) for d in WIDTHS] + [long_case(d) for d in LONG_WIDTHS]
    out += [chunk_case(ch, d) for ch, d in CHUNK_CASES]
    return out + [conditioning(lam, alpha) for lam in LAMBDAS for alpha in ALPHAS]


def both(cases):
    return [c for case in cases for c in (case, swapped(case))]


CASES = both(small_cases())
# the cases small enough for the definition itself (dense_half, loss_dense) and for five iterations on the CPU
DENSE_IDS = tuple(c["id"] for c in CASES if c["id"].startswith(("chunk", "conditioning"))
                  or c["id"].split("-swapped")[0] in ("widths-d1", "widths-d33", "widths-d63", "widths-d64", "long-d9"))
