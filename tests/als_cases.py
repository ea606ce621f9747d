"""Constructed rating sets for the per-entity ALS checks (tests/test_als_step_ref_host.py, tests/test_gpu_als_step.py).

A case is a dict: id, d, lam, bias, ch (the value of TFR_ALS_CHUNK around the load, or None), nu, nw, the rating columns
u, w, y and the tables U, V, Wu, Ww that ``load_state`` sets.  Everything is drawn from a seeded RandomState; the bias is
set explicitly and is NOT mean(y) (ratings are 2.5 .. 5, mean 3.75), so that it visibly enters both b and w.  Tables are
uniform in [0, 1) like the reference's init_vars and ratings positive, so that b does not cancel (tests/als_step_ref.py).
``swapped(case)`` is the same case with the two id columns (and the two sides' tables) exchanged: every edge then lands on
k_als_fit once as the user half and once as the work half.  CASES holds both orientations of every case.

lambda = 0 with N < d makes A singular; that is outside the contract of the kernel (and of the reference class, whose
solve would fail) and no case has it.
"""
import numpy as np

from tests import widths as W

BIAS = 1.375
TILE_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1024, 1025)


def _ratings(rs, n):
    return rs.randint(5, 11, n) / 2.0                      # 2.5 .. 5.0, never 0


def _finish(cid, d, lam, ch, nu, nw, u, w, y, rs, shuffle=True):
    u, w, y = (np.concatenate(a) if isinstance(a, list) else a for a in (u, w, y))
    if shuffle:                                            # lists in insertion order: mix the entities' ratings
        p = rs.permutation(u.size)
        u, w, y = u[p], w[p], y[p]
    return dict(id=cid, d=d, lam=lam, bias=BIAS, ch=ch, nu=nu, nw=nw,
                u=np.ascontiguousarray(u, np.int64), w=np.ascontiguousarray(w, np.int64), y=np.ascontiguousarray(y, np.float64),
                U=rs.uniform(0.0, 1.0, (nu, d)), V=rs.uniform(0.0, 1.0, (nw, d)),
                Wu=rs.uniform(0.0, 0.5, nu), Ww=rs.uniform(0.0, 0.5, nw))


def _users_of_lengths(rs, lengths, nw):
    """user k rates lengths[k] distinct works"""
    u = [np.full(n, k, np.int64) for k, n in enumerate(lengths)]
    w = [rs.choice(nw, n, replace=False) for n in lengths]
    return u, w


def swapped(c):
    return dict(c, id=c["id"] + "-swapped", nu=c["nw"], nw=c["nu"], u=c["w"], w=c["u"], U=c["V"], V=c["U"], Wu=c["Ww"], Ww=c["Wu"])


def tile_edges(d):
    """one user per list length at every tile and chunk edge over 1100 works; user 13 rates work 7 twice; users 14 and 15
    have no ratings"""
    rs = np.random.RandomState(1000 + d)
    nw = 1100
    u, w = _users_of_lengths(rs, TILE_LENGTHS, nw)
    k = len(TILE_LENGTHS)
    u.append(np.full(5, k, np.int64))
    w.append(np.array([3, 7, 500, 7, 1099]))
    n = sum(a.size for a in u)
    return _finish("tile_edges-d%d" % d, d, 0.1, None, k + 3, nw, u, w, _ratings(rs, n), rs)


def chunk_edges(ch, d, env=True):
    """users 0..4 at the chunk edges, users 5..7 short, and ch + 9 further users who all rate work 0, which is then the one
    chunked work: many chunks on the user side, two on the work side (the reverse once swapped).  env=False: the same
    ratings and tables loaded without TFR_ALS_CHUNK, where nothing is chunked."""
    rs = np.random.RandomState(2000 + 100 * ch + d)
    nw = 3 * ch + 20
    lengths = (ch, ch + 1, 2 * ch, 2 * ch + 1, 3 * ch - 1, 1, 5, 31)
    u, w = _users_of_lengths(rs, lengths, nw)
    k = len(lengths)
    for f in range(ch + 9):
        extra = 1 + rs.choice(nw - 1, 3, replace=False)
        u.append(np.full(4, k + f, np.int64))
        w.append(np.concatenate(([0], extra)))
    n = sum(a.size for a in u)
    c = _finish("chunk_edges-ch%d-d%d" % (ch, d), d, 0.1, ch, k + ch + 9, nw, u, w, _ratings(rs, n), rs)
    return c if env else dict(c, id=c["id"] + "-unchunked", ch=None)


def sweep_sets():
    """user 0: all ratings 0.0 (never fitted, its partners still read its row); user 1: one 0.0 and one non-zero rating
    (fitted, N = 2); user 2 and work 9: no ratings; work 8: rated only by user 0 (never fitted); users 3..7 ordinary"""
    rs = np.random.RandomState(3000)
    nu, nw = 8, 10
    u = [np.array([0, 0, 0]), np.array([1, 1])]
    w = [np.array([8, 1, 2]), np.array([1, 3])]
    y = [np.zeros(3), np.array([0.0, 3.5])]
    for k in range(3, 8):
        ws = rs.choice(8, 4, replace=False)
        u.append(np.full(4, k)); w.append(ws); y.append(_ratings(rs, 4))
    return _finish("sweep_sets", 5, 0.1, None, nu, nw, u, w, y, rs)


def conditioning(lam):
    """d = 32 with N = 1, 5 and 31 (the Gram matrix is rank-deficient: only the ridge makes A SPD) and N = 40"""
    rs = np.random.RandomState(4000)
    nw = 60
    u, w = _users_of_lengths(rs, (1, 5, 31, 40), nw)
    n = sum(a.size for a in u)
    return _finish("conditioning-lam%g" % lam, 32, lam, None, 4, nw, u, w, _ratings(rs, n), rs)


def grid_stride(nu=70000, nw=300, n=2200000):
    """d = 2, TFR_ALS_CHUNK = 32: more than 65 535 fitted users (k_als_fit's stride loop) and more than 65 535 chunks on the
    work side (k_als_partial's).  Smaller arguments give the same shape of case for the CPU."""
    rs = np.random.RandomState(5000)
    u = np.concatenate((np.arange(nu), rs.randint(0, nu, n - nu)))
    w = rs.randint(0, nw, n)
    c = _finish("grid_stride", 2, 0.1, 32, nu, nw, u, w, _ratings(rs, n), rs)
    return c if nu == 70000 else dict(c, id="grid_stride-reduced")


CHUNK_CASES = [(ch, d) for ch in (32, 64) for d in (9, 32)]
LAMBDAS = (0.1, 1e-3, 1e-6)


def small_cases():
    """every case but grid_stride, as given"""
    out = [tile_edges(d) for d in W.ALS_STEP]
    for ch, d in CHUNK_CASES:
        out += [chunk_edges(ch, d), chunk_edges(ch, d, env=False)]
    return out + [sweep_sets()] + [conditioning(lam) for lam in LAMBDAS]


def both(cases):
    return [c for case in cases for c in (case, swapped(case))]


CASES = both(small_cases())
