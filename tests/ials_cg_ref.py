"""The conjugate-gradient half-sweep of the implicit ALS restated (csrc/ials_cg.hip; include/tfrecomm.h states the solver).

Per entity with list N, w = alpha r, c = 1 + w, G = Y^T Y and the row x0 as it stands:

    x = x0;  r = sum_N (c - w (y.x)) y - (G x + lam x);  p = r;  rs = r.r;  stop = 2^-104 rs
    at most `steps` times, while rs > stop:
        Ap = G p + lam p + sum_N w (y.p) y;  a = rs / (p.Ap);  x += a p;  r -= a Ap;  rn = r.r;  p = r + (rn / rs) p;  rs = rn

    cg_half        that in np.longdouble, every entity in step (a dict like ials_ref.half's: x, cond, xmax, N, and `used`)
    cg_half_f64    float64 in the kernels' order: wave w takes the list entries and the rows of G with index = w mod 4, a
                   lane the components l + 64 j, a dot is the lane's products (j ascending) then the butterfly, the four
                   waves' vectors are added in wave order
    gram_f64       ials_ref.gram_f64 itself: both solvers share one Gram (k_ials_gram_tiled + k_ials_gram_sum)
    loss_f64       k_ials_loss_users_wide + k_ials_loss_reduce

Bounds (eps = 2^-52; cond2(A) of A = G + sum_N w y y^T + lam I), per entity and for the loss:

    same steps    |x - x_ref|_inf <= K_CG eps cond2(A) max(|x0|_inf, |x_ref|_inf)     x_ref = cg_half at the SAME steps in {1, 2, 3}
    converged     |x - x*|_inf    <= K_CONV eps cond2(A) max(|x0|_inf, |x*|_inf)      steps = 3 d, d <= 33, x* = ials_ref.half
    loss          |L - L_ref|     <= K_LOSS_WIDE eps sum|term|                        sum|term| = ials_ref.loss_terms

x0 belongs in the unit because the iterate is x0 plus corrections built from it.  Iterates at MORE steps are not compared:
once a Ritz value has converged the float64 and the longdouble recurrences legitimately part.

MEASURED on the CPU (tests/test_ials_cg_ref_host.py: cg_half_f64 and loss_f64 against the longdouble references, both halves
from the case's own tables, over every case of tests/ials_cg_cases.CASES at 1, 2 and 3 steps, CONV_CASES at 3 d steps and the
LOSS_IDS): the figures and the cases that gave them stand below.  The N(0, 0.1) tables, whose sums cancel, set all but the loss's.  Each K is ceil(8 * its figure): the margin of 8 and its reasoning are those of K = 106 in
tests/als_step_ref.py.  The host test asserts that the restatement stays within K / 8 and that the figures are the ones it
measures.
"""
import numpy as np

from tests.als_step_ref import EPS, LD
from tests import ials_ref as R

WAVES, LANES, MAXD, THREADS = 4, 64, 256, 256
STOP = 2.0 ** -104

MEASURED_RHO_CG = 75.513          # cg-long-d1-normal, item half, 1 step: cond = 1, the rounding of 1100-term sums
MEASURED_RHO_CONV = 15.639        # cg-conv-d1-swapped-normal, user half
MEASURED_RHO_LOSS_WIDE = 1.096    # cg-widths-d256-swapped, tables as set
K_CG = 605                        # ceil(8 * 75.513)
K_CONV = 126                      # ceil(8 * 15.639)
K_LOSS_WIDE = 9                   # ceil(8 * 1.096)


def lane_components(d):
    """components per lane of cg_pass<NC>"""
    return -(-d // LANES)


gram_tiles, gram_f64 = R.gram_tiles, R.gram_f64              # the Gram is not restated here


# ----------------------------------------------------------------------------- longdouble reference
def conds(other, lst, lam, alpha, G):
    """cond2(A) per entity, A = G + sum_N w y y^T + lam I, in float64 (1 for an empty list's entry is never used)"""
    ptr, ids, vals, _ = lst
    d = other.shape[1]
    G = np.asarray(G, np.float64).reshape(d, d)
    out = np.ones(ptr.size - 1)
    for e in np.flatnonzero(np.diff(ptr)):
        y = other[ids[ptr[e]:ptr[e + 1]]]
        ev = np.linalg.eigvalsh(G + (y * (alpha * vals[ptr[e]:ptr[e + 1]])[:, None]).T @ y + lam * np.eye(d))
        out[e] = ev[-1] / ev[0]
    return out


def cg_half(own, other, lst, lam, alpha, steps, G=None, early_exit=True, cond=None):
    """The reference.  ``own``: the rows as they stand (the warm start); ``G`` defaults to the longdouble Gram of ``other``.
    Returns x [n, d] (longdouble, exactly 0 for an empty list), cond (``conds`` of these arguments unless given), xmax =
    max(|x0|_inf, |x|_inf), N and used (steps taken)."""
    ptr, ids, vals, _ = lst
    n, d = ptr.size - 1, other.shape[1]
    G = R.gram(other) if G is None else np.asarray(G).astype(LD).reshape(d, d)
    N = np.diff(ptr)
    full = np.flatnonzero(N)
    out = np.zeros((n, d), LD)
    used = np.zeros(n, np.int64)
    if full.size:
        starts = ptr[full].astype(np.int64)                 # the pairs of the non-empty entities are contiguous
        rowpos = np.repeat(np.arange(full.size), N[full])
        Yi = other[ids].astype(LD)
        w = LD(alpha) * vals.astype(LD)
        c, lamL = 1 + w, LD(lam)
        lsum = lambda coef: np.add.reduceat(coef[:, None] * Yi, starts, axis=0)
        sdot = lambda v: (Yi * v[rowpos]).sum(1)
        x = own[full].astype(LD)
        r = lsum(c - w * sdot(x)) - (x @ G + lamL * x)
        p = r.copy()
        rs = (r * r).sum(1)
        stop = LD(STOP) * rs if early_exit else np.full(rs.shape, -1, LD)
        for _ in range(steps):
            act = rs > stop
            if not act.any():
                break
            Ap = p @ G + lamL * p + lsum(w * sdot(p))
            with np.errstate(divide="ignore", invalid="ignore"):
                a = rs / (p * Ap).sum(1)
                xn, rn_v = x + a[:, None] * p, r - a[:, None] * Ap
                rn = (rn_v * rn_v).sum(1)
                pn = rn_v + (rn / rs)[:, None] * p
            m = act[:, None]
            x, r, p, rs = np.where(m, xn, x), np.where(m, rn_v, r), np.where(m, pn, p), np.where(act, rn, rs)
            used[full] += act
        out[full] = x
    x0 = np.abs(np.asarray(own, np.float64)).max(1)
    return dict(x=out, cond=conds(other, lst, lam, alpha, G.astype(np.float64)) if cond is None else cond, N=N, used=used,
                xmax=np.maximum(np.where(N > 0, x0, 0.0), np.abs(out).max(1).astype(np.float64)))


def against_exact(own, exact):
    """ials_ref.half's result with x0 in the unit: the reference of the converged statement"""
    x0 = np.abs(np.asarray(own, np.float64)).max(1)
    return dict(exact, xmax=np.maximum(np.where(exact["N"] > 0, x0, 0.0), exact["xmax"]))


# ----------------------------------------------------------------------------- float64 in the kernels' order
def _fold(s):
    """the butterfly xor 32, 16, .. 1 over the last axis of 64: what every lane ends with"""
    o = LANES // 2
    while o >= 1:
        s = s[..., :o] + s[..., o:2 * o]
        o //= 2
    return s[..., 0]


def _pad(a, width):
    out = np.zeros(a.shape[:-1] + (width,))
    out[..., :a.shape[-1]] = a
    return out


def _wave_dot(Y, v):
    """y_k . v per row of Y: lane l sums its components l + 64 j, j ascending, then the butterfly"""
    nc = lane_components(Y.shape[1])
    Yp, vp = _pad(Y, nc * LANES), _pad(v, nc * LANES)
    s = np.zeros((Y.shape[0], LANES))
    for j in range(nc):
        s = s + Yp[:, j * LANES:(j + 1) * LANES] * vp[j * LANES:(j + 1) * LANES]
    return _fold(s)


def _block_dot(a, b):
    """thread c's product, a butterfly per wave, the waves' sums in wave order"""
    wsum = _fold(_pad(a * b, THREADS).reshape(WAVES, LANES))
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]


def _by_wave(rows, fault=None):
    """the four waves' sums of rows k = w, w + 4, ... (each in that order), added in wave order"""
    part = [R._seq(np.zeros(rows.shape[1]), rows[w::WAVES]) for w in range(WAVES)]
    if fault == "drop_last_wave":
        part[WAVES - 1] = np.zeros(rows.shape[1])
    return ((part[0] + part[1]) + part[2]) + part[3]


def cg_half_f64(own, other, lst, lam, alpha, steps, G=None, fault=None):
    """x [n, d] in float64 in the order of k_ials_gram_tiled / k_ials_cg_fit.  ``fault`` plants one error: no_ridge_in_Ap
    (lam p dropped from Ap), c_for_w (c used for w in Ap), no_beta ((rn / rs) forced to 0: seen from step 2), cold_start
    (x0 = 0), drop_last_wave (the entries k = 3 mod 4 of every list dropped), drop_last_tile (of the Gram)."""
    ptr, ids, vals, _ = lst
    n, d = ptr.size - 1, other.shape[1]
    G = gram_f64(other, fault) if G is None else np.asarray(G, np.float64).reshape(d, d)
    out = np.zeros((n, d))
    for e in range(n):
        lo, hi = int(ptr[e]), int(ptr[e + 1])
        if lo == hi:
            continue
        Y, w = other[ids[lo:hi]], alpha * vals[lo:hi]
        x = np.zeros(d) if fault == "cold_start" else np.array(own[e], np.float64)

        def passes(v, first):
            s = _wave_dot(Y, v)
            coef = ((1.0 + w) - w * s) if first else ((1.0 + w) * s if fault == "c_for_w" else w * s)
            return _by_wave(coef[:, None] * Y, fault), _by_wave(G * v[:, None])

        ls, gs = passes(x, True)
        r = ls - (gs + lam * x)
        p = r.copy()
        rs = _block_dot(r, r)
        stop = STOP * rs
        for _ in range(steps):
            if not rs > stop:
                break
            ls, gs = passes(p, False)
            Ap = (gs + (0.0 if fault == "no_ridge_in_Ap" else lam * p)) + ls
            with np.errstate(divide="ignore", invalid="ignore"):
                a = rs / _block_dot(p, Ap)
                x = x + a * p
                r = r - a * Ap
                rn = _block_dot(r, r)
                p = r + (0.0 if fault == "no_beta" else rn / rs) * p
            rs = rn
        out[e] = x
    return out


def sweep_f64(case, X, Y, steps, n=1):
    """n x (user half, item half) of the float64 restatement"""
    X, Y = np.array(X), np.array(Y)
    lu, li = R.lists(case, 0), R.lists(case, 1)
    for _ in range(n):
        X = cg_half_f64(X, Y, lu, case["lam"], case["alpha"], steps)
        Y = cg_half_f64(Y, X, li, case["lam"], case["alpha"], steps)
    return X, Y


def loss_f64(X, Y, case):
    """k_ials_loss_users_wide: thread c < d holds x_c ((G x)_c + lam x_c), (G x)_c summed over the rows of G ascending; lane
    0 of wave w adds the terms of the entries w, w + 4, ... after its own head term; the halving tree; then
    k_ials_loss_reduce as ials_ref.loss_f64 restates it"""
    ptr, ids, vals = case["indptr"], case["items"], case["vals"]
    d, lam = X.shape[1], case["lam"]
    G = gram_f64(Y)
    per = np.zeros(case["nu"])
    for u in range(case["nu"]):
        x = X[u]
        gx = R._seq(np.zeros(d), G * x[:, None])
        lanes = _pad(x * (gx + lam * x), THREADS)
        y = Y[ids[ptr[u]:ptr[u + 1]]]
        s = _wave_dot(y, x)
        cc = 1.0 + case["alpha"] * vals[ptr[u]:ptr[u + 1]]
        term = cc * ((1.0 - s) * (1.0 - s)) - s * s
        for w in range(WAVES):
            lanes[w * LANES] = R._seq(np.array(lanes[w * LANES]), term[w::WAVES])
        per[u] = R._tree(lanes)
    tr = 0.0
    for c in range(d):
        tr = tr + G[c, c]
    return R._tree(per) + lam * tr
