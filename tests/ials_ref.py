"""Implicit-feedback ALS restated (csrc/ials.hip; the model is defined in include/tfrecomm.h).

A case (tests/ials_cases.py) holds the user x item CSR (indptr, items, vals), d, lam, alpha, chunk and the tables X, Y.
``lists(case, side)`` gives (ptr, ids, vals, n_other) of side 0 (the CSR as given) or side 1 (its transpose, users ascending).

    dense_half   the definition: per entity the full confidence vector over ALL partners,
                 (Y^T diag(c) Y + lambda I) x = Y^T diag(c) p, in np.longdouble
    half         the decomposed form, A = G + sum_N w y y^T + lambda I, b = sum_N c y, in longdouble; takes a given G
    gram_f64     the one Gram of both solvers (k_ials_gram_tiled + k_ials_gram_sum), float64 in the kernels' order
    half_f64     float64 in the kernels' order: Gram slices, 32-row tiles, chunks, (w y_r) y_c, (G + acc) + lambda
    loss_dense / loss / loss_f64   the loss by its definition, by the formula that never forms the dense matrix, and that
                 formula in float64 in the kernels' order

Bounds (eps = 2^-52), per entity and for the loss:

    |x - x_ref|_inf <= K eps cond2(A) |x_ref|_inf
    |L - L_ref|     <= K_LOSS eps sum|term|,   sum|term| = sum_u [|x_u|^T (|Y|^T |Y|) |x_u| + sum_N (c (1 - s)^2 + s^2)]
                                                            + lambda (|X|^2 + |Y|^2)

MEASURED on the CPU (tests/test_ials_ref_host.py: half_f64 and loss_f64 against the longdouble references over every case of
tests/ials_cases.CASES, half by half, two iterations of the dense ones): max rho_x = 8.357 (long-d1-swapped, item half:
d = 1 has cond = 1, so the bound is eps |x| and the error is the rounding of an 1100-term sum), max rho_loss = 0.544
(widths-d1).  K = ceil(8 * 8.357) = 67 and K_LOSS = ceil(8 * 0.544) = 5: the margin of 8 and its reasoning are those of
K = 106 in tests/als_step_ref.py.  The host test asserts that the restatement stays within K / 8 and K_LOSS / 8 and that
these figures are the ones it measures.
"""
import numpy as np

from tests.als_step_ref import EPS, LD, chol_solve

TILE, CHUNK, THREADS = 32, 512, 256
GRAM_TILE = 64                                             # csrc/ials.hip GRAM_T: the edge of a block's output tile
GRAM_NARROW = 23                                           # csrc/ials.hip GRAM_NARROW_D: up to here one block keeps a whole slice
GRAM_ROWS, GRAM_SLICES = 128, 1024                         # csrc/ials.hip IALS_GRAM_ROWS, IALS_GRAM_SLICES
MAXD = 64
MEASURED_RHO_X, MEASURED_RHO_LOSS = 8.357, 0.544
K = 67
K_LOSS = 5


def gram_slice_rows(n):
    """rows per Gram slice (csrc/ials.hip gram_slice_rows): a function of n alone"""
    per = -(-n // GRAM_SLICES)
    return max(GRAM_ROWS, -(-per // TILE) * TILE)


def lists(case, side):
    """(ptr, ids, vals, n_other) of the side's entities; side 1 is the transpose with users ascending in each list"""
    ptr, items, vals = case["indptr"], case["items"], case["vals"]
    if side == 0:
        return ptr, items, vals, case["ni"]
    rows = np.repeat(np.arange(case["nu"]), np.diff(ptr))
    order = np.argsort(items, kind="stable")
    tptr = np.searchsorted(items[order], np.arange(case["ni"] + 1)).astype(np.int64)
    return tptr, rows[order].astype(np.int32), vals[order], case["nu"]


def n_chunks(ptr, ch):
    N = np.diff(ptr)
    return np.where(N > ch, -(-N // ch), 0)


# ----------------------------------------------------------------------------- longdouble references
def gram(T):
    T = T.astype(LD)
    return (T[:, :, None] * T[:, None, :]).sum(0) if T.shape[0] * T.shape[1] ** 2 <= 1 << 24 else _gram_blocked(T)


def _gram_blocked(T):
    d = T.shape[1]
    G = np.zeros((d, d), LD)
    step = max(1, (1 << 22) // (d * d))
    for s in range(0, T.shape[0], step):
        t = T[s:s + step]
        G += (t[:, :, None] * t[:, None, :]).sum(0)
    return G


def gram_bound(T):
    """(n + 2) eps (|T|^T |T|)_rc: the bound of a sum of n rounded products in any order, FMA allowed"""
    a = np.abs(T)
    return (T.shape[0] + 2) * EPS * (a.T @ a)


def _finish(x, A, N):
    d = x.shape[1]
    ev = np.linalg.eigvalsh(A.astype(np.float64)) if len(A) else np.zeros((0, d))
    return dict(x=x, cond=ev[:, -1] / ev[:, 0], xmax=np.abs(x).max(1).astype(np.float64), N=N)


def half(other, lst, lam, alpha, G=None, batch=1 << 18):
    """The reference, decomposed form.  Returns per-entity x [n, d] (longdouble; exactly 0 for an empty list), cond (cond2
    of A), xmax and N.  ``G`` defaults to the longdouble Gram of ``other``; a test feeds the device's own."""
    ptr, ids, vals, _ = lst
    n, d = ptr.size - 1, other.shape[1]
    G = gram(other) if G is None else np.asarray(G).astype(LD).reshape(d, d)
    N = np.diff(ptr)
    A = np.broadcast_to(G + LD(lam) * np.eye(d, dtype=LD), (n, d, d)).copy()
    b = np.zeros((n, d), LD)
    iu = np.triu_indices(d)
    full = np.flatnonzero(N)
    e0 = 0
    while e0 < full.size:                                   # batches of whole entities, about `batch` pairs each
        e1 = max(e0 + 1, int(np.searchsorted(ptr[full + 1], ptr[full[e0]] + batch, side="right")))
        ent = full[e0:e1]
        lo, hi = int(ptr[ent[0]]), int(ptr[ent[-1] + 1])
        start = (ptr[ent] - lo).astype(np.int64)            # entities of `full` are contiguous in the pair arrays between empties
        Yi = other[ids[lo:hi]].astype(LD)
        w = LD(alpha) * vals[lo:hi].astype(LD)
        tri = np.add.reduceat((w[:, None] * Yi[:, iu[0]]) * Yi[:, iu[1]], start, axis=0)
        A[ent[:, None], iu[0][None, :], iu[1][None, :]] += tri
        off = iu[0] != iu[1]
        A[ent[:, None], iu[1][off][None, :], iu[0][off][None, :]] += tri[:, off]
        b[ent] = np.add.reduceat((1 + w)[:, None] * Yi, start, axis=0)
        e0 = e1
    x = chol_solve(A, b)
    x[N == 0] = 0
    return _finish(x, A, N)


def dense_half(other, lst, lam, alpha):
    """The definition itself, entity by entity over all partners: small cases only"""
    ptr, ids, vals, n_other = lst
    n, d = ptr.size - 1, other.shape[1]
    Y = other.astype(LD)
    A, b = np.zeros((n, d, d), LD), np.zeros((n, d), LD)
    for e in range(n):
        c, p = np.ones(n_other, LD), np.zeros(n_other, LD)
        j = ids[ptr[e]:ptr[e + 1]]
        c[j] = 1 + LD(alpha) * vals[ptr[e]:ptr[e + 1]].astype(LD)
        p[j] = 1
        A[e] = (Y * c[:, None]).T @ Y + LD(lam) * np.eye(d, dtype=LD)
        b[e] = Y.T @ (c * p)
    return _finish(chol_solve(A, b), A, np.diff(ptr))


def ratios(ref, x):
    """per entity: the error of x in units of eps cond2(A) |x_ref|; 0 where both are 0"""
    ex = np.abs(np.asarray(x).astype(LD) - ref["x"]).max(1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ex == 0, 0.0, ex / (EPS * ref["cond"] * ref["xmax"]))


def check_half(ref, x, k, what=""):
    """[] or lines naming what is outside k times its bound (NaN counts as outside) or not exactly 0 for an empty list"""
    bad = []
    x = np.asarray(x)
    empty = ref["N"] == 0
    if empty.any() and not (x[empty] == 0).all():
        bad.append("%s: %d entities without pairs are not exactly 0" % (what, int((x[empty] != 0).any(1).sum())))
    rho = ratios(ref, x)
    out = ~(rho <= k) & ~empty
    if out.any():
        i = int(np.flatnonzero(out)[np.argmax(np.where(np.isnan(rho[out]), np.inf, rho[out]))])
        bad.append("%s: %d of %d entities outside the bound, worst entity %d: ratio %.3g > K = %g at d = %d, N = %d, cond = %.3g"
                   % (what, int(out.sum()), out.size, i, rho[i], k, x.shape[1], int(ref["N"][i]), ref["cond"][i]))
    return bad


def _pair_scores(X, Y, case):
    rows = np.repeat(np.arange(case["nu"]), np.diff(case["indptr"]))
    return rows, (X[rows].astype(LD) * Y[case["items"]].astype(LD)).sum(1)


def loss_dense(X, Y, case):
    """sum over ALL U x I pairs of c (p - x.y)^2 + lambda (|X|^2 + |Y|^2), longdouble: small cases only"""
    Xl, Yl = X.astype(LD), Y.astype(LD)
    S = Xl @ Yl.T
    Cm, P = np.ones(S.shape, LD), np.zeros(S.shape, LD)
    rows = np.repeat(np.arange(case["nu"]), np.diff(case["indptr"]))
    Cm[rows, case["items"]] = 1 + LD(case["alpha"]) * case["vals"].astype(LD)
    P[rows, case["items"]] = 1
    return (Cm * (P - S) ** 2).sum() + LD(case["lam"]) * ((Xl ** 2).sum() + (Yl ** 2).sum())


def loss(X, Y, case):
    """the same by the formula: sum_u [x^T G x + sum_N (c (1 - s)^2 - s^2)] + lambda (|X|^2 + |Y|^2), longdouble"""
    Xl, Yl = X.astype(LD), Y.astype(LD)
    G = gram(Y)
    _, s = _pair_scores(X, Y, case)
    c = 1 + LD(case["alpha"]) * case["vals"].astype(LD)
    return ((Xl @ G) * Xl).sum() + (c * (1 - s) ** 2 - s ** 2).sum() + LD(case["lam"]) * ((Xl ** 2).sum() + (Yl ** 2).sum())


def loss_terms(X, Y, case):
    """sum|term| of the loss bound, float64"""
    aX, aY = np.abs(X), np.abs(Y)
    _, s = _pair_scores(X, Y, case)
    s = s.astype(np.float64)
    c = 1 + case["alpha"] * case["vals"]
    return float(((aX @ (aY.T @ aY)) * aX).sum() + (c * (1 - s) ** 2 + s ** 2).sum() + case["lam"] * ((X ** 2).sum() + (Y ** 2).sum()))


# ----------------------------------------------------------------------------- float64 in the kernels' order
def _seq(acc, terms):
    """acc + terms[0] + terms[1] + ... one after the other"""
    return np.cumsum(np.concatenate((acc[None], terms)), axis=0)[-1]


def gram_tiles(d):
    """64-wide output tiles per side of k_ials_gram_tiled"""
    return -(-d // GRAM_TILE)


def gram_f64(T, fault=None):
    """k_ials_gram_tiled (k_ials_gram_narrow below 24 columns: the same order) + k_ials_gram_sum, any d <= 256: slices of
    gram_slice_rows(n) rows, row after row inside a slice, the slices' partials added in ascending order.  ``fault`` = drop_last_slice: the last of several slices is left out of
    the sum; drop_last_tile: the last 64 x 64 output tile is never written."""
    n, d = T.shape
    rows = gram_slice_rows(n)
    G = np.zeros((d, d))
    for lo in range(0, n, rows):
        if fault == "drop_last_slice" and lo + rows >= n and lo > 0:
            break
        t = T[lo:min(n, lo + rows)]
        G = G + _seq(np.zeros((d, d)), t[:, :, None] * t[:, None, :])
    if fault == "drop_last_tile":
        G[(gram_tiles(d) - 1) * GRAM_TILE:, (gram_tiles(d) - 1) * GRAM_TILE:] = 0.0
    return G


def _accumulate(rows, w, acc, accb, fault):
    for s in range(0, rows.shape[0], TILE):
        t, wk = rows[s:s + TILE], w[s:s + TILE]
        if fault == "drop_partial_tile" and t.shape[0] < TILE:
            break
        o = (wk[:, None] * t)[:, :, None] * t[:, None, :]
        if fault == "skip_slot15":
            o.reshape(t.shape[0], -1)[:, 15 * THREADS:] = 0.0
        acc = _seq(acc, o)
        accb = _seq(accb, (1.0 + wk)[:, None] * t)
    return acc, accb


def half_f64(other, lst, lam, alpha, ch=CHUNK, G=None, fault=None):
    """x [n, d] in float64 in the order of k_ials_gram_tiled / k_ials_partial / k_ials_fit.  ``fault`` plants one error:
    drop_partial_tile, skip_slot15 (A entries 3840.. never accumulated), drop_last_chunk, drop_last_slice, unit_confidence
    (b summed with c = 1), no_ridge."""
    ptr, ids, vals, _ = lst
    n, d = ptr.size - 1, other.shape[1]
    G = gram_f64(other, fault) if G is None else np.asarray(G, np.float64)
    A, B = np.zeros((n, d, d)), np.zeros((n, d))
    for e in range(n):
        lo, hi = int(ptr[e]), int(ptr[e + 1])
        rows, w = other[ids[lo:hi]], alpha * vals[lo:hi]
        acc, accb = np.zeros((d, d)), np.zeros(d)
        if hi - lo > ch:
            starts = list(range(0, hi - lo, ch))
            for s in starts[:-1] if fault == "drop_last_chunk" else starts:
                pa, pb = _accumulate(rows[s:s + ch], w[s:s + ch], np.zeros((d, d)), np.zeros(d), fault)
                acc, accb = acc + pa, accb + pb
        else:
            acc, accb = _accumulate(rows, w, acc, accb, fault)
        if fault == "unit_confidence":
            accb = rows.sum(0)
        A[e] = (G + acc) + np.eye(d) * (0.0 if fault == "no_ridge" else lam)
        B[e] = accb
    with np.errstate(invalid="ignore", divide="ignore"):
        x = chol_solve(A, B)
    x[np.diff(ptr) == 0] = 0.0
    return x


def _tree(v):
    """THREADS strided sums, then the halving tree (k_ials_loss_users, k_ials_loss_reduce)"""
    pad = np.zeros(-(-max(v.size, 1) // THREADS) * THREADS)
    pad[:v.size] = v
    red = _seq(np.zeros(THREADS), pad.reshape(-1, THREADS))
    o = THREADS // 2
    while o >= 1:
        red[:o] = red[:o] + red[o:2 * o]
        o //= 2
    return red[0]


def loss_f64(X, Y, case):
    ptr, ids, vals = case["indptr"], case["items"], case["vals"]
    d, lam = X.shape[1], case["lam"]
    G = gram_f64(Y)
    per = np.zeros(case["nu"])
    for u in range(case["nu"]):
        x = X[u]
        gx = np.zeros(d)
        for c in range(d):
            gx = gx + G[:, c] * x[c]
        head = x * (gx + lam * x)
        y = Y[ids[ptr[u]:ptr[u + 1]]]
        s = np.zeros(y.shape[0])
        for c in range(d):
            s = s + x[c] * y[:, c]
        cc = 1.0 + case["alpha"] * vals[ptr[u]:ptr[u + 1]]
        term = cc * ((1.0 - s) * (1.0 - s)) - s * s
        head256 = np.zeros(THREADS)                            # thread tid: its head entry first, then its list entries
        head256[:d] = head
        pad = np.zeros(-(-term.size // THREADS) * THREADS)
        pad[:term.size] = term
        lanes = _seq(head256, pad.reshape(-1, THREADS))
        per[u] = _tree(lanes)
    tr = 0.0
    for c in range(d):
        tr = tr + G[c, c]
    return _tree(per) + lam * tr


def sweep_f64(case, X, Y, n=1, fault=None):
    """n x (user half, item half) of the float64 restatement"""
    X, Y = np.array(X), np.array(Y)
    lu, li = lists(case, 0), lists(case, 1)
    for _ in range(n):
        X = half_f64(Y, lu, case["lam"], case["alpha"], case["chunk"], fault=fault)
        Y = half_f64(X, li, case["lam"], case["alpha"], case["chunk"], fault=fault)
    return X, Y
