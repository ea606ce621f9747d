"""One ALS half-sweep per entity, restated twice (csrc/als_kernels.hip, oracle/als_oracle.py ``_fit``).

    A = V[J]^T V[J] + lambda N I       b = (R - W_other[J] - (W_own[e] + bias)) . V[J]
    x = solve(A, b)                    w = mean(R - x . V[J]^T - W_other[J]) / (1 + lambda) - bias

``half_sweep`` is the reference: A, b, the Cholesky solve and the mean in ``np.longdouble`` (80-bit: eps 1.1e-19) from the
float64 inputs, every entity of the sweep set, vectorised.  ``half_sweep_f64`` is the same in float64 in the kernels' order:
32-rating tiles added in list order, per-chunk partial sums added in list order for lists longer than the chunk size, the
row-owned Cholesky with the two column-wise substitutions, 256 strided partial sums and a halving tree for w.  It runs on the
CPU only: it measures the tolerance constant below, takes the planted faults of tests/test_als_step_ref_host.py, and is a
second opinion when a GPU test fails.

The bounds, per entity (eps = 2^-52):

    |x - x_ref|_inf <= K eps cond2(A) |x_ref|_inf                                               = dx
    |w - w_ref|     <= (d dx max_k ||v_k||_1 + K eps (N + d) scale) / (1 + lambda)
    scale = mean_k(|r_k| + sum_c |x_c v_kc| + |w_other_k|) + |bias| (1 + lambda)

The first is the backward-error bound of a Cholesky solve with the constant left to measure.  The second propagates it: a
row off by dx moves each residual by at most dx ||v_k||_1 (the factor d is the issue's, slack); each residual is a d-term dot
and two subtractions, their mean an N-term sum, so rounding adds at most about (N + d) eps times the mean magnitude of the
terms; the bias is subtracted after the division, hence its factor (1 + lambda) inside ``scale``.

MEASURED on the CPU (tests/test_als_step_ref_host.py, every case of tests/als_cases.py, both orientations, both halves; the
float64 kernel-order restatement against the longdouble reference): max rho_x = 13.154 (tile_edges-d1, work half), max
rho_w = 0.337 (tile_edges-d1-swapped, user half); away from d = 1 no rho_x is above 6.5.  K = ceil(8 * 13.154) = 106.  The
host test asserts that the restatement stays within K / 8 and that these figures are the ones it measures.

eps cond |x| bounds the solve, not the rounding of b: where the terms of b cancel, x is small against them and rho_x grows
without the arithmetic being any worse (with tables and ratings of mixed sign it reached 2000 at d = 1, where cond = 1).  The
cases of tests/als_cases.py therefore draw tables and ratings like the reference's own (rand() tables, positive ratings);
the work half, whose b is built from fitted rows, is what sets the maximum.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the ALS reference needs an extended-precision long double"
EPS = float(np.finfo(np.float64).eps)
TILE, CHUNK, THREADS = 32, 512, 256                        # csrc/als_kernels.hip ALS_TILE, CH in tfr_als_load, the block
MEASURED_RHO_X, MEASURED_RHO_W = 13.154, 0.337
K = 106


def chunk_size(env=None):
    """CH as tfr_als_load reads it from TFR_ALS_CHUNK: values below a tile are ignored, others rounded down to tiles"""
    if env is not None and int(env) >= TILE:
        return int(env) // TILE * TILE
    return CHUNK


def build_lists(key, oth, y, rows):
    """per-entity lists in insertion order (duplicates of a pair kept) and the sweep set: entities with a non-zero rating"""
    key, oth, y = np.asarray(key, np.int64), np.asarray(oth, np.int64), np.asarray(y, np.float64)
    order = np.argsort(key, kind="stable")
    ptr = np.searchsorted(key[order], np.arange(rows + 1))
    nz = np.zeros(rows, bool)
    nz[key[y != 0]] = True
    return (ptr, oth[order], y[order]), np.flatnonzero(nz)


def sides(case):
    """((user lists, fitted users), (work lists, fitted works)) of a case of tests/als_cases.py"""
    return (build_lists(case["u"], case["w"], case["y"], case["nu"]), build_lists(case["w"], case["u"], case["y"], case["nw"]))


def check_untouched(what, own0, w0, own1, w1, entities):
    """[] or a line: the rows and W entries of entities outside the sweep set keep their bits"""
    rest = np.setdiff1d(np.arange(own0.shape[0]), entities)
    same = lambda a, b: a.shape == b.shape and a.tobytes() == b.tobytes()
    if same(own0[rest], own1[rest]) and same(w0[rest], w1[rest]):
        return []
    moved = [int(e) for e in rest if not (same(own0[e], own1[e]) and same(w0[e:e + 1], w1[e:e + 1]))]
    return ["%s: %d entities outside the sweep set changed, first %s" % (what, len(moved), moved[:5])]


def n_chunks(lists, ch=CHUNK):
    """chunks per entity: 0 up to ch ratings, ceil(N / ch) above"""
    N = np.diff(lists[0])
    return np.where(N > ch, -(-N // ch), 0)


def chol_solve(A, b):
    """x of A x = b for a stack of SPD matrices, in A's dtype and in the kernel's order: row r of L owned by one lane, column j
    of L from s = A[r][j] - sum_{k<j} L[r][k] L[j][k] (k ascending), then L y = b and L^T x = y column by column"""
    L, y = np.array(A), np.array(b)
    d = L.shape[-1]
    for j in range(d):
        s = L[..., j:, j].copy()
        for k in range(j):
            s -= L[..., j:, k] * L[..., j, k][..., None]
        piv = np.sqrt(s[..., 0])
        L[..., j, j] = piv
        L[..., j + 1:, j] = s[..., 1:] / piv[..., None]
    for i in range(d):
        y[..., i] = y[..., i] / L[..., i, i]
        y[..., i + 1:] -= L[..., i + 1:, i] * y[..., i][..., None]
    for i in range(d - 1, -1, -1):
        y[..., i] = y[..., i] / L[..., i, i]
        y[..., :i] -= L[..., i, :i] * y[..., i][..., None]
    return y


def _gather(lists, ent):
    ptr = lists[0]
    N = ptr[ent + 1] - ptr[ent]
    assert N.size == 0 or N.min() >= 1                     # an entity of the sweep set has a (non-zero) rating
    start = np.cumsum(N) - N
    pos = np.repeat(ptr[ent] - start, N) + np.arange(int(N.sum()))
    return N, start, pos, np.repeat(np.arange(ent.size), N)


def half_sweep(own, w_own, other, w_other, lists, entities, bias, lam):
    """The reference.  Returns a dict of per-entity arrays (in the order of ``entities``): x [n, d], w, cond (cond2 of A),
    xmax (max |x|), N, vmax (max_k ||v_k||_1) and scale (see the module docstring), x and w in longdouble."""
    ent = np.asarray(entities, np.int64)
    d = own.shape[1]
    if ent.size == 0:
        z = np.zeros(0)
        return dict(ent=ent, x=np.zeros((0, d), LD), w=np.zeros(0, LD), cond=z, xmax=z, N=np.zeros(0, np.int64), vmax=z, scale=z)
    N, start, pos, seg = _gather(lists, ent)
    J = lists[1][pos]
    Vi, Wi, R = other[J].astype(LD), w_other[J].astype(LD), lists[2][pos].astype(LD)
    b0 = w_own[ent].astype(LD) + LD(bias)
    A = np.add.reduceat(Vi[:, :, None] * Vi[:, None, :], start, axis=0)
    A += (LD(lam) * N.astype(LD))[:, None, None] * np.eye(d, dtype=LD)
    b = np.add.reduceat((R - Wi - b0[seg])[:, None] * Vi, start, axis=0)
    x = chol_solve(A, b)
    dots = (x[seg] * Vi).sum(1)
    w = np.add.reduceat(R - dots - Wi, start) / N.astype(LD) / (1 + LD(lam)) - LD(bias)
    ev = np.linalg.eigvalsh(A.astype(np.float64))
    scale = np.add.reduceat(np.abs(R) + (np.abs(x[seg]) * np.abs(Vi)).sum(1) + np.abs(Wi), start) / N.astype(LD)
    return dict(ent=ent, x=x, w=w, cond=ev[:, -1] / ev[:, 0], xmax=np.abs(x).max(1).astype(np.float64), N=N,
                vmax=np.maximum.reduceat(np.abs(Vi).sum(1), start).astype(np.float64),
                scale=scale.astype(np.float64) + abs(bias) * (1 + lam))


def bounds(ref, lam, k=1.0):
    """(dx, dw) per entity at the constant k"""
    d = ref["x"].shape[1]
    dx = k * EPS * ref["cond"] * ref["xmax"]
    return dx, (d * dx * ref["vmax"] + k * EPS * (ref["N"] + d) * ref["scale"]) / (1 + lam)


def ratios(ref, x, w, lam):
    """(rho_x, rho_w) per entity: the error of (x, w) in units of the bound at K = 1.  An entity whose bound is 0 (x_ref = 0)
    and whose error is 0 has ratio 0."""
    dx, dw = bounds(ref, lam)
    ex = np.abs(np.asarray(x).astype(LD) - ref["x"]).max(1).astype(np.float64) if len(x) else np.zeros(0)
    ew = np.abs(np.asarray(w).astype(LD) - ref["w"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ex == 0, 0.0, ex / dx), np.where(ew == 0, 0.0, ew / dw)


def check_half(ref, x, w, lam, k, chunks=None, what=""):
    """[] or one line naming the worst entity of x and of w that is outside k times its bound (NaN counts as outside)"""
    if ref["ent"].size == 0:
        return []
    rx, rw = ratios(ref, x, w, lam)
    bad = []
    for name, rho in (("x", rx), ("w", rw)):
        out = ~(rho <= k)
        if out.any():
            i = int(np.flatnonzero(out)[np.argmax(np.where(np.isnan(rho[out]), np.inf, rho[out]))])
            e = int(ref["ent"][i])
            bad.append("%s %s: %d of %d entities outside the bound, worst entity %d: ratio %.3g > K = %g at d = %d, N = %d, "
                       "chunks = %d, cond = %.3g" % (what, name, int(out.sum()), out.size, e, rho[i], k, ref["x"].shape[1],
                                                     int(ref["N"][i]), 0 if chunks is None else int(chunks[e]), ref["cond"][i]))
    return bad


# ----------------------------------------------------------------------------- float64 in the kernels' order
def _accumulate(rows, coef, acc, accb, fault):
    """als_accumulate: 32-rating tiles, inside a tile rating after rating into the running sums"""
    for s in range(0, rows.shape[0], TILE):
        t, c = rows[s:s + TILE], coef[s:s + TILE]
        if fault == "drop_partial_tile" and t.shape[0] < TILE:
            break
        o = t[:, :, None] * t[:, None, :]
        if fault == "skip_slot3":
            o.reshape(t.shape[0], -1)[:, 3 * THREADS:] = 0.0
        acc = np.cumsum(np.concatenate((acc[None], o)), axis=0)[-1]
        accb = np.cumsum(np.concatenate((accb[None], c[:, None] * t)), axis=0)[-1]
    return acc, accb


def half_sweep_f64(own, w_own, other, w_other, lists, entities, bias, lam, ch=CHUNK, fault=None):
    """(x [n, d], w [n]) in float64 in the order of k_als_partial / k_als_fit.  ``fault`` plants one error:
    drop_partial_tile, skip_slot3 (A entries 768.. never accumulated), drop_last_chunk, n_minus_1 (lambda (N - 1))."""
    ent = np.asarray(entities, np.int64)
    ptr, ids, vals = lists
    d = own.shape[1]
    A, B = np.zeros((ent.size, d, d)), np.zeros((ent.size, d))
    for i, e in enumerate(ent):
        lo, hi = int(ptr[e]), int(ptr[e + 1])
        J = ids[lo:hi]
        rows = other[J]
        coef = vals[lo:hi] - w_other[J] - (w_own[e] + bias)
        acc, accb = np.zeros((d, d)), np.zeros(d)
        if hi - lo > ch:
            starts = list(range(0, hi - lo, ch))
            for s in starts[:-1] if fault == "drop_last_chunk" else starts:
                pa, pb = _accumulate(rows[s:s + ch], coef[s:s + ch], np.zeros((d, d)), np.zeros(d), fault)
                acc, accb = acc + pa, accb + pb
        else:
            acc, accb = _accumulate(rows, coef, acc, accb, fault)
        n = hi - lo - 1 if fault == "n_minus_1" else hi - lo
        A[i], B[i] = acc + np.eye(d) * (lam * float(n)), accb
    with np.errstate(invalid="ignore", divide="ignore"):
        x = chol_solve(A, B) if ent.size else B
    w = np.zeros(ent.size)
    for i, e in enumerate(ent):
        lo, hi = int(ptr[e]), int(ptr[e + 1])
        J = ids[lo:hi]
        v = other[J]
        dot = np.zeros(hi - lo)
        for c in range(d):
            dot = dot + x[i, c] * v[:, c]
        term = vals[lo:hi] - dot - w_other[J]
        pad = np.zeros(-(-(hi - lo) // THREADS) * THREADS)
        pad[:hi - lo] = term
        red = np.cumsum(np.concatenate((np.zeros((1, THREADS)), pad.reshape(-1, THREADS))), axis=0)[-1]
        o = THREADS // 2
        while o >= 1:
            red[:o] = red[:o] + red[o:2 * o]
            o //= 2
        w[i] = red[0] / float(hi - lo) / (1.0 + lam) - bias
    return x, w


def predict(U, V, Wu, Ww, bias, u, w):
    """(U[u] . V[w] + W_user[u] + W_work[w] + bias, the sum of the terms' magnitudes) in longdouble"""
    pu, pv = U[u].astype(LD), V[w].astype(LD)
    val = (pu * pv).sum(1) + Wu[u].astype(LD) + Ww[w].astype(LD) + LD(bias)
    return val, (np.abs(pu * pv).sum(1) + np.abs(Wu[u]) + np.abs(Ww[w]) + abs(bias)).astype(np.float64)


# ----------------------------------------------------------------------------- one sweep, its two halves told apart
def check_sweep(case, after, k, report=None):
    """``after`` holds U, V, W_user, W_work one sweep after the case's own tables.  The user half is held to the reference
    from the case's V, W_work and W_user; the work half to the reference fed the U and W_user of ``after`` itself, so an
    error of one half fails that half's statements only.  Returns the violated statements."""
    (lu, users), (lw, works) = sides(case)
    ch, lam, bias = chunk_size(case["ch"]), case["lam"], case["bias"]
    bad = []
    for what, lists, ent, own0, w0, own1, w1, other, w_other in (
            ("user half", lu, users, case["U"], case["Wu"], after["U"], after["W_user"], case["V"], case["Ww"]),
            ("work half", lw, works, case["V"], case["Ww"], after["V"], after["W_work"], after["U"], after["W_user"])):
        if not (np.isfinite(other).all() and np.isfinite(w_other).all()):
            bad.append("%s, %s: not checked, the tables it reads are not finite" % (case["id"], what))
            continue
        ref = half_sweep(own0, w0, other, w_other, lists, ent, bias, lam)
        bad += check_half(ref, own1[ent], w1[ent], lam, k, n_chunks(lists, ch), "%s, %s" % (case["id"], what))
        bad += check_untouched("%s, %s" % (case["id"], what), own0, w0, own1, w1, ent)
        if report is not None:
            rx, rw = ratios(ref, own1[ent], w1[ent], lam)
            report[what] = (float(np.max(rx, initial=0.0)), float(np.max(rw, initial=0.0)))
    return bad


def sweep_f64(case, fault=None):
    """one sweep of the float64 kernel-order restatement from the case's tables.  fault ``fit_all_zero`` fits every entity
    that has a rating; the others are those of ``half_sweep_f64``."""
    (lu, users), (lw, works) = sides(case)
    if fault == "fit_all_zero":
        users, works = np.flatnonzero(np.diff(lu[0])), np.flatnonzero(np.diff(lw[0]))
    ch, lam, bias = chunk_size(case["ch"]), case["lam"], case["bias"]
    U, V, Wu, Ww = (np.array(case[k]) for k in ("U", "V", "Wu", "Ww"))
    U[users], Wu[users] = half_sweep_f64(U, Wu, V, Ww, lu, users, bias, lam, ch, fault)
    V[works], Ww[works] = half_sweep_f64(V, Ww, U, Wu, lw, works, bias, lam, ch, fault)
    return dict(U=U, V=V, W_user=Wu, W_work=Ww)
