"""One SVD training step stated per row: the float64 gradient sum, a first-order bound on what float32 may lose of
it, and the consistency checks that tie a device's moments and weights to its own gradient.  NumPy only.

A step is judged by three separate statements instead of "the table is near the oracle's":

  gradient  the summed gradient g the device used (recovered from its own m, or from w under SGD) lies within
            ``limit * eps32 * E`` of the float64 sum G, E being the per-element bound below;
  moments   v follows from g and the device's previous v to a few roundings;
  apply     w follows from the device's own m and v to a few roundings.

The last two compare the device with itself through float64 arithmetic, so nothing here is ill-conditioned in the way
Adam's first steps (~lr * sign(g)) are when a table is compared with the oracle's table.

eps32 = 2^-24 is the unit throughout (half an ulp of 1.0f, one rounding's relative error)."""
import numpy as np

from oracle import svd_oracle as so

EPS32 = 2.0 ** -24
NAMES = ("P", "Q", "bu", "bi", "mu")
TID = {"mu": so.MU, "bu": so.BU, "bi": so.BI, "P": so.PF, "Q": so.QF}
LONG_RUN = 64                                   # rows with more entries are reported (and limited) as a class of their own
B1F, B2F = np.float32(so.BETA1), np.float32(so.BETA2)
OMB1, OMB2 = float(np.float32(1) - B1F), float(np.float32(1) - B2F)      # 1.f - b1 is exact in float32 for 0.9 and 0.999
EPS_ADAM = float(np.float32(so.EPSILON))


def f64_tables(t):
    return {k: np.asarray(t[k], np.float64) for k in ("mu", "bu", "bi", "P", "Q")}


def seg_sum(values, ids, n):
    """dense (n, ...) float64 sum of ``values`` per id.  Small inputs go through the oracle's ``segment_sum``; large ones
    through a stable sort + ``np.add.reduceat`` (np.add.at on 300000 x 64 takes minutes) - tests/test_step_ref_host.py holds
    the two against each other."""
    values = np.asarray(values)
    if values.size <= 1 << 16:
        return so.segment_sum(values, ids, n)
    out = np.zeros((n,) + values.shape[1:], values.dtype)
    if ids.size == 0:
        return out
    order = np.argsort(ids, kind="stable")
    sk = ids[order]
    heads = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1])))
    out[sk[heads]] = np.add.reduceat(values[order], heads, axis=0)
    return out


def step_grads(t, u, i, r, loss, item_abs, reg_bias, lam):
    """{name: (G, E, n)} for P, Q, bu, bi, mu: G the float64 gradient sum (dense, zero on untouched rows), E the
    first-order float32 loss bound in units of eps32, n the entries per row (broadcastable against G).

    An entry's logit x_k is a float32 sum of the terms p_d q~_d, mu, bu, bi, so it - and with it g_k - is off by up to
    eps32 * X_k, X_k the sum of the terms' magnitudes (+ |r_k| for the subtraction under mse).  Under nll
    g = sigmoid(x) - z: |sigmoid'| <= 1/4 damps the logit's error and sigmoid / the subtraction round once more, |g_k| in
    all.  That error delta_k reaches every product g_k * (partner element); the products and the running sum lose at most
    one rounding of each term's magnitude more, to first order (the sum's growth with n is what ``ratio`` reports per run
    length)."""
    t = f64_tables(t)
    u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    r = np.asarray(r, np.float64)
    P, Q, bu, bi, mu = t["P"], t["Q"], t["bu"], t["bi"], t["mu"]
    U, I = P.shape[0], Q.shape[0]
    x = so.forward(P, Q, bu, bi, mu, u, i, item_abs)
    g = so.dlogits(x, r, loss)
    oP, oQ, obu, obi, _ = so.occurrence_grads(P, Q, bu, bi, u, i, g, lam, item_abs, reg_bias)
    pu, qt = P[u], np.abs(Q[i])
    X = np.sum(np.abs(pu) * qt, axis=1) + abs(float(mu)) + np.abs(bu[u]) + np.abs(bi[i])
    delta = X + np.abs(r) if loss == so.MSE else X / 4 + np.abs(g)
    nu = np.bincount(u, minlength=U).astype(np.int64)
    ni = np.bincount(i, minlength=I).astype(np.int64)
    out = {
        "P": (seg_sum(oP, u, U), seg_sum(np.abs(oP) + delta[:, None] * qt, u, U), nu[:, None]),
        "Q": (seg_sum(oQ, i, I), seg_sum(np.abs(oQ) + delta[:, None] * np.abs(pu), i, I), ni[:, None]),
        "bu": (seg_sum(obu, u, U), seg_sum(np.abs(obu) + delta, u, U), nu),
        "bi": (seg_sum(obi, i, I), seg_sum(np.abs(obi) + delta, i, I), ni),
        "mu": (np.float64(g.sum()), np.float64(np.sum(np.abs(g) + delta)), np.int64(u.size)),
    }
    return out, x, g


def f32_oracle_grads(t, u, i, r, loss, item_abs, reg_bias, lam, rows=None):
    """The same sums the way ``SvdOracle(dtype=np.float32)`` forms them: float32 arithmetic, zero-initialised rows,
    ``np.add.at`` in batch order (the TF CPU kernel's order).  ``rows = {"P": ids, "Q": ids}`` restricts the two feature
    tables to a sample of rows (every entry of a sampled row is still added, in order); other rows stay zero."""
    f = {k: np.asarray(t[k], np.float32) for k in ("mu", "bu", "bi", "P", "Q")}
    u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    r = np.asarray(r, np.float32)
    x = so.forward(f["P"], f["Q"], f["bu"], f["bi"], f["mu"], u, i, item_abs)
    g = so.dlogits(x, r, loss).astype(np.float32)
    out = {}
    for name, ids, n in (("P", u, f["P"].shape[0]), ("Q", i, f["Q"].shape[0])):
        sel = slice(None) if rows is None else np.flatnonzero(np.isin(ids, rows[name]))
        uu, ii, gg = u[sel], i[sel], g[sel]
        occ = so.occurrence_grads(f["P"], f["Q"], f["bu"], f["bi"], uu, ii, gg, lam, item_abs, reg_bias)[0 if name == "P" else 1]
        out[name] = so.segment_sum(occ, ids[sel], n)
    _, _, obu, obi, _ = so.occurrence_grads(f["P"][:, :1], f["Q"][:, :1], f["bu"], f["bi"], u, i, g, lam, item_abs, reg_bias)
    out["bu"] = so.segment_sum(obu, u, f["bu"].shape[0])
    out["bi"] = so.segment_sum(obi, i, f["bi"].shape[0])
    out["mu"] = np.cumsum(g, dtype=np.float32)[-1] if g.size else np.float32(0)      # cumsum adds in order
    return out


def ratio(g, G, E, n, rows=None):
    """{"short": x, "long": y}: max |g - G| / (eps32 * E) over the elements with E > 0, for rows of at most LONG_RUN
    entries and for longer ones (a long run legitimately loses ~sqrt(n) more).  A class without elements reports 0.
    ``rows`` restricts the comparison to a sample of rows."""
    g, G, E = np.asarray(g, np.float64), np.asarray(G, np.float64), np.asarray(E, np.float64)
    n = np.broadcast_to(np.asarray(n), E.shape)
    ok = E > 0
    if rows is not None:
        pick = np.zeros(E.shape[0], bool)
        pick[rows] = True
        ok = ok & (pick[:, None] if E.ndim == 2 else pick)
    q = np.zeros(E.shape)
    np.divide(np.abs(g - G), EPS32 * E, out=q, where=ok)
    out = {}
    for cls, mask in (("short", ok & (n <= LONG_RUN)), ("long", ok & (n > LONG_RUN))):
        out[cls] = float(q[mask].max()) if mask.any() else 0.0
    return out


def limit_from(c_ref):
    """what the device may reach where the float32 oracle reaches c_ref: a sum in pieces and trees should lose less than a
    sequential one; 2 covers another order on the same data and __expf / fused multiply-adds in the logit; the floor 4
    keeps a class of a handful of elements from setting a limit below two roundings"""
    return {cls: max(4.0, 2.0 * c) for cls, c in c_ref.items()}


# ----------------------------------------------------------------------------- the device's own gradient
def grad_from_fresh_adam(m_now):
    """fresh slots: m = fl(g * (1 - b1)), so g = m / (1 - b1).  One rounding of m: |g| more in E."""
    g = np.asarray(m_now, np.float64) / OMB1
    return g, np.abs(g)


def grad_from_adam(m_now, m_prev):
    """m_t = fl(b1 * m_{t-1} + fl(g (1 - b1))) (fused multiply-add; bias_global: m += fl(fl(g - m) (1 - b1))), so
    g = (m_t - b1 m_{t-1}) / (1 - b1).  Roundings: m_t itself (|m_t|), the product (|g| (1 - b1)), and for bias_global
    the difference g - m (|g| + |m_{t-1}|, times (1 - b1)); divided by (1 - b1): |m_t| / (1 - b1) + 2 |g| + |m_{t-1}|."""
    m_now, m_prev = np.asarray(m_now, np.float64), np.asarray(m_prev, np.float64)
    g = (m_now - float(B1F) * m_prev) / OMB1
    return g, np.abs(m_now) / OMB1 + 2 * np.abs(g) + np.abs(m_prev)


def grad_from_sgd(w_before, w_after, lr):
    """w' = fl(w - lr g) with lr a power of two (lr g is exact): g = (w - w') / lr; one rounding of w': |w| / lr."""
    assert np.log2(lr) == int(np.log2(lr)), "lr must be a power of two"
    w_before, w_after = np.asarray(w_before, np.float64), np.asarray(w_after, np.float64)
    return (w_before - w_after) / lr, np.maximum(np.abs(w_before), np.abs(w_after)) / lr


def alpha_f32(lr, b1p, b2p):
    """lr_t as the library forms it on the host, in float32 and in its order: lr * sqrtf(1 - b2p) / (1 - b1p)"""
    one = np.float32(1)
    return float(np.float32(lr) * np.sqrt(one - np.float32(b2p)) / (one - np.float32(b1p)))


# ----------------------------------------------------------------------------- consistency (arrays only)
def moments_excess(v_prev, v_now, g, dg=0.0):
    """max of |v_now - (b2 v_prev + (1 - b2) g^2)| over its allowance, 8 eps32 of the larger term: v takes four float32
    roundings (g g, times (1 - b2), the fused b2 v + ., and g itself comes from a rounded m), doubled.  Past the first step
    g carries the recovery's own rounding dg (``grad_from_adam``'s second value times eps32), which reaches v as
    (1 - b2)(2 |g| dg + dg^2): counted, not measured.  <= 1 passes."""
    v_prev, v_now, g = (np.asarray(a, np.float64) for a in (v_prev, v_now, g))
    a, b = float(B2F) * v_prev, OMB2 * g * g
    allow = 8 * EPS32 * np.maximum(a, b) + OMB2 * (2 * np.abs(g) * dg + dg * dg)
    diff = np.abs(v_now - (a + b))
    return _excess(diff, allow)


def apply_excess(w_before, w_after, m_now, v_now, alpha):
    """max of |w_after - (w_before - alpha m / (sqrt(v) + eps))| over 2 eps32 (|w_before| + 4 |update|): the update takes
    four roundings (alpha m, sqrt, + eps, the division), the subtraction one.  <= 1 passes."""
    w_before, w_after, m_now, v_now = (np.asarray(a, np.float64) for a in (w_before, w_after, m_now, v_now))
    upd = alpha * m_now / (np.sqrt(v_now) + EPS_ADAM)
    allow = 2 * EPS32 * (np.abs(w_before) + 4 * np.abs(upd))
    return _excess(np.abs(w_after - (w_before - upd)), allow)


def _excess(diff, allow):
    diff, allow = np.atleast_1d(diff), np.atleast_1d(allow)
    if diff.size == 0:
        return 0.0
    if not np.isfinite(diff).all():
        return float("inf")
    q = np.where(allow > 0, diff / np.where(allow > 0, allow, 1.0), np.where(diff > 0, np.inf, 0.0))
    return float(q.max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_step(before, after, u, i, r, *, opt, mode, loss, item_abs, reg_bias, lam, lr, powers, fresh, frozen=0,
               sample=None, report=None):
    """Every per-row statement about one step.  ``before`` / ``after``: {name: dict(w=, m=, v=)} of float32 arrays as read
    from the device around the step (m, v absent under SGD); ``powers`` = (b1p, b2p) before the step; ``fresh``: the slots
    were all zero before.  Returns the list of violated statements (empty = the step is right); ``report`` (a dict)
    receives the measured ratios."""
    bad = []
    adam, tf1 = opt == so.ADAM, opt == so.ADAM and mode == so.TF1
    tabs = {k: before[k]["w"] for k in NAMES}
    ref, _, _ = step_grads(tabs, u, i, r, loss, item_abs, reg_bias, lam)
    rows = None
    if sample is not None:
        rows = {}
        for name, ids in (("P", u), ("Q", i)):
            n = np.bincount(ids, minlength=before[name]["w"].shape[0])
            touched = np.flatnonzero(n)
            pick = touched[np.random.RandomState(7).permutation(touched.size)[:sample]]
            rows[name] = np.union1d(pick, np.argsort(n, kind="stable")[-20:])
    f32 = f32_oracle_grads(tabs, u, i, r, loss, item_abs, reg_bias, lam, rows)
    alpha = alpha_f32(lr, *powers) if adam else 0.0
    for name in NAMES:
        G, E, n = ref[name]
        check_table(bad, name, G, E, n, before[name], after[name], f32[name], adam=adam, tf1=tf1, fresh=fresh, lr=lr,
                    alpha=alpha, frozen=frozen >> TID[name] & 1, srows=rows.get(name) if rows else None, report=report)
    return bad


def check_table(bad, name, G, E, n, b, a, f32g, *, adam, tf1, fresh, lr, alpha, frozen=0, srows=None, report=None):
    """The statements about one table (``check_step``'s loop body; tests/fm_ref.py states the FM tables with it): ``G, E, n``
    as ``step_grads`` returns them, ``b`` / ``a`` the table's dict(w=, m=, v=) before and after, ``f32g`` the float32
    oracle's gradient.  "mu" is the scalar, judged as a table of one row.  Appends the violated statements to ``bad``."""
    if name == "mu":                                  # the scalar as a table of one row
        G, E, n = (np.reshape(x, (1,)) for x in (G, E, n))
        b, a = ({k: np.reshape(np.asarray(x, np.float32), (1,)) for k, x in d.items()} for d in (b, a))
        f32g = np.reshape(f32g, (1,))
    if frozen:
        for slot in b:
            if not same_bits(b[slot], a[slot]):
                bad.append("%s.%s: a frozen table changed" % (name, slot))
        return
    touched = np.broadcast_to(np.asarray(n) > 0, np.shape(G))
    # -- gradient
    if adam:
        g, extra = grad_from_fresh_adam(a["m"]) if fresh else grad_from_adam(a["m"], b["m"])
    else:
        g, extra = grad_from_sgd(b["w"], a["w"], lr)
    if not tf1 and name != "mu":
        extra = np.where(touched, extra, 0.0)        # lazy Adam, SGD: an untouched row is held to identical bits below
    c_ref = ratio(f32g, G, E, n, srows)
    lim = limit_from(c_ref)
    got = ratio(g, G, E + extra, n)
    if report is not None:
        report[name] = dict(c_ref=c_ref, dev=got)
    for cls in ("short", "long"):
        if not got[cls] <= lim[cls]:
            bad.append("%s gradient, %s runs: %.1f x eps32 x E, limit %.1f (float32 oracle %.1f)"
                       % (name, cls, got[cls], lim[cls], c_ref[cls]))
    # -- moments and apply, against the device's own numbers
    if adam:
        # lazy Adam moves the touched rows only (the others are held to identical bits below); TF1 and bias_global: all
        act = touched if (not tf1 and name != "mu") else np.ones(np.shape(G), bool)
        dg = 0.0 if fresh else (EPS32 * extra)[act]
        ex = moments_excess(b["v"][act], a["v"][act], g[act], dg)
        if not ex <= 1:
            bad.append("%s: v does not follow from g and the previous v (%.2f x its allowance)" % (name, ex))
        ex = apply_excess(b["w"][act], a["w"][act], a["m"][act], a["v"][act], alpha)
        if not ex <= 1:
            bad.append("%s: w does not follow from m and v (%.2f x its allowance)" % (name, ex))
    # -- rows the batch did not touch
    if name != "mu" and not touched.all():
        still = ~touched
        if not tf1 or fresh:                          # TF1 with all-zero moments: the dense sweep moves nothing
            for slot in b:
                if not same_bits(b[slot][still], a[slot][still]):
                    bad.append("%s.%s: rows outside the batch changed" % (name, slot))
        elif not same_bits(a["m"][still], (b["m"][still].astype(np.float64) * float(B1F)).astype(np.float32)):
            bad.append("%s.m: rows outside the batch did not decay by b1" % name)
