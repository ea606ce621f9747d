"""One factorisation-machine training step stated per row, and the FM forward per row: the float64 gradient sum of the
contract in include/tfrecomm.h, a first-order bound on what float32 may lose of it, a float32 restatement in batch order
that sets the limit, and the consistency checks of tests/step_ref.py on the device's own moments and weights.  NumPy only.

Per stored entry (row r, feature j, value x), with s_r = sum_j x V_j and g_r = d loss / d y_r:

    dV_j += g_r x (s_r - x V_j) + lam V_j        dW_j += g_r x + lam W_j        dmu += g_r  (once per row)

An entry is what the CSR stores: an explicit zero and a second entry of the same column in a row are entries of their own."""
import numpy as np

from oracle import svd_oracle as so
from tests import step_ref as R

NAMES = ("V", "W", "mu")
TID = {"mu": so.MU, "W": so.BU, "V": so.PF}               # the wrapped model's tables (csrc/api.hip tfr_fm)


def _entries(indptr, indices, data):
    indptr = np.asarray(indptr, np.int64)
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    return rows, np.asarray(indices, np.int64), indptr.size - 1


def forward_terms(mu, W, V, indptr, indices, data):
    """float64: dict(y = the prediction per row, X = the magnitudes its error scales with, S = x V per row, A = sum |x v|
    per row and element, nnz = entries per row).

    y_r = (mu + sum x w) + 0.5 sum_d (s_d^2 - q_d), s_d = sum_j x v_jd, q_d = sum_j (x v_jd)^2.  In float32 each term is
    rounded once where it is formed and once where it is added: mu and the x w by their magnitudes; s_d by A_d = sum_j
    |x v_jd|, which reaches 0.5 s_d^2 as |s_d| A_d; the square itself 0.5 s_d^2; a product x v rounded before it is
    squared moves 0.5 (x v)^2 by (x v)^2, and q_d's sum adds 0.5 q_d: X_r = |mu| + sum |x w| + sum_d (0.5 s_d^2 +
    |s_d| A_d + 1.5 q_d).  The growth with the row's length is what ``ratio`` reports per length class."""
    mu, W, V = float(mu), np.asarray(W, np.float64), np.asarray(V, np.float64)
    rows, f, n = _entries(indptr, indices, data)
    x = np.asarray(data, np.float64)
    xv = x[:, None] * V[f]
    S, A, Q = (R.seg_sum(t, rows, n) for t in (xv, np.abs(xv), xv * xv))
    xw = x * W[f]
    y = mu + R.seg_sum(xw, rows, n) + 0.5 * np.sum(S * S - Q, axis=1)
    X = abs(mu) + R.seg_sum(np.abs(xw), rows, n) + np.sum(0.5 * S * S + np.abs(S) * A + 1.5 * Q, axis=1)
    return dict(y=y, X=X, S=S, A=A, nnz=np.bincount(rows, minlength=n).astype(np.int64))


def fm_step_grads(mu, W, V, indptr, indices, data, y, loss, lam):
    """({"V": (G, E, n), "W": ..., "mu": ...}, terms): G the float64 gradient sum of the contract (dense, zero on features
    outside the batch), E the first-order float32 loss bound in units of eps32, n the entries per feature (rows for mu);
    ``terms`` is ``forward_terms`` plus g and the data loss with its own bound.

    The prediction is off by up to eps32 X_r (``forward_terms``), so g_r by delta_r = X_r + |y_r| under mse (the
    subtraction) and X_r / 4 + |g_r| under nll (|sigmoid'| <= 1/4; sigmoid and the subtraction round once more).  An
    entry's V contribution is formed as a s + b V_j with a = g x and b = lam - a x:
      delta_r |x| |s - x V_j|         the error of g reaches both terms through the same a
      |g x| A                         the error of s_r, per element
      |g x s|                         a is rounded
      4 |g x^2 V_j| + 2 lam |V_j|     a, a x, the subtraction b and b V_j are rounded
      2 |contribution|                the sum a s + b V_j, and one rounding as a term of the feature's sum
    An entry's W contribution g x + lam W_j: delta_r |x|, |g x| and lam |W_j| for the two products, 2 |contribution| as
    above.  mu: delta_r + |g_r| per row.  The data loss sum_r l_r moves by |g_r| eps32 X_r with the prediction (g is its
    derivative) and each l_r is rounded where it is formed and where it is added: sum_r (|g_r| X_r + 2 |l_r|)."""
    t = forward_terms(mu, W, V, indptr, indices, data)
    W, V = np.asarray(W, np.float64), np.asarray(V, np.float64)
    rows, f, n = _entries(indptr, indices, data)
    x, y = np.asarray(data, np.float64), np.asarray(y, np.float64)
    F = V.shape[0]
    g = so.dlogits(t["y"], y, loss)
    delta = t["X"] + np.abs(y) if loss == so.MSE else t["X"] / 4 + np.abs(g)
    gx, vf, S = g[rows] * x, V[f], t["S"][rows]
    xvf = x[:, None] * vf
    rest = S - xvf
    occV = gx[:, None] * rest + lam * vf
    EV = ((delta[rows] * np.abs(x))[:, None] * np.abs(rest) + np.abs(gx)[:, None] * (t["A"][rows] + np.abs(S) + 4 * np.abs(xvf))
          + 2 * lam * np.abs(vf) + 2 * np.abs(occV))
    occW = gx + lam * W[f]
    EW = delta[rows] * np.abs(x) + np.abs(gx) + lam * np.abs(W[f]) + 2 * np.abs(occW)
    nf = np.bincount(f, minlength=F).astype(np.int64)
    lrow = _row_loss(t["y"], y, loss)
    t.update(g=g, loss=(np.float64(lrow.sum()), np.float64(np.sum(np.abs(g) * t["X"] + 2 * np.abs(lrow))), np.int64(n)))
    out = {
        "V": (R.seg_sum(occV, f, F), R.seg_sum(EV, f, F), nf[:, None]),
        "W": (R.seg_sum(occW, f, F), R.seg_sum(EW, f, F), nf),
        "mu": (np.float64(g.sum()), np.float64(np.sum(np.abs(g) + delta)), np.int64(n)),
    }
    return out, t


def _row_loss(yhat, y, loss):
    """the data loss per row (``so.data_loss`` is their sum)"""
    if loss == so.MSE:
        return 0.5 * (yhat - y) ** 2
    return np.maximum(yhat, 0) - yhat * y + np.log1p(np.exp(-np.abs(yhat)))


def f32_fm(mu, W, V, indptr, indices, data, y=None, loss=None, lam=0.0):
    """The same numbers in float32 arithmetic the way ``so.fm_train_step`` forms them on float32 tables: the contract's
    expressions as written, every sum by ``so.segment_sum`` (``np.add.at``, entry order: a row's entries in CSR order, a feature's in batch
    order).  dict(y=) for the forward alone; with targets also V, W, mu (the gradients) and loss.  It supplies c_ref."""
    f4 = np.float32
    mu, W, V = f4(mu), np.asarray(W, f4), np.asarray(V, f4)
    rows, f, n = _entries(indptr, indices, data)
    x = np.asarray(data, f4)
    xv = x[:, None] * V[f]
    S = so.segment_sum(xv, rows, n)
    yhat = (mu + so.segment_sum(x * W[f], rows, n)) + f4(0.5) * np.sum(S * S - so.segment_sum(xv * xv, rows, n), axis=1, dtype=f4)
    out = dict(y=yhat)
    if y is None:
        return out
    y = np.asarray(y, f4)
    g = so.dlogits(yhat, y, loss).astype(f4)
    gx = g[rows] * x
    F = V.shape[0]
    out["V"] = so.segment_sum(gx[:, None] * (S[rows] - xv) + f4(lam) * V[f], f, F)
    out["W"] = so.segment_sum(gx + f4(lam) * W[f], f, F)
    out["mu"] = np.cumsum(g, dtype=f4)[-1] if n else f4(0)             # cumsum adds in order
    lrow = _row_loss(yhat, y, loss).astype(f4)
    out["loss"] = np.cumsum(lrow, dtype=f4)[-1] if n else f4(0)
    return out


def forward_excess(pred, mu, W, V, indptr, indices, data, report=None, what="forward"):
    """Every row's prediction within ``limit * eps32 * X_r`` of float64, X_r the row's own term magnitudes and the limit
    ``limit_from`` of the float32 restatement, per row-length class (at most LONG_RUN entries, longer): a row with a small
    prediction is held as tightly as one with a large one.  Returns the violated statements."""
    t = forward_terms(mu, W, V, indptr, indices, data)
    c_ref = R.ratio(f32_fm(mu, W, V, indptr, indices, data)["y"], t["y"], t["X"], t["nnz"])
    return _held(what, np.asarray(pred, np.float64), t["y"], t["X"], t["nnz"], c_ref, report)


def _held(what, got, G, E, n, c_ref, report):
    lim, dev = R.limit_from(c_ref), R.ratio(got, G, E, n)
    if report is not None:
        report[what] = dict(c_ref=c_ref, dev=dev)
    return ["%s, %s rows: %.1f x eps32 x X, limit %.1f (float32 restatement %.1f)" % (what, cls, dev[cls], lim[cls], c_ref[cls])
            for cls in ("short", "long") if not dev[cls] <= lim[cls]]


def check_fm_step(before, after, csr, y, *, opt, loss, lam, lr, powers, fresh, pred=None, lossv=None, report=None):
    """Every per-row statement about one FM step.  ``before`` / ``after``: {"V" | "W" | "mu": dict(w=, m=, v=)} of float32
    arrays read around the step (m, v absent under SGD); ``csr`` = (indptr, indices, data); ``powers`` = (b1p, b2p) before
    the step; ``fresh``: the slots were all zero before.  Per table (mu as a table of one row) and run-length class the
    gradient the device used lies within ``limit_from(c_ref)`` x eps32 x E of the float64 sum; v follows from g and the
    previous v; w from the device's own m and v; every slot of a feature outside the batch keeps its bits
    (``step_ref.check_table``: FM trains with SGD or lazy Adam).  ``pred`` and ``lossv`` (the step's predictions and data
    loss), when given, are held per row and as a sum of one row.  Returns the list of violated statements."""
    indptr, indices, data = csr
    tabs = [before[k]["w"] for k in ("mu", "W", "V")]
    ref, t = fm_step_grads(*tabs, indptr, indices, data, y, loss, lam)
    f32 = f32_fm(*tabs, indptr, indices, data, y, loss, lam)
    adam = opt == so.ADAM
    alpha = R.alpha_f32(lr, *powers) if adam else 0.0
    bad = []
    for name in NAMES:
        G, E, n = ref[name]
        R.check_table(bad, name, G, E, n, before[name], after[name], f32[name], adam=adam, tf1=False, fresh=fresh, lr=lr,
                      alpha=alpha, report=report)
    if pred is not None:
        bad += _held("forward", np.asarray(pred, np.float64), t["y"], t["X"], t["nnz"],
                     R.ratio(f32["y"], t["y"], t["X"], t["nnz"]), report)
    if lossv is not None:
        G, E, n = (np.reshape(a, (1,)) for a in t["loss"])
        bad += _held("loss", np.reshape(np.float64(lossv), (1,)), G, E, n, R.ratio(np.reshape(f32["loss"], (1,)), G, E, n), report)
    return bad
