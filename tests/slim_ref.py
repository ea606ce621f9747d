"""NumPy restatement of SLIM (include/tfrecomm.h, the tfr_slim block): what tests/test_slim_host.py checks by hand and
tests/test_gpu_slim.py holds the device to, bit for bit.

``solve_column`` is the header's pseudo-code, line for line, for one column.  ``solve`` runs every column at once: the columns
are independent and walk the coordinates in the same order, so step ``i`` of a sweep is one vector operation over the columns
still running; each column sees exactly the operations of ``solve_column`` (tests/test_slim_host.py holds the two against each
other).  NumPy rounds ``dl * A[i]`` and the subtraction separately, which is the contract.  The Gram matrix is
``tests/ease_ref.gram`` with ``lam = beta``; scores, keys, top-K and ranks are ``tests/ease_ref``'s on ``W``.

``kkt_excess`` measures in long double how far a ``W`` is from the optimality conditions of the columns' problems, whatever
path produced it."""
import numpy as np

from tests.ease_ref import gram, keys, ranks, topk, user_scores  # noqa: F401  (Gram and serving are EASE's, word for word)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def solve_column(A, j, l1, positive=True, max_iter=100, tol=1e-4):
    """(w float64 [n], sweeps, updates, converged) of column j"""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    l1, tol = np.float64(l1), np.float64(tol)
    q = A[:, j].copy()
    w = np.zeros(n)
    d = np.diag(A).copy()
    updates, sweep, conv = 0, 0, False
    while sweep < max_iter:
        sweep += 1
        dmax = np.float64(0)
        for i in range(n):
            if i == j or not d[i] > 0:
                continue
            if positive:
                t = q[i] - l1
                wn = t / d[i] if t > 0 else np.float64(0)
            else:
                t = np.abs(q[i]) - l1
                wn = np.copysign(t / d[i], q[i]) if t > 0 else np.float64(0)
            dl = wn - w[i]
            if dl != 0:
                own = q[i]
                q = q - dl * A[i]                          # the product rounds, then the difference
                q[i] = own                                 # k != i
                w[i] = wn
                updates += 1
                dmax = max(dmax, np.abs(dl))
        if dmax <= tol * np.abs(w).max():
            conv = True
            break
    return w, sweep, updates, conv


def to_f32(w64):
    """W's storage: the float32 of each non-zero weight, +0 elsewhere"""
    w64 = np.asarray(w64, np.float64)
    return np.where(w64 != 0, w64.astype(np.float32), np.float32(0)).astype(np.float32)


def solve(A, l1, positive=True, max_iter=100, tol=1e-4):
    """(W float32 [n, n], sweeps int32 [n], updates int32 [n], converged bool [n], W64 float64 [n, n]) of all columns"""
    A = np.ascontiguousarray(A, np.float64)
    n = A.shape[0]
    l1, tol = np.float64(l1), np.float64(tol)
    d = np.diag(A).copy()
    Q = A.copy()                                           # Q[j] = q of column j (A is symmetric: row j is column j)
    Wt = np.zeros((n, n))                                  # Wt[j] = w of column j
    sweeps, updates = np.zeros(n, np.int32), np.zeros(n, np.int32)
    conv, active = np.zeros(n, bool), np.ones(n, bool)
    for sweep in range(1, max_iter + 1):
        cols = np.flatnonzero(active)
        if cols.size == 0:
            break
        sweeps[cols] = sweep
        dmax = np.zeros(n)
        for i in range(n):
            if not d[i] > 0:
                continue
            c = cols[cols != i]
            qi = Q[c, i]
            if positive:
                t = qi - l1
                wn = np.where(t > 0, t / d[i], 0.0)
            else:
                t = np.abs(qi) - l1
                wn = np.where(t > 0, np.copysign(t / d[i], qi), 0.0)
            dl = wn - Wt[c, i]
            nz = dl != 0
            if not nz.any():
                continue
            cc, dln = c[nz], dl[nz]
            own = Q[cc, i].copy()
            Q[cc] = Q[cc] - dln[:, None] * A[i][None, :]
            Q[cc, i] = own
            Wt[cc, i] = wn[nz]
            updates[cc] += 1
            dmax[cc] = np.maximum(dmax[cc], np.abs(dln))
        done = dmax[cols] <= tol * np.abs(Wt[cols]).max(axis=1)
        conv[cols[done]] = True
        active[cols[done]] = False
    W64 = np.ascontiguousarray(Wt.T)
    return to_f32(W64), sweeps, updates, conv, W64


def kkt_excess(A, W, l1, positive=True):
    """(excess, r) long double [n, n]: for column j and coordinate i != j with d_i > 0, r[i, j] = a_ij - sum over k != i of
    A[i, k] W[k, j], and excess[i, j] = how far (i, j) is from optimal:
        W[i, j] > 0:  |r - l1 - d_i W[i, j]|        W[i, j] < 0 (not positive):  |r + l1 - d_i W[i, j]|
        W[i, j] = 0:  max(r - l1, 0) when positive, max(|r| - l1, 0) otherwise
    and 0 on the diagonal and where d_i <= 0"""
    A = np.asarray(A).astype(LD)
    W = np.asarray(W).astype(LD)
    d = np.diag(A).copy()
    r = A - A @ W + d[:, None] * W
    l1 = LD(l1)
    at_zero = np.maximum(r - l1, 0) if positive else np.maximum(np.abs(r) - l1, 0)
    ex = np.where(W > 0, np.abs(r - l1 - d[:, None] * W), np.where(W < 0, np.abs(r + l1 - d[:, None] * W), at_zero))
    ex[~(d > 0), :] = 0
    np.fill_diagonal(ex, 0)
    return ex, r
