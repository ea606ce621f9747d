"""NumPy restatement of EASE (include/tfrecomm.h, the tfr_ease block): what tests/test_ease_host.py checks by hand and
tests/test_gpu_ease.py holds the device to.

The Gram matrix is ``X.T @ X`` in int64 plus lambda on the diagonal; the weights are the float64 expression
``-P / diag(P)`` rounded once by ``astype(float32)``; user scores are a Python loop of float32 adds in list order; keys, top-K
and ranks are those of tests/itemknn_ref.py (the ``tfr_topk`` key over all non-excluded items).

Two inverses: ``inverse_ld``, a Cholesky inverse in ``np.longdouble`` written out in NumPy (the reference the device's error
is measured against), and ``inverse_blocked``, float64 in the device's own order - the same block size and the same stage
sequence as csrc/ease.hip - whose error against ``inverse_ld`` gives the error constant of the GPU tests."""
import numpy as np

from tests.itemknn_ref import keys, pattern, ranks, topk  # noqa: F401  (the serving side is ItemKNN's, word for word)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def gram(indptr, items, n_users, n_items, lam):
    """float64 [n_items, n_items]: the exact integers of X^T X, (double)n_i + lam on the diagonal"""
    x = pattern(indptr, items, n_users, n_items)
    c = np.asarray((x.T @ x).todense()).astype(np.int64)
    g = c.astype(np.float64)
    idx = np.arange(n_items)
    g[idx, idx] = np.diag(c).astype(np.float64) + np.float64(lam)
    return g


def weights(P):
    """float32 B from a float64 (or long double) P: one division, one rounding, +0 on the diagonal"""
    P = np.asarray(P)
    B = (-P / np.diag(P)[None, :]).astype(np.float32)
    np.fill_diagonal(B, np.float32(0))
    return B


def user_scores(lst, B):
    """float32 [n_items]: the add chain from +0 over the list in the order given (ascending)"""
    acc = np.zeros(B.shape[1], np.float32)
    for i in lst:
        acc = acc + B[i]
    return acc


def inverse_ld(G):
    """G^-1 in long double: G = L L^T column by column, L^-1 row by row, P = L^-T L^-1"""
    A = np.asarray(G).astype(LD)
    n = A.shape[0]
    Lo = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - (Lo[j, :j] * Lo[j, :j]).sum()
        assert d > 0, "not positive definite at column %d" % j
        Lo[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lo[j + 1:, j] = (A[j + 1:, j] - Lo[j + 1:, :j] @ Lo[j, :j]) / Lo[j, j]
    Li = np.zeros_like(A)
    for i in range(n):
        Li[i, i] = LD(1) / Lo[i, i]
        if i:
            Li[i, :i] = -(Lo[i, :i] @ Li[:i, :i]) / Lo[i, i]
    return Li.T @ Li


def _diag_block(S):
    """k_ease_diag: (factor, its inverse) of one block, float64, in the kernel's order; None at a pivot that is not positive"""
    S = np.tril(S).copy()
    b = S.shape[0]
    for c in range(b):
        p = S[c, c]
        if not (p > 0 and np.isfinite(p)):
            return None, c
        d = np.sqrt(p)
        S[c + 1:, c] = S[c + 1:, c] / d
        S[c, c] = d
        if c + 1 < b:
            S[c + 1:, c + 1:] -= np.tril(np.outer(S[c + 1:, c], S[c + 1:, c]))
    W = np.zeros_like(S)
    for r in range(b):
        s = np.zeros(b)
        for l in range(r):
            s = s + S[r, l] * W[l, :]
        W[r, :r] = -s[:r] / S[r, r]
        W[r, r] = 1.0 / S[r, r]
    return S, W


def inverse_blocked(G, nb):
    """G^-1 in float64 by the device's stages: (1) blocked Cholesky on the lower triangle with the inverted diagonal blocks
    kept, (2) M = L^-1 by block rows, (3) P = M^T M by block rows, (4) the upper triangle from the lower.  Raises
    ValueError naming the column at a pivot that is not positive and finite."""
    A = np.asarray(G, np.float64).copy()
    n = A.shape[0]
    W = {}
    for j in range(0, n, nb):
        e = min(j + nb, n)
        S, w = _diag_block(A[j:e, j:e])
        if S is None:
            raise ValueError("pivot of column %d" % (j + w))
        A[j:e, j:e] = S
        W[j] = w
        if e < n:
            A[e:, j:e] = A[e:, j:e] @ w.T
            A[e:, e:] -= A[e:, j:e] @ A[e:, j:e].T
    for j in range(0, n, nb):
        e = min(j + nb, n)
        if j:
            T = A[j:e, :j] @ np.tril(A[:j, :j])
            A[j:e, :j] = -(W[j] @ T)
        A[j:e, j:e] = W[j]
    for j in range(0, n, nb):
        e = min(j + nb, n)
        A[j:e, :e] = A[j:, j:e].T @ A[j:, :e]
    return np.tril(A) + np.tril(A, -1).T


def error_ratio(P, P_ld, cond):
    """max|P - P_ld| / (eps * cond2(G) * max|P_ld|)"""
    err = float(np.abs(np.asarray(P).astype(LD) - P_ld).max())
    return err / (EPS * cond * float(np.abs(P_ld).max()))
