"""PureSVD restated (csrc/puresvd.hip; the model is defined in include/tfrecomm.h): float64 NumPy in the kernels' order, with a
long double twin of the dense stages.

    spmm            k_psvd_spmm: out[row] = the rows in[id] of the row's list added one after the other from +0; a list of
                    more than ``chunk`` entries is added chunk by chunk, the chunks' sums then one after the other from +0.
                    Adds only: the device gives the same bits.
    gram            tests/ials_ref.gram_f64, not restated here: the device runs the ALS Gram launches.  That kernel contracts
                    ``acc += a * b`` into a fused multiply-add and the restatement rounds the product first, so the two agree
                    bit for bit exactly where the products are exact: the orthonormalise test's blocks hold float32 values
                    (24-bit significands: every product fits in 48 bits).  Elsewhere both stay inside ials_ref.gram_bound.
    chol / orth     k_psvd_chol's right-looking Cholesky, its column-by-column inverse, V = Z R^-1 with k ascending; any dtype
    jacobi / eig    k_psvd_jacobi: the circle-method rounds, rotations from T as a round finds it, rows then columns; any dtype
    fit             the whole algorithm from a start block

Bounds (eps = 2^-52).  Each constant is 8 times the largest ratio the float64 restatement shows against the long double one
over tests/puresvd_cases.py, measured by tests/test_puresvd_host.py, which asserts the figures below are the ones it finds:

    orth:  max|R1 - R1_ref| <= K eps cond2(S1) max|R1_ref|,   max|V - V_ref| <= K eps cond2(S1) max|V_ref|
           max|V^T V - I|   <= K_ORTH eps r
    eig:   max|lambda - lambda_ref|, max|T Qe - Qe diag(lambda)| <= K_EIG eps r max|lambda_ref|,  max|Qe^T Qe - I| <= K_EIG eps r
    fits:  the block case against its exact answer, |sigma^2 - a b|, |Q - Q_exact|, |P - P_exact| <= K_BLOCK[.] eps max|exact|;
           the random case, |sigma - sigma_ref| <= K_SIGMA eps sigma_1 (single factor columns are not compared: close Ritz
           values make them ill-conditioned); the wide case alike with K_SIGMA_WIDE
"""
import numpy as np

from tests import ials_ref
from tests.als_step_ref import EPS, LD

PIVOT_REL = 2.0 ** -44                                     # csrc/puresvd.h PSVD_PIVOT_REL
ROT_REL = 2.0 ** -52                                       # csrc/puresvd.h PSVD_ROT_REL
LD_EPS = float(np.finfo(LD).eps)

# MEASURED on the CPU by tests/test_puresvd_host.py (float64 restatement against the long double twin, or against the exact
# answer of the block case): orth 1.317 (case "one": a single column has cond 1, the error is the rounding of a 140-term
# sum), orthogonality 1.417 (Q = V Qe of the random fit), eigen step 1.353 (planted-127; over the sizes of
# tests/list_paths.py PSVD_EIG_SIZES the planted inputs give 1.283 at r = 4, 1.160 at 99, 0.954 at 100, 1.051 at 101, and T of
# the random fit 1.330; at most 11 sweeps); the block fit's sigma^2, Q, P: 4.867, 1.118, 2.0 eps of the largest exact entry;
# the random fit's sigma: 5.131 eps sigma_1; the wide fit's sigma (puresvd_cases.wide_case, r = 101): 31.959 eps sigma_1 -
# sigma_2 .. sigma_8 of a random pattern lie within 7 % of each other, so four iterations leave the Ritz values sensitive.
MEASURED_RHO_ORTH, MEASURED_RHO_ORTHOGONAL, MEASURED_RHO_EIG = 1.317, 1.417, 1.353
MEASURED_RHO_BLOCK = (4.867, 1.118, 2.0)
MEASURED_RHO_SIGMA = 5.131
MEASURED_RHO_SIGMA_WIDE = 31.959
K = int(np.ceil(8 * MEASURED_RHO_ORTH))
K_ORTH = int(np.ceil(8 * MEASURED_RHO_ORTHOGONAL))
K_EIG = int(np.ceil(8 * MEASURED_RHO_EIG))
K_BLOCK = tuple(int(np.ceil(8 * v)) for v in MEASURED_RHO_BLOCK)
K_SIGMA = int(np.ceil(8 * MEASURED_RHO_SIGMA))
K_SIGMA_WIDE = int(np.ceil(8 * MEASURED_RHO_SIGMA_WIDE))


class PivotError(ArithmeticError):
    def __init__(self, call, pass_, col):
        super().__init__("orthonormalisation %d, pass %d: the pivot of column %d is not positive and finite" % (call, pass_, col))
        self.call, self.pass_, self.col = call, pass_, col


class SweepCapError(ArithmeticError):
    pass


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def transpose_lists(indptr, items, n_users, n_items):
    """the item lists, users ascending (csrc/item_lists.h load_lists)"""
    rows = np.repeat(np.arange(n_users), np.diff(indptr))
    order = np.argsort(items, kind="stable")
    tptr = np.searchsorted(items[order], np.arange(n_items + 1)).astype(np.int64)
    return tptr, rows[order].astype(np.int32)


def _seq(rows):
    """+0 + rows[0] + rows[1] + ... one after the other"""
    return np.cumsum(np.concatenate((np.zeros((1,) + rows.shape[1:], rows.dtype), rows)), axis=0)[-1]


def spmm(ptr, ids, B, chunk, order="list"):
    """``order``: list (the kernel's), reversed (each list backwards) or unchunked (long lists in one run): the two wrong ones
    are what the host test plants"""
    B = np.asarray(B)
    out = np.zeros((ptr.size - 1, B.shape[1]), B.dtype)
    for e in range(ptr.size - 1):
        lst = ids[ptr[e]:ptr[e + 1]]
        if order == "reversed":
            lst = lst[::-1]
        if lst.size > chunk and order != "unchunked":
            out[e] = _seq(np.stack([_seq(B[lst[s:s + chunk]]) for s in range(0, lst.size, chunk)]))
        elif lst.size:
            out[e] = _seq(B[lst])
    return out


def gram(T, dtype=np.float64):
    return ials_ref.gram_f64(T) if dtype == np.float64 else ials_ref.gram(T)


def chol(S, dtype=np.float64, call=0, pass_=1):
    """(R, Rinv) upper, in k_psvd_chol's order"""
    r = S.shape[0]
    L = np.tril(np.asarray(S).astype(dtype))
    dg = np.diag(L).copy()
    for c in range(r):
        p = L[c, c]
        if not (p > 0 and p > dtype(PIVOT_REL) * dg[c]) or not np.isfinite(p):
            raise PivotError(call, pass_, c)
        d = np.sqrt(p)
        L[c + 1:, c] = L[c + 1:, c] / d
        L[c, c] = d
        L[c + 1:, c + 1:] -= np.tril(L[c + 1:, c][:, None] * L[c + 1:, c][None, :])
    R = L.T.copy()
    W = L.copy()
    for j in range(r - 1, -1, -1):
        dj = L[j, j]
        if j + 1 < r:                                      # W[i, k] is zero for k > i: running the sum to the end adds zeros
            s = np.cumsum(np.concatenate((np.zeros((r - j - 1, 1), dtype), W[j + 1:, j + 1:] * L[j + 1:, j][None, :]), axis=1), axis=1)[:, -1]
            W[j + 1:, j] = -s / dj
        W[j, j] = dtype(1) / dj
    return R, W.T.copy()


def matmul_seq(A, B):
    """A B with k ascending (k_ease_gemm walks k upwards)"""
    out = np.zeros((A.shape[0], B.shape[1]), A.dtype)
    for k in range(A.shape[1]):
        out += A[:, k][:, None] * B[k][None, :]
    return out


def orth(Z, dtype=np.float64, call=0):
    """(V, S [2, r, r], R [2, r, r]) of CholeskyQR twice"""
    V = np.asarray(Z).astype(dtype)
    S, R = [], []
    for p in range(2):
        s = gram(V.astype(np.float64), np.float64) if dtype == np.float64 else ials_ref.gram(V)
        Rp, Ri = chol(s, dtype, call, p + 1)
        V = matmul_seq(V, Ri)
        S.append(s)
        R.append(Rp)
    return V, np.stack(S), np.stack(R)


def rounds(r):
    """the pairs (p < q) of each round of a sweep, k_psvd_jacobi's order; an index r (odd r) sits out"""
    m = (r + 1) & ~1
    out = []
    for t in range(m - 1):
        pairs = []
        for k in range(m // 2):
            x, y = (t, m - 1) if k == 0 else ((t + k) % (m - 1), (t - k + m - 1) % (m - 1))
            p, q = min(x, y), max(x, y)
            if q < r:
                pairs.append((p, q))
        out.append(pairs)
    return out


def jacobi(T, dtype=np.float64, cap=30, rot_rel=None):
    """(lambda descending, Qe, sweeps): the sign and order rules of the kernel"""
    T = np.asarray(T).astype(dtype).copy()
    r = T.shape[0]
    Q = np.eye(r, dtype=dtype)
    rot_rel = (ROT_REL if dtype == np.float64 else LD_EPS) if rot_rel is None else rot_rel
    thr = dtype(rot_rel) * np.abs(T).max()
    plan = rounds(r)
    sweeps = 0
    while True:
        if sweeps == cap:
            raise SweepCapError("still rotating in sweep %d" % cap)
        sweeps += 1
        n_rot = 0
        for pairs in plan:
            if not pairs:
                continue
            P, Qx = np.array([p for p, _ in pairs]), np.array([q for _, q in pairs])
            apq = T[P, Qx]
            on = np.abs(apq) > thr
            if not on.any():
                continue
            P, Qx, apq = P[on], Qx[on], apq[on]
            n_rot += P.size
            theta = (T[Qx, Qx] - T[P, P]) / (2 * apq)
            tn = np.copysign(dtype(1), theta) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            c = 1 / np.sqrt(tn * tn + 1)
            s = tn * c
            x, y = T[P, :].copy(), T[Qx, :].copy()
            T[P, :], T[Qx, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
            x, y = T[:, P].copy(), T[:, Qx].copy()
            T[:, P], T[:, Qx] = c[None, :] * x - s[None, :] * y, s[None, :] * x + c[None, :] * y
            x, y = Q[:, P].copy(), Q[:, Qx].copy()
            Q[:, P], Q[:, Qx] = c[None, :] * x - s[None, :] * y, s[None, :] * x + c[None, :] * y
            T[P, Qx] = 0
            T[Qx, P] = 0
        if n_rot == 0:
            break
    lam = np.diag(T).copy()
    order = np.lexsort((np.arange(r), -lam))                # descending, equal values by column index
    lam, Q = lam[order], Q[:, order]
    at = np.abs(Q).argmax(0)                               # the first of equal magnitudes
    flip = Q[at, np.arange(r)] < 0
    Q = np.where(flip[None, :], -Q, Q) + 0                 # + 0: no negative zeros
    return lam, Q, sweeps


def fit(indptr, items, n_users, n_items, factors, oversample, iterations, V0, chunk, dtype=np.float64):
    """the whole algorithm; ``dtype`` long double gives the twin (its sums are in the same order, which no longer matters)"""
    tptr, tids = transpose_lists(indptr, items, n_users, n_items)
    V, _, _ = orth(V0, dtype, call=0)
    for it in range(iterations):
        W = spmm(indptr, items, V, chunk)
        V, _, _ = orth(spmm(tptr, tids, W, chunk), dtype, call=it + 1)
    W = spmm(indptr, items, V, chunk)
    T = gram(W, dtype)
    lam, Qe, sweeps = jacobi(T, dtype)
    Q = matmul_seq(V, Qe[:, :factors])
    return dict(sigma=np.sqrt(np.maximum(lam[:factors], 0)), ritz=lam, Q=Q, P=spmm(indptr, items, Q, chunk), T=T, V=V, sweeps=sweeps)


def residuals(indptr, items, n_users, n_items, Q, sigma, chunk):
    """the diagnostic from given factors: the two products are the kernel's bits, the column norms are in long double"""
    tptr, tids = transpose_lists(indptr, items, n_users, n_items)
    B = spmm(tptr, tids, spmm(indptr, items, Q, chunk), chunk)
    s2 = sigma * sigma
    d = B.astype(LD) - s2.astype(LD)[None, :] * Q.astype(LD)
    return (np.sqrt((d * d).sum(0)) / LD(s2[0])).astype(np.float64)


def residual_bound(n_items, ref, sigma):
    """k_psvd_resid adds ceil(I / 256) + 8 rounded squares per entry of its tree (relative error at most that many eps, half
    of it after the root), each difference B - s2 q carries one rounding of s2 q: at most eps s2_j |q_j| = eps s2_j in norm;
    the root and the division add two roundings.  Doubled."""
    s2 = sigma * sigma
    return 2 * (((-(-n_items // 256) + 8) / 2 + 2) * EPS * ref + EPS * s2 / s2[0])


# ----------------------------------------------------------------------------- ratios against the long double twin
def cond2(S):
    ev = np.linalg.eigvalsh(np.asarray(S, np.float64))
    return float(ev[-1] / ev[0])


def orth_ratios(Z, V, R1):
    """(rho, rho_orthogonal) of an orthonormalised V and first-pass factor R1 against the long double restatement of Z"""
    Vr, Sr, Rr = orth(Z, LD)
    c = cond2(Sr[0].astype(np.float64))
    eR = float(np.abs(R1.astype(LD) - Rr[0]).max() / np.abs(Rr[0]).max())
    eV = float(np.abs(V.astype(LD) - Vr).max() / np.abs(Vr).max())
    r = V.shape[1]
    o = float(np.abs(V.astype(LD).T @ V.astype(LD) - np.eye(r, dtype=LD)).max())
    return max(eR, eV) / (EPS * c), o / (EPS * r)


def eig_ratio(T, lam, Qe):
    """the largest of the three eigen-step errors in units of its bound without the constant"""
    r = T.shape[0]
    lam_ref, _, _ = jacobi(T, LD)
    scale = float(np.abs(lam_ref).max())
    if scale == 0:
        return 0.0 if not np.abs(lam).max() else np.inf
    Tl, Ql, ll = np.asarray(T).astype(LD), Qe.astype(LD), lam.astype(LD)
    e1 = float(np.abs(ll - lam_ref).max()) / scale
    e2 = float(np.abs(Tl @ Ql - Ql * ll[None, :]).max()) / scale
    e3 = float(np.abs(Ql.T @ Ql - np.eye(r, dtype=LD)).max())
    return max(e1, e2, e3) / (EPS * r)


def eig_rules(lam, Qe):
    """[] or what breaks the order and sign rules"""
    bad = []
    if not (np.diff(lam) <= 0).all():
        bad.append("eigenvalues are not descending")
    at = np.abs(Qe).argmax(0)
    if not (Qe[at, np.arange(Qe.shape[1])] > 0).all():
        bad.append("an eigenvector's largest entry is not positive")
    return bad
