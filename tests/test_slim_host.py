"""SLIM without a GPU: the NumPy restatement (tests/slim_ref.py) against a problem solved by hand, its two forms against each
other, tfr_slim_plan's consistency and refusals (it is host-only), the argument errors that need no handle, and - where
sklearn imports - the restatement against ``ElasticNet`` under the mapping of include/tfrecomm.h.

tfr_slim_create refuses without a device after its argument checks, so everything that needs a handle is in
tests/test_gpu_slim.py."""
import ctypes as C
import warnings

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import slim as S
from tests import slim_cases as SC
from tests import slim_ref as R
from tests.test_abi import declared_functions

# tests/test_ease_host.py's 4 users x 3 items with beta = 1: users of item 0: {0, 1, 2}, of 1: {0, 1}, of 2: {2, 3}
A3 = np.array([[4.0, 2.0, 1.0], [2.0, 3.0, 0.0], [1.0, 0.0, 3.0]])


def test_slim_is_exported_and_bound():
    assert T.SLIM is S.SLIM and "SLIM" in T.__all__
    for name in ("load", "fit", "fit_gram", "build_gram", "gram", "solve", "weights", "set_weights", "sweeps", "updates",
                 "converged", "recommend", "recommend_lists", "rank_items", "close"):
        assert callable(getattr(T.SLIM, name))
    assert callable(S.plan)
    names = [n for n in declared_functions() if n.startswith("tfr_slim_")]
    want = ["create", "destroy", "load", "last_error", "plan", "gram", "set_gram", "get_gram", "solve", "get_weights",
            "set_weights", "get_stats", "topk", "topk_lists", "rank_items"]
    assert sorted(names) == sorted("tfr_slim_" + w for w in want)
    lib = L.load()
    for n in names:
        assert hasattr(lib, n) and n in L.SIGNATURES


def test_restatement_two_free_coordinates_by_hand():
    """column 2 of A3: the free coordinates are 0 and 1, their block of A is [[4, 2], [2, 3]] (determinant 8), a = (1, 0)"""
    g = R.gram(np.array([0, 2, 4, 6, 7], np.int64), np.array([0, 1, 0, 1, 0, 2, 2], np.int32), 4, 3, 1.0)
    assert np.array_equal(g, A3)
    # positive, l1 = 1/4.  Sweep 1: i = 0: t = 1 - 1/4, wn = 3/16, q[1] = 0 - (3/16 * 2) = -3/8; i = 1: t < 0, wn = 0 = w[1].
    # Sweep 2 changes nothing: dmax = 0 stops it.  w = (3/16, 0): 4 w0 = 1 - l1, and q[1] - l1 < 0 keeps w1 at 0.
    w, sweeps, updates, conv = R.solve_column(A3, 2, 0.25, True, 100, 1e-4)
    assert w.tolist() == [0.1875, 0.0, 0.0] and (sweeps, updates, conv) == (2, 1, True)
    # signed, l1 = 1/4: 4 w0 + 2 w1 = 1 - 1/4 and 2 w0 + 3 w1 = 0 + 1/4 (w0 > 0 > w1): w0 = (9/4 - 1/2) / 8, w1 = (1 - 3/2) / 8
    w, sweeps, _, conv = R.solve_column(A3, 2, 0.25, False, 200, 0.0)
    assert conv and np.allclose(w, [0.21875, -0.0625, 0.0], rtol=1e-14, atol=0) and w[2] == 0
    # signed, l1 = 0: the plain solve [[4, 2], [2, 3]] w = (1, 0), w = (3, -2) / 8; positive: w1 is held at 0, w0 = 1/4
    w, _, _, conv = R.solve_column(A3, 2, 0.0, False, 200, 0.0)
    assert conv and np.allclose(w, [0.375, -0.25, 0.0], rtol=1e-14, atol=0)
    w, sweeps, updates, conv = R.solve_column(A3, 2, 0.0, True, 100, 1e-4)
    assert w.tolist() == [0.25, 0.0, 0.0] and (sweeps, updates, conv) == (2, 1, True)
    # signed, l1 = 0, stopped after one sweep: i = 0: wn = 1/4, q[1] = -1/2; i = 1: t = 1/2, wn = -(1/2) / 3
    w, sweeps, updates, conv = R.solve_column(A3, 2, 0.0, False, 1, 1e-4)
    assert w.tolist() == [0.25, -(0.5 / 3.0), 0.0] and (sweeps, updates, conv) == (1, 2, False)
    # l1 at the largest |a_ij|: nothing enters, in every column, and one sweep proves it
    for positive in (True, False):
        W, sweeps, updates, conv, W64 = R.solve(A3, 2.0, positive, 100, 1e-4)
        assert W.dtype == np.float32 and not W.view(np.uint32).any() and not W64.any()
        assert sweeps.tolist() == [1, 1, 1] and updates.tolist() == [0, 0, 0] and conv.all()
    # all columns at once: column 0 sees the blocks' complement [[3, 0], [0, 3]], a = (2, 1): w = (2 - l1, 1 - l1) / 3
    W, sweeps, updates, conv, W64 = R.solve(A3, 0.25, True, 100, 1e-4)
    assert W64[:, 0].tolist() == [0.0, 1.75 / 3.0, 0.75 / 3.0] and W64[:, 2].tolist() == [0.1875, 0.0, 0.0]
    assert W[:, 0].tolist() == [0.0, np.float32(1.75 / 3.0), np.float32(0.75 / 3.0)] and not np.diag(W).any()
    assert R.to_f32(np.array([-0.0, 0.5])).view(np.uint32).tolist() == [0, 0x3f000000]      # a zero weight is stored as +0


def test_the_two_forms_of_the_restatement_agree():
    """solve (all columns at once) against solve_column (the pseudo-code, line for line): weights bit for bit, sweeps,
    updates, converged - with an item nobody has, an item everybody has, duplicate columns, both signs, stopped early"""
    for name in ("size:2", "full_user", "duplicates"):
        for l1, beta in SC.PENALTIES:
            for positive, max_iter, tol in ((True, 10, 1e-4), (False, 10, 1e-4), (True, 2, 0.0)):
                A = SC.gram(name, beta)
                W, sweeps, updates, conv, W64 = R.solve(A, l1, positive, max_iter, tol)
                assert np.array_equal(W.view(np.uint32), R.to_f32(W64).view(np.uint32))
                for j in range(A.shape[0]):
                    w, s, u, c = R.solve_column(A, j, l1, positive, max_iter, tol)
                    assert np.array_equal(w.view(np.uint64), W64[:, j].view(np.uint64)), (name, l1, beta, positive, j)
                    assert (s, u, c) == (sweeps[j], updates[j], conv[j]), (name, l1, beta, positive, j)
    A = SC.gram("lengths", 0.0)
    assert A[0, 0] == 0 and not A[0].any()                                     # nobody has item 0 and beta = 0: d = 0
    W = R.solve(A, 0.0, False, 5, 1e-4)[0]
    assert not W[0].any() and not W[:, 0].any()


def test_kkt_excess_is_zero_at_a_solution_and_not_beside_it():
    W = np.zeros((3, 3))
    W[:, 2] = [0.1875, 0.0, 0.0]
    W[:, 0] = [0.0, 1.75 / 3.0, 0.75 / 3.0]
    W[:, 1] = R.solve_column(A3, 1, 0.25, True, 500, 0.0)[0]
    ex, r = R.kkt_excess(A3, W, 0.25, True)
    assert ex.dtype == np.longdouble and float(ex.max()) < 1e-15
    assert float(r[1, 2]) == -0.375                                            # a_12 - A[1, 0] w0 = 0 - 2 * 3/16
    W[0, 2] = 0.25
    ex, _ = R.kkt_excess(A3, W, 0.25, True)
    assert float(ex[0, 2]) == 0.25                                             # |1 - 1/4 - 4 * 1/4|


def test_plan_is_consistent():
    for n_items in (1, 2, 255, 256, 257, 1024, 2048, 2049, 3706, 8192, 16384):
        p = S.plan(n_items)
        assert p["window"] % 64 == 0 and 64 <= p["window"] <= 1024
        assert 1 <= p["grid"] <= n_items
        assert p["grid"] == n_items or p["grid"] % 256 == 0                    # whole compute units' worth of workgroups
        q_bytes = 8 * n_items * (1 if not p["w_in_lds"] else 2)
        assert q_bytes <= p["lds"] <= 163840
        scratch = 0 if p["w_in_lds"] else p["grid"] * n_items
        assert p["f64_bytes"] == 8 * (n_items * n_items + n_items + scratch)
        assert p["f32_bytes"] == 4 * n_items * n_items
        for k in (1, 10, 256):
            s = S.plan(n_items, k, 3000, 1)
            e = T.ease.plan(n_items, k, 3000, 1)
            assert {x: s[x] for x in ("width", "slices", "chunk", "ahead", "lds")} == {x: e[x] for x in ("width", "slices", "chunk", "ahead", "lds")}
    assert SC.stride_items() - 2 > S.plan(SC.stride_items())["grid"]


def test_plan_and_create_argument_errors():
    lib = L.load()
    none = (None,) * 10
    for bad in [(0, 10, 1, 0), (16385, 10, 1, 0), (16385, 10, 1, 1), (100, 0, 1, 0), (100, 257, 1, 1), (100, 10, -1, 1),
                (100, 10, 1, 2), (100, 10, 1, -1)]:
        assert lib.tfr_slim_plan(*bad, *none) == L.ERR_ARG, bad
    assert lib.tfr_slim_plan(16384, 256, 1, 1, *none) == L.OK and lib.tfr_slim_plan(16384, 1, 0, 0, *none) == L.OK
    with pytest.raises(T.TfrError) as e:
        S.plan(16385)
    assert e.value.code == L.ERR_ARG and "16384" in str(e.value)
    h = L._p()

    def create(n_users=10, n_items=10, beta=1.0, out=C.byref(h)):
        return lib.tfr_slim_create(out, n_users, n_items, beta, 0)
    assert create(n_items=16385) == L.ERR_ARG and b"16384" in lib.tfr_slim_last_error()      # before any device work
    assert create(n_users=0) == L.ERR_ARG and create(n_items=0) == L.ERR_ARG
    for beta in (-1.0, float("nan"), float("inf")):
        assert create(beta=beta) == L.ERR_ARG
        assert b"beta" in lib.tfr_slim_last_error()
    assert create(out=None) == L.ERR_ARG
    assert not h
    assert lib.tfr_slim_destroy(None) == L.OK
    for call in (lambda: lib.tfr_slim_load(None, None, None), lambda: lib.tfr_slim_gram(None),
                 lambda: lib.tfr_slim_set_gram(None, None), lambda: lib.tfr_slim_get_gram(None, 0, 0, None),
                 lambda: lib.tfr_slim_solve(None, 1.0, 1, 10, 1e-4, None), lambda: lib.tfr_slim_get_stats(None, None, None, None),
                 lambda: lib.tfr_slim_get_weights(None, 0, 0, None), lambda: lib.tfr_slim_set_weights(None, 0, 0, None),
                 lambda: lib.tfr_slim_topk(None, None, 0, 1, None, None, None, None),
                 lambda: lib.tfr_slim_topk_lists(None, None, None, 0, 1, None, None, None, None),
                 lambda: lib.tfr_slim_rank_items(None, None, 0, None, None, None, None, None)):
        assert call() == L.ERR_ARG


def test_no_cpu_path():
    """without a HIP device a well-formed create is refused; with one it gives a handle"""
    if L.load().tfr_device_count() > 0:
        with T.SLIM(10, 10) as m:
            assert m._h
        return
    with pytest.raises(T.TfrError) as e:
        T.SLIM(10, 10)
    assert e.value.code == L.ERR_HIP and "no CPU path" in str(e.value)


def test_restatement_agrees_with_sklearn_elastic_net():
    """ElasticNet(alpha, l1_ratio, positive=True) on (X with column j zeroed, y = column j of X) minimises, times the U users,
    F(w) = 1/2 |y - X w|^2 + U alpha l1_ratio |w|_1 + 1/2 U alpha (1 - l1_ratio) |w|^2 = 1/2 w^T A w - a_j^T w + l1 |w|_1 + const
    with l1 = U alpha l1_ratio, beta = U alpha (1 - l1_ratio), A = X^T X + beta I: the header's problem for column j.
    F is strongly convex with modulus mu = the smallest eigenvalue of A (>= beta).

    sklearn stops at a duality gap below tol_sk * |y|^2 (in this F: cd_fast scales alpha and beta by U), so
    F(w_sk) - F* <= tol_sk |y|^2 and, by strong convexity, |w_sk - w*|_2 <= sqrt(2 tol_sk |y|^2 / mu).

    The restatement stops after a sweep whose largest change is dmax <= tol max|w|.  Coordinate i was exactly optimal for
    the q[i] it saw; the coordinates after it then moved q[i] by at most delta_i = dmax * sum over k != i of |A[i, k]|.  So w
    is the exact minimiser of F with a_j shifted by some delta, and minimisers of strongly convex problems that differ by a
    linear term delta lie within |delta|_2 / mu: |w - w*|_2 <= tol max|w| |rowsum|_2 / mu.  (Float64 rounding, about
    updates * eps * max|A|, is far below both at these tolerances and gets a 1e-12 allowance.)

    Every weight is therefore within the sum of the two of sklearn's."""
    linear_model = pytest.importorskip("sklearn.linear_model")
    from sklearn.exceptions import ConvergenceWarning
    (indptr, items, nu, ni), _, _ = SC.planted_case()
    X = np.zeros((nu, ni))
    for u in range(nu):
        X[u, items[indptr[u]:indptr[u + 1]]] = 1.0
    tol, tol_sk = 1e-8, 1e-10
    worst = 0.0
    for l1, beta in ((1.0, 5.0), (0.5, 1.0)):
        A = SC.planted_gram(beta)
        assert np.array_equal(A, X.T @ X + beta * np.eye(ni))
        W, sweeps, updates, conv, W64 = R.solve(A, l1, True, 2000, tol)
        assert conv.all()
        mu = float(np.linalg.eigvalsh(A).min())
        assert mu >= beta * (1 - 1e-9)
        rowsum = np.abs(A).sum(axis=1) - np.abs(np.diag(A))
        alpha, l1_ratio = (l1 + beta) / nu, l1 / (l1 + beta)
        for j in range(ni):
            y = X[:, j]
            assert y.any()
            Xj = X.copy()
            Xj[:, j] = 0.0
            with warnings.catch_warnings():
                warnings.simplefilter("error", ConvergenceWarning)
                en = linear_model.ElasticNet(alpha=alpha, l1_ratio=l1_ratio, positive=True, fit_intercept=False, tol=tol_sk,
                                             max_iter=100000).fit(Xj, y)
            w = W64[:, j]
            bound = tol * np.abs(w).max() * float(np.linalg.norm(rowsum)) / mu + np.sqrt(2 * tol_sk * float(y @ y) / mu) + 1e-12
            err = float(np.abs(en.coef_ - w).max())
            worst = max(worst, err / bound)
            assert err <= bound, (l1, beta, j, err, bound)
            assert en.coef_[j] == 0 and w[j] == 0
    print("restatement against ElasticNet: largest |difference| / bound = %.3g" % worst)
