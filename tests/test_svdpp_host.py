"""SVD++ without a device: the float64 restatement (tests/svdpp_ref.py) against finite differences and against the SVD
oracle (Y = 0 and frozen gives exactly the SVD step), and the host checks of the implicit sets that run before any device
call (tfrecomm_amd.svdpp.implicit_csr)."""
import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from oracle import svd_oracle as so
from tests import svdpp_ref as R


def _problem(seed=0, U=7, I=9, D=4, B=12, full_user=True):
    rs = np.random.RandomState(seed)
    rows = []
    for u in range(U):
        if u == 0:
            rows.append(np.zeros(0, np.int64))                 # empty N(u)
        elif u == 1 and full_user:
            rows.append(np.arange(I))                          # N(u) holds every item
        else:
            rows.append(np.sort(rs.choice(I, rs.randint(1, I), replace=False)))
    indptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    items = np.concatenate(rows).astype(np.int64)
    t = {R.MU: np.array(rs.normal(0, .5)), R.BU: rs.normal(0, .5, U), R.BI: rs.normal(0, .5, I),
         R.PF: rs.normal(0, .4, (U, D)), R.QF: rs.normal(0, .4, (I, D)), R.YF: rs.normal(0, .4, (I, D))}
    u = np.concatenate(([0, 1, 1], rs.randint(0, U, B - 3)))
    i = rs.randint(0, I, B)
    return t, indptr, items, u, i, rs


@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("item_abs", [False, True])
@pytest.mark.parametrize("reg_bias", [False, True])
def test_gradients_match_finite_differences(loss, item_abs, reg_bias):
    t, indptr, items, u, i, rs = _problem(seed=3 + 2 * item_abs + reg_bias)
    r = rs.randint(0, 2, u.size).astype(np.float64) if loss == "nll" else rs.randint(1, 6, u.size).astype(np.float64)
    lam = 0.07
    G = R.gradients(t, indptr, items, u, i, r, loss, item_abs, reg_bias, lam)
    h = 1e-6
    for tid, tab in t.items():
        flat = tab.reshape(-1)
        idx = range(flat.size) if flat.size <= 40 else rs.choice(flat.size, 40, replace=False)
        for x in idx:
            old = flat[x]
            flat[x] = old + h
            cp = R.cost(t, indptr, items, u, i, r, loss, item_abs, reg_bias, lam)
            flat[x] = old - h
            cm = R.cost(t, indptr, items, u, i, r, loss, item_abs, reg_bias, lam)
            flat[x] = old
            fd = (cp - cm) / (2 * h)
            an = G[tid].reshape(-1)[x]
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd)), (tid, x, fd, an)


def test_y_gradient_per_user_form_equals_per_occurrence_sum():
    t, indptr, items, u, i, rs = _problem(seed=11)
    r = rs.randint(1, 6, u.size).astype(np.float64)
    lam = 0.05
    g = so.dlogits(R.forward(t, indptr, items, u, i), r)
    z, s, _ = R.implicit_parts(t[R.YF], indptr, items, u)
    want = np.zeros_like(t[R.YF])
    for k in range(u.size):                                # dY[j] += g_k s_u Q[i_k] + lam Y[j], one occurrence at a time
        for j in items[indptr[u[k]]:indptr[u[k] + 1]]:
            want[j] += g[k] * s[k] * t[R.QF][i[k]] + lam * t[R.YF][j]
    got = R.gradients(t, indptr, items, u, i, r, "mse", False, False, lam)[R.YF]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("loss,item_abs,reg_bias", [("mse", False, False), ("nll", True, True)])
def test_zero_frozen_y_is_exactly_the_svd_step(optimizer, loss, item_abs, reg_bias):
    t, indptr, items, u, i, rs = _problem(seed=5)
    U, I, D = t[R.PF].shape[0], t[R.QF].shape[0], t[R.PF].shape[1]
    r = rs.randint(0, 2, u.size).astype(np.float64) if loss == "nll" else rs.randint(1, 6, u.size).astype(np.float64)
    t[R.YF][...] = 0.0
    ref = R.SvdppRef(U, I, D, indptr, items, loss=loss, item_abs=item_abs, reg_bias=reg_bias, optimizer=optimizer,
                     lr=0.01, reg=0.05)
    ref.set_tables(t)
    ref.frozen = 1 << R.YF
    orc = so.SvdOracle(U, I, D, loss=loss, item_abs=item_abs, reg_bias=reg_bias, optimizer=optimizer,
                       adam_mode=so.LAZY, lr=0.01, reg=0.05)
    orc.set_tables(t[R.MU], t[R.BU], t[R.BI], t[R.PF], t[R.QF])
    for _ in range(3):
        a = ref.train_step(u, i, r)
        b = orc.train_step(u, i, r)
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2]
    for tid, want in ((R.MU, orc.mu), (R.BU, orc.bu), (R.BI, orc.bi), (R.PF, orc.P), (R.QF, orc.Q)):
        np.testing.assert_array_equal(ref.t[tid], want)
    assert not ref.t[R.YF].any()


# ---- implicit_csr: the checks set_implicit runs before any device call ----------------------------------------------
def test_implicit_csr_accepts_pairs_and_sparse():
    ip, it = T.svdpp.implicit_csr((np.array([0, 2, 2, 3]), np.array([1, 4, 0])), 3, 5)
    assert ip.dtype == np.int64 and it.dtype == np.int32
    assert ip.tolist() == [0, 2, 2, 3] and it.tolist() == [1, 4, 0]
    x = T.rated_matrix([2, 0, 0, 0], [0, 4, 1, 4], 3, 5)      # repeats merged, rows sorted
    ip, it = T.svdpp.implicit_csr(x, 3, 5)
    assert ip.tolist() == [0, 2, 2, 3] and it.tolist() == [1, 4, 0]
    ip, it = T.svdpp.implicit_csr(sp.csr_matrix((3, 5), dtype=np.float32), 3, 5)
    assert ip.tolist() == [0, 0, 0, 0] and it.size == 0


@pytest.mark.parametrize("items", [[4, 1, 0], [1, 1, 0]])
def test_implicit_csr_rejects_unsorted_or_repeated_rows(items):
    with pytest.raises(ValueError):
        T.svdpp.implicit_csr((np.array([0, 2, 2, 3]), np.array(items)), 3, 5)


@pytest.mark.parametrize("items", [[1, 5, 0], [-1, 2, 0]])
def test_implicit_csr_rejects_ids_out_of_range(items):
    with pytest.raises(T.OutOfRangeError):
        T.svdpp.implicit_csr((np.array([0, 2, 2, 3]), np.array(items)), 3, 5)


@pytest.mark.parametrize("indptr", [[0, 2, 3], [0, 2, 2, 3, 3], [1, 2, 2, 3], [0, 2, 1, 3], [0, 2, 2, 4]])
def test_implicit_csr_rejects_a_bad_indptr(indptr):
    with pytest.raises(ValueError):
        T.svdpp.implicit_csr((np.array(indptr), np.array([1, 4, 0])), 3, 5)


def test_implicit_csr_rejects_a_sparse_matrix_of_the_wrong_shape():
    with pytest.raises(ValueError):
        T.svdpp.implicit_csr(sp.csr_matrix((3, 6), dtype=np.float32), 3, 5)


def test_svdpp_model_is_exported():
    assert T.SvdppModel is T.svdpp.SvdppModel
    assert T._lib.Y == 5
