"""UserKNN without a GPU: the NumPy restatement (tests/userknn_ref.py) against ItemKNN's on the transposed matrix and against
a dense float64 formula, the launch plan (tfr_uknn_plan is host-only), the argument errors that need no handle, the export.

tfr_uknn_create refuses without a device after its argument checks, so everything that needs a handle is in
tests/test_gpu_userknn.py (test_argument_and_state_errors)."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import userknn as UK
from tests import itemknn_ref as IR
from tests import userknn_cases as UC
from tests import userknn_ref as R

METRICS = [("cosine", 0.0), ("cosine", 2.5), ("jaccard", 0.0), ("jaccard", 2.5), ("count", 0.0)]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_userknn_is_exported():
    assert T.UserKNN is UK.UserKNN and "UserKNN" in T.__all__ and UK.UserKNN._family == "uknn"
    for name in ("load", "fit", "neighbours", "set_neighbours", "similar_users", "recommend", "recommend_lists", "rank_items"):
        assert callable(getattr(T.UserKNN, name))
    assert callable(UK.plan)


@pytest.mark.parametrize("metric,shrink", METRICS)
def test_restatement_neighbours_are_itemknn_of_the_transpose(metric, shrink):
    for name in ("lengths", "sparse_lengths", "ties"):
        indptr, items, nu, ni = UC.case(name)
        tp, ti, tnu, tni = UC.transpose((indptr, items, nu, ni))
        assert (tnu, tni) == (ni, nu)
        for K in (1, 10, 256):
            nb, sc = R.fit(indptr, items, nu, ni, K, metric, shrink)
            wnb, wsc = IR.fit(*IR.cooccurrence(tp, ti, tnu, tni), K, metric, shrink)
            assert np.array_equal(nb, wnb) and np.array_equal(bits(sc), bits(wsc)), (name, K)


def test_restatement_by_hand():
    # 4 users x 5 items: rows {0,1}, {0,1,2}, {2}, {3,4}
    rows = [[0, 1], [0, 1, 2], [2], [3, 4]]
    indptr, items, nu, ni = UC.csr_of_rows(rows, 5)
    c, d = R.cooccurrence(indptr, items, nu, ni)
    assert d.tolist() == [2, 3, 1, 2] and c.toarray().tolist() == [[2, 2, 0, 0], [2, 3, 1, 0], [0, 1, 1, 0], [0, 0, 0, 2]]
    nb, sc = R.fit(indptr, items, nu, ni, 2, "cosine", 0.0)
    s01, s12 = F(2 / np.sqrt(6.0)), F(1 / np.sqrt(3.0))
    assert nb.tolist() == [[1, -1], [0, 2], [1, -1], [-1, -1]]
    assert bits(sc).tolist() == bits(np.array([[s01, -np.inf], [s01, s12], [s12, -np.inf], [-np.inf, -np.inf]], F)).tolist()
    got = R.user_scores(nb[1], sc[1], indptr, items, ni)                      # user 0's items at s01, then user 2's at s12
    assert got.dtype == np.float32 and got.tolist() == [s01, s01, s12, 0, 0]
    assert R.user_scores(nb[3], sc[3], indptr, items, ni).tolist() == [0] * 5
    # a list equal to row 1 finds user 1 first at exactly 1, itself not left out; a list nobody shares finds nobody
    lnb, lsc = R.list_neighbours([0, 1, 2], indptr, items, nu, ni, 3, "cosine", 0.0)
    assert lnb.tolist() == [1, 0, 2] and bits(lsc).tolist() == bits(np.array([1.0, s01, s12], F)).tolist()
    lnb, lsc = R.list_neighbours([], indptr, items, nu, ni, 2, "cosine", 0.0)
    assert lnb.tolist() == [-1, -1] and np.isneginf(lsc).all()
    lnb, lsc = R.list_neighbours([3], indptr, items, nu, ni, 2, "jaccard", 1.0)
    assert lnb.tolist() == [3, -1] and lsc[0] == F(1 / (2.0 + 1.0))             # c 1, |L| 1, d_3 2: 1 / (1 + 2 - 1 + 1)


@pytest.mark.parametrize("metric,shrink", METRICS)
def test_restatement_scores_agree_with_a_dense_formula(metric, shrink):
    """score(u, .) = sum over kept neighbours of s(u, v) X[v, .]: the float32 chain of at most K terms is within
    K * 2^-24 * sum |terms| of the float64 sum (each of the K - 1 adds rounds once, relative 2^-24 of a partial sum that the
    sum of magnitudes bounds)"""
    indptr, items, nu, ni = UC.case("lengths")
    x = IR.pattern(indptr, items, nu, ni).toarray().astype(np.float64)
    K = 20
    nb, sc = R.fit(indptr, items, nu, ni, K, metric, shrink)
    for u in range(nu):
        kept = nb[u] >= 0
        s = sc[u][kept].astype(np.float64)
        want = s @ x[nb[u][kept]]
        mag = np.abs(s) @ x[nb[u][kept]]
        got = R.user_scores(nb[u], sc[u], indptr, items, ni).astype(np.float64)
        assert (np.abs(got - want) <= K * 2.0 ** -24 * mag).all(), u
        assert (got[mag == 0] == 0).all()


def test_restatement_constructed_order_matters():
    """the constructed row 8 is there so that another order of the adds changes the bits"""
    indptr, items, nu, ni = UC.case("scoring")
    for K in (7, 64, 256):
        nb, sc = UC.constructed_lists(nu, K)
        fwd = R.user_scores(nb[8], sc[8], indptr, items, ni)
        back = R.user_scores(nb[8][::-1], sc[8][::-1], indptr, items, ni)
        assert K < 64 or bits(fwd)[6] != bits(back)[6]
        assert R.user_scores(nb[7], sc[7], indptr, items, ni)[6] == 0.0         # (1 + 1e8) - 1e8 in float32
        assert R.user_scores(nb[7][::-1], sc[7][::-1], indptr, items, ni)[6] == 1.0
        assert (R.user_scores(nb[9], sc[9], indptr, items, ni) == 0).all()
        for v in nb[8][nb[8] >= 0][:5]:
            assert 6 in items[indptr[v]:indptr[v + 1]]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_plan_is_consistent(which):
    width = 8192 if which == 1 else 16384
    for n_cols in (1, 100, 8191, 8192, 8193, 16383, 16384, 16385, 32771, 70000, 262144, 500000):
        for k in (1, 10, 50, 64, 65, 192, 193, 256):
            for n_rows in (0, 1, 3000, 70000, 10 ** 7):
                try:
                    p = UK.plan(n_cols, k, n_rows, which)
                except T.TfrError as e:
                    assert e.code == L.ERR_ARG
                    assert -(-n_cols // width) * k > 8192 or -(-n_cols // width) > 256        # refused only past the merge
                    continue
                assert p["width"] == width
                assert p["slices"] * p["width"] >= n_cols > (p["slices"] - 1) * p["width"]
                assert p["slices"] * k <= 8192 and p["slices"] <= 256
                assert 0 < p["lds"] <= 163840
                assert p["chunk"] >= 1 and p["chunk"] * p["slices"] * k * 8 <= max(128 << 20, p["slices"] * k * 8)
                assert p["ahead"] == 64
    assert UK.plan(70000, 10, 70000, 0)["chunk"] < 70000                       # the 70 000-user case takes two row chunks
    assert UK.plan(70000, 10, 70000, 0)["slices"] == 5
    assert (UC.w_fit(), UC.w_score(), UC.w_lists()) == (16384, 8192, 16384)


def test_plan_and_create_argument_errors():
    lib = L.load()
    for bad in [(0, 10, 1, 0), (100, 0, 1, 0), (100, 257, 1, 1), (100, 10, -1, 0), (100, 10, 1, 3), (100, 10, 1, -1), (2 ** 31, 10, 1, 0),
                (16384 * 32 + 1, 256, 1, 0), (16384 * 32 + 1, 256, 1, 2), (8192 * 32 + 1, 256, 1, 1)]:
        assert lib.tfr_uknn_plan(*bad, None, None, None, None, None) == L.ERR_ARG, bad
        assert lib.tfr_uknn_last_error().startswith(b"uknn plan")
    for which in (0, 1, 2):
        assert lib.tfr_uknn_plan(100, 10, 1, which, None, None, None, None, None) == L.OK
    assert lib.tfr_uknn_plan(16384 * 32, 256, 1, 0, None, None, None, None, None) == L.OK
    with pytest.raises(T.TfrError):
        UK.plan(100, 10, 1, 3)
    h = L._p()

    def create(n_users=10, n_items=10, K=5, metric=0, shrink=0.0, out=C.byref(h)):
        return lib.tfr_uknn_create(out, n_users, n_items, K, metric, shrink, 0)
    before = lib.tfr_knn_last_error()
    assert create(K=0) == L.ERR_ARG and b"k must be" in lib.tfr_uknn_last_error()
    assert create(K=257) == L.ERR_ARG
    assert create(metric=3) == L.ERR_ARG and create(metric=-1) == L.ERR_ARG
    assert b"metric" in lib.tfr_uknn_last_error()
    assert create(shrink=-0.5) == L.ERR_ARG
    assert create(shrink=float("nan")) == L.ERR_ARG
    assert create(shrink=float("inf")) == L.ERR_ARG
    assert b"shrink" in lib.tfr_uknn_last_error()
    assert create(metric=2, shrink=1.0) == L.ERR_ARG
    assert create(n_users=0) == L.ERR_ARG and create(n_items=0) == L.ERR_ARG
    assert create(n_users=16384 * 32 + 1, K=256) == L.ERR_ARG                    # 33 slices of 256 keys: past the merge
    assert b"users" in lib.tfr_uknn_last_error()
    assert create(n_users=16384 * 163 + 1, K=50) == L.ERR_ARG                    # 164 slices of 50 keys
    assert create(out=None) == L.ERR_ARG
    assert not h
    assert lib.tfr_knn_last_error() == before                                  # a text of its own
    assert lib.tfr_uknn_destroy(None) == L.OK
    for call in (lambda: lib.tfr_uknn_fit(None, None), lambda: lib.tfr_uknn_load(None, None, None),
                 lambda: lib.tfr_uknn_get_neighbours(None, 0, 0, None, None), lambda: lib.tfr_uknn_set_neighbours(None, 0, 0, None, None),
                 lambda: lib.tfr_uknn_topk(None, None, 0, 1, None, None, None, None),
                 lambda: lib.tfr_uknn_topk_lists(None, None, None, 0, 1, None, None, None, None),
                 lambda: lib.tfr_uknn_rank_items(None, None, 0, None, None, None, None, None)):
        assert call() == L.ERR_ARG
    with pytest.raises(ValueError):
        T.UserKNN(10, 10, metric="dice")


def test_no_cpu_path():
    """without a HIP device a well-formed create is refused; with one it gives a handle"""
    if L.load().tfr_device_count() > 0:
        with T.UserKNN(10, 10) as m:
            assert m._h
        return
    with pytest.raises(T.TfrError) as e:
        T.UserKNN(10, 10)
    assert e.value.code == L.ERR_HIP and "no CPU path" in str(e.value)
