"""EASE without a GPU: the NumPy restatement (tests/ease_ref.py) against values worked out by hand, the rank / top-K
equivalence, tfr_ease_plan's consistency and refusals (it is host-only), the argument errors that need no handle, and the
error constant of the inverse: how far the float64 restatement of the device's blocked order lands from the long double
inverse over the cases the GPU test runs, which bounds the device (tests/ease_cases.py error_constant).

tfr_ease_create refuses without a device after its argument checks, so everything that needs a handle is in
tests/test_gpu_ease.py (test_argument_and_state_errors)."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import ease as E
from tests import ease_cases as EC
from tests import ease_ref as R

F = np.float32
# 4 users x 3 items: users of item 0: {0, 1, 2}, of 1: {0, 1}, of 2: {2, 3}
ROWS = [[0, 1], [0, 1], [0, 2], [2]]
INDPTR = np.cumsum([0] + [len(r) for r in ROWS]).astype(np.int64)
ITEMS = np.concatenate(ROWS).astype(np.int32)


def test_ease_is_exported():
    assert T.EASE is E.EASE and "EASE" in T.__all__
    for name in ("load", "fit", "fit_gram", "gram", "inverse", "weights", "set_weights", "recommend", "recommend_lists",
                 "rank_items", "close"):
        assert callable(getattr(T.EASE, name))
    assert callable(E.plan)


def test_restatement_three_items_by_hand():
    g = R.gram(INDPTR, ITEMS, 4, 3, 1.0)
    assert g.tolist() == [[4, 2, 1], [2, 3, 0], [1, 0, 3]]                     # counts 3, 2, 2 plus lambda 1
    # det = 4 * 9 - 2 * 6 + 1 * (-3) = 21; adj = [[9, -6, -3], [-6, 11, 2], [-3, 2, 8]]
    want = np.array([[9, -6, -3], [-6, 11, 2], [-3, 2, 8]], np.float64) / 21.0
    for P in (R.inverse_ld(g).astype(np.float64), R.inverse_blocked(g, 2), R.inverse_blocked(g, 64)):
        assert np.allclose(P, want, rtol=1e-14, atol=0)
        assert np.array_equal(P, P.T)
    B = R.weights(want)
    assert B.dtype == np.float32
    assert B.tolist() == [[0, F(6 / 11), F(3 / 8)], [F(6 / 9), 0, F(-2 / 8)], [F(3 / 9), F(-2 / 11), 0]]
    got = R.user_scores([0, 2], B)                                             # items 0 then 2
    assert got.dtype == np.float32 and got.tolist() == [F(3 / 9), F(F(6 / 11) + F(-2 / 11)), F(3 / 8)]
    assert R.user_scores([], B).view(np.uint32).tolist() == [0, 0, 0]
    items, scores = R.topk(got, 3, excl=[0, 2])
    assert items.tolist() == [1, -1, -1] and scores.tolist() == [got[1], -np.inf, -np.inf]
    assert R.ranks(got, [0, 1, 2], excl=[2]).tolist() == [1, 0, -1]            # 4/11 = 0.364 beats 1/3


def test_restatement_four_items_by_hand():
    """two pairs of items that never meet: G is block diagonal, so are P and B, and the blocks are 2 x 2 inverses"""
    rows = [[0, 1], [0], [2, 3], [2, 3], [3]]
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    g = R.gram(indptr, np.concatenate(rows).astype(np.int32), 5, 4, 0.5)
    assert g.tolist() == [[2.5, 1, 0, 0], [1, 1.5, 0, 0], [0, 0, 2.5, 2], [0, 0, 2, 3.5]]
    P = R.inverse_blocked(g, 64)
    want = np.zeros((4, 4))
    want[:2, :2] = np.array([[1.5, -1], [-1, 2.5]]) / 2.75
    want[2:, 2:] = np.array([[3.5, -2], [-2, 2.5]]) / 4.75
    assert np.allclose(P, want, rtol=1e-14, atol=0) and not P[:2, 2:].any() and not P[2:, :2].any()
    B = R.weights(want)
    assert B[0, 1] == F(1 / 2.5) and B[1, 0] == F(1 / 1.5) and B[2, 3] == F(2 / 2.5) and B[3, 2] == F(2 / 3.5)
    assert not B[:2, 2:].any() and not B[2:, :2].any()
    assert R.user_scores([0, 1], B).tolist() == [F(1 / 1.5), F(1 / 2.5), 0, 0]


def test_restatement_refuses_an_indefinite_matrix():
    with pytest.raises(ValueError) as e:
        R.inverse_blocked(EC.indefinite_case(), EC.nb())
    assert "column 67" in str(e.value)
    assert np.linalg.eigvalsh(EC.indefinite_case()).min() < 0 and (np.diag(EC.indefinite_case()) > 0).all()


def test_restatement_rank_is_the_position_in_topk():
    """rank < k exactly when top-k returns the item, at that position: every k <= 12 on a 12-item catalogue, scores summed
    from weights with exact ties, and exclusions"""
    rs = np.random.RandomState(3)
    B = EC.constructed_weights(12)
    for trial in range(40):
        lst = np.sort(rs.choice(12, rs.randint(0, 6), replace=False))
        scores = R.user_scores(lst, B)
        excl = rs.choice(12, rs.randint(0, 5), replace=False)
        rk = R.ranks(scores, np.arange(12), excl)
        assert sorted(rk[rk >= 0].tolist()) == list(range(12 - excl.size))
        assert set(np.flatnonzero(rk < 0).tolist()) == set(excl.tolist())
        for k in range(1, 13):
            items, _ = R.topk(scores, k, excl)
            for t in range(12):
                assert (0 <= rk[t] < k) == (t in items.tolist())
                if 0 <= rk[t] < k:
                    assert items[rk[t]] == t


def test_plan_is_consistent():
    for n_items in (1, 2, 63, 64, 65, 1023, 1024, 1025, 3706, 16384, 16385, 32768):
        fit = E.plan(n_items)
        blocks = -(-n_items // fit["nb"])
        assert fit["nb"] >= 16 and fit["tile"] % 16 == 0 and fit["nb"] % fit["tile"] == 0
        assert fit["f64_bytes"] == 8 * (n_items * n_items + fit["nb"] * n_items + blocks * fit["nb"] ** 2)
        assert fit["f32_bytes"] == 4 * n_items * n_items
        assert fit["f64_bytes"] + fit["f32_bytes"] <= 12 * n_items * n_items + 16 * fit["nb"] * (n_items + fit["nb"])
        assert 0 < fit["lds"] <= 163840 and fit["lds"] >= 2 * 8 * fit["nb"] ** 2     # the diagonal block and its inverse
        assert fit["slices"] * fit["width"] >= n_items > (fit["slices"] - 1) * fit["width"]
        for k in (1, 10, 64, 65, 256):
            for n_rows in (0, 1, 3000, 70000, 10 ** 7):
                p = E.plan(n_items, k, n_rows, 1)                              # the cap is servable at every k
                assert (p["nb"], p["tile"], p["f64_bytes"]) == (fit["nb"], fit["tile"], fit["f64_bytes"])
                assert p["slices"] * p["width"] >= n_items > (p["slices"] - 1) * p["width"]
                assert p["slices"] * k <= 8192 and p["slices"] <= 256
                assert p["width"] % 64 == 0 and 0 < p["lds"] <= 163840
                assert p["chunk"] >= 1 and p["chunk"] * p["slices"] * k * 8 <= max(128 << 20, p["slices"] * k * 8)
                assert p["ahead"] >= 1


def test_plan_and_create_argument_errors():
    lib = L.load()
    none = (None,) * 9
    for bad in [(0, 10, 1, 0), (32769, 10, 1, 0), (32769, 10, 1, 1), (100, 0, 1, 0), (100, 257, 1, 0), (100, 0, 1, 1),
                (100, 257, 1, 1), (100, 10, -1, 1), (100, 10, 1, 2), (100, 10, 1, -1)]:
        assert lib.tfr_ease_plan(*bad, *none) == L.ERR_ARG, bad
    assert lib.tfr_ease_plan(32768, 256, 1, 1, *none) == L.OK
    with pytest.raises(T.TfrError) as e:
        E.plan(32769)
    assert e.value.code == L.ERR_ARG and "32768" in str(e.value)
    h = L._p()

    def create(n_users=10, n_items=10, lam=1.0, out=C.byref(h)):
        return lib.tfr_ease_create(out, n_users, n_items, lam, 0)
    assert create(n_items=32769) == L.ERR_ARG and b"32768" in lib.tfr_ease_last_error()      # before any device work
    assert create(n_users=0) == L.ERR_ARG and create(n_items=0) == L.ERR_ARG
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        assert create(lam=lam) == L.ERR_ARG
        assert b"lambda" in lib.tfr_ease_last_error()
    assert create(out=None) == L.ERR_ARG
    assert not h
    assert lib.tfr_ease_destroy(None) == L.OK
    for call in (lambda: lib.tfr_ease_load(None, None, None), lambda: lib.tfr_ease_gram(None),
                 lambda: lib.tfr_ease_set_gram(None, None), lambda: lib.tfr_ease_solve(None, 0, None),
                 lambda: lib.tfr_ease_get_f64(None, 0, 0, None), lambda: lib.tfr_ease_get_weights(None, 0, 0, None),
                 lambda: lib.tfr_ease_set_weights(None, 0, 0, None),
                 lambda: lib.tfr_ease_topk(None, None, 0, 1, None, None, None, None),
                 lambda: lib.tfr_ease_topk_lists(None, None, None, 0, 1, None, None, None, None),
                 lambda: lib.tfr_ease_rank_items(None, None, 0, None, None, None, None, None)):
        assert call() == L.ERR_ARG


def test_no_cpu_path():
    """without a HIP device a well-formed create is refused; with one it gives a handle"""
    if L.load().tfr_device_count() > 0:
        with T.EASE(10, 10) as m:
            assert m._h
        return
    with pytest.raises(T.TfrError) as e:
        T.EASE(10, 10)
    assert e.value.code == L.ERR_HIP and "no CPU path" in str(e.value)


def test_integer_cases_are_exact_in_the_restatement():
    """the condition the inputs of the GPU's exact-integer test must meet: the float64 restatement of the device's order
    returns (I - N)^T (I - N) bit for bit"""
    nb, tile = EC.nb(), EC.tile()
    for n, split in ((2 * nb + 3, nb + 6), (2 * tile + 1, tile - 7)):
        assert split % nb not in (0, nb - 1)                                   # the split is not on a block edge
        g, p = EC.integer_case(n, split)
        assert np.array_equal(g, g.T) and (np.diag(g) > 0).all() and np.array_equal(g, np.rint(g))
        assert np.array_equal(R.inverse_blocked(g, nb), p)


def test_the_error_constant_of_the_inverse():
    """r_max over the inverse cases, and K = 8 r_max, which tests/test_gpu_ease.py holds the device to.  The cases kept are
    those with cond2(G) <= 1e6; every lambda and every catalogue size keeps some."""
    cases = EC.inverse_cases()
    assert {lam for _, lam in cases} == set(EC.LAMBDAS)
    assert {name for name, _ in cases} == set(EC.gram_case_names())
    ratios = {}
    for name, lam in cases:
        g, p_ld, cond = EC.inverse_case(name, lam)
        assert cond <= EC.COND_MAX
        p = R.inverse_blocked(g, EC.nb())
        assert np.array_equal(p, p.T)
        ratios[(name, lam)] = R.error_ratio(p, p_ld, cond)
    r_max, K = EC.error_constant()
    worst = max(ratios, key=ratios.get)
    print("inverse cases: %d, cond2 up to %.3g, ratio from %.3g to r_max = %.3g at %s, K = %.3g" % (
        len(cases), max(EC.inverse_case(*c)[2] for c in cases), min(ratios.values()), r_max, worst, K))
    assert r_max == ratios[worst] and K == 8 * r_max
    assert 0 < r_max < 64                                                      # a backward-stable order: a small multiple of eps cond


def test_twin_case_gives_one_set_of_keys_in_both_restatements():
    """tests/test_gpu_ease.py holds the two devices' scoring tails against each other on this case: here the two restatements
    agree on it first, key for key, so a difference there is the device's"""
    from tests import itemknn_cases as IC, itemknn_ref as KR
    nb, sc, B = EC.twin_case()
    ni = B.shape[0]
    assert E.plan(ni, 10, 1, 1)["slices"] == 2 and not B.diagonal().any()
    indptr, items, nu, _ = EC.ladder(ni, seed=43)
    assert 0 in np.diff(indptr)                                                # a query with an empty list
    for lst in IC.rows_of(indptr, items, range(nu)):
        a, b = KR.user_scores(lst, nb, sc, ni), R.user_scores(lst, B)
        assert np.array_equal(KR.keys(a), R.keys(b))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
