"""The weighted fit and RP3beta without a GPU: the NumPy restatement (tests/rp3_ref.py) against sums, scales and lists worked
out by hand, its derived distance to the unrounded float64 model, P3alpha at beta = 0, the choice of the shift, the plan's
consistency (tfr_knn_weighted_plan is host-only), the argument errors that need no handle, and the export.

tfr_knn_create refuses without a device, so every check of tfr_knn_fit_weighted past the NULL handle is in
tests/test_gpu_rp3.py."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import rp3beta as RP
from tests import itemknn_ref as R
from tests import rp3_ref as R3

# 4 users x 5 items: users of item 0: {0,1,2}, of 1: {0,1,3}, of 2: {1,2}, of 3: {3}, of 4: nobody
ROWS = [[0, 1], [0, 1, 2], [0, 2], [1, 3]]
INDPTR = np.cumsum([0] + [len(r) for r in ROWS]).astype(np.int64)
ITEMS = np.concatenate(ROWS).astype(np.int32)
F, D = np.float32, np.float64


def test_classes_are_exported():
    assert T.RP3beta is RP.RP3beta and T.WeightedItemKNN is RP.WeightedItemKNN
    assert "RP3beta" in T.__all__ and "WeightedItemKNN" in T.__all__
    assert issubclass(T.RP3beta, T.WeightedItemKNN) and issubclass(T.WeightedItemKNN, T.ItemKNN)
    for name in ("fit", "neighbours", "set_neighbours", "similar_items", "recommend", "recommend_lists", "rank_items"):
        assert callable(getattr(T.RP3beta, name))
    for name in ("neighbours", "set_neighbours", "similar_items", "recommend", "recommend_lists", "rank_items"):
        assert getattr(T.RP3beta, name) is getattr(T.ItemKNN, name)          # inherited, not restated


def test_restatement_by_hand():
    """alpha 1, beta 0.5 at shift 4: w = 1/2, 1/3, 1/2, 1/2 -> q = 8, 5 (5.33 rounds down), 8, 8"""
    q, rs, cs, shift = R3.rp3_terms(INDPTR, ITEMS, 4, 5, 1.0, 0.5, shift=4)
    assert q.dtype == np.uint64 and q.tolist() == [8, 5, 8, 8] and shift == 4
    assert rs.dtype == cs.dtype == np.float64
    assert np.allclose(rs, [1 / 3, 1 / 3, 0.5, 1.0, 0.0], rtol=1e-15, atol=0)
    assert np.allclose(cs, [3 ** -0.5, 3 ** -0.5, 2 ** -0.5, 1.0, 0.0], rtol=1e-15, atol=0)
    s = R3.weighted_sums(INDPTR, ITEMS, 4, 5, q)
    assert s.dtype == np.int64
    assert s.toarray().tolist() == [[21, 13, 13, 0, 0], [13, 21, 5, 8, 0], [13, 5, 13, 0, 0], [0, 8, 0, 8, 0], [0, 0, 0, 0, 0]]
    nb, sc = R3.fit(s, rs, cs, 4, 2)
    assert nb.tolist() == [[2, 1], [3, 0], [0, 1], [1, -1], [-1, -1]]
    sim = lambda s_ij, i, j: F(D(s_ij) / 16 * rs[i] * cs[j])                  # left to right, one rounding to float32
    want = [[sim(13, 0, 2), sim(13, 0, 1)],                                  # 0.1915, 0.1564
            [sim(8, 1, 3), sim(13, 1, 0)],                                   # 0.1667, 0.1564; item 2 at 0.0737 is cut
            [sim(13, 2, 0), sim(5, 2, 1)],
            [sim(8, 3, 1), F(-np.inf)],
            [F(-np.inf), F(-np.inf)]]
    assert [round(float(v), 4) for v in want[0] + want[1]] == [0.1915, 0.1564, 0.1667, 0.1564]
    assert sc.dtype == np.float32 and sc.view(np.uint32).tolist() == np.array(want, F).view(np.uint32).tolist()
    # the picked shift: the longest item list has 3 users
    assert R3.rp3_terms(INDPTR, ITEMS, 4, 5, 1.0, 0.5)[3] == 40
    assert R3.rp3_terms(INDPTR, ITEMS, 4, 5, 1.0, 0.5)[0].tolist() == [2 ** 39, int(np.rint(2 ** 40 / 3)), 2 ** 39, 2 ** 39]


def test_restatement_zero_weights_and_zero_scales():
    one = np.ones(5)
    # user 3 is the only link between items 1 and 3: at weight 0 they are not neighbours
    s = R3.weighted_sums(INDPTR, ITEMS, 4, 5, [1, 1, 1, 0])
    nb, sc = R3.fit(s, one, one, 0, 4)
    assert nb[3].tolist() == [-1] * 4 and 3 not in nb[1].tolist()
    assert nb[1].tolist() == [0, 2, -1, -1] and sc[1, :2].tolist() == [2.0, 1.0]
    # a row scale of 0: the row keeps its candidates, all at +0, in id order
    s = R3.weighted_sums(INDPTR, ITEMS, 4, 5, [3, 1, 2, 5])
    nb, sc = R3.fit(s, [1, 0, 1, 1, 1], one, 0, 4)
    assert nb[1].tolist() == [0, 2, 3, -1] and sc[1, :3].view(np.uint32).tolist() == [0, 0, 0]
    # equal sums with different column scales are told apart; different sums that round to one float32 tie by id
    s = R3.weighted_sums(INDPTR, ITEMS, 4, 5, [3, 1, 3, 5])                  # S_01 = S_02 = 4
    nb, sc = R3.fit(s, one, [1, 0.5, 1, 1, 1], 0, 4)
    assert nb[0].tolist() == [2, 1, -1, -1] and sc[0, :2].tolist() == [4.0, 2.0]
    big = R3.weighted_sums(INDPTR, ITEMS, 4, 5, [2 ** 30, 2 ** 30 + 1, 2 ** 30 + 2, 0])
    nb, sc = R3.fit(big, one, one, 0, 4)                                     # S_01 = 2^31 + 1, S_02 = 2^31 + 3: one float32
    assert nb[0].tolist() == [1, 2, -1, -1] and sc[0, 0] == sc[0, 1] == F(2 ** 31)


def zipf_case(n_users=600, n_items=400, seed=31):
    rs = np.random.RandomState(seed)
    p = 1.0 / (np.arange(n_items) + 5.0)
    p /= p.sum()
    rows = [np.unique(rs.choice(n_items, rs.randint(1, 60), p=p)) for _ in range(n_users)]
    indptr = np.cumsum([0] + [r.size for r in rows]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), n_users, n_items


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.6), (0.5, 0.0), (2.0, 1.0)])
def test_distance_to_the_unrounded_model(alpha, beta):
    """every kept similarity within 2^-(shift+1) / min_u w_u + 2^-24 + (c_ij + 8) * 2^-53, relative, of scipy's float64
    diag(n^-alpha) X^T diag(d^-alpha) X diag(n^-beta): one rounding per user weight, the float32 rounding, and the float64
    chains of both sides"""
    indptr, items, nu, ni = zipf_case()
    q, rs, cs, shift = R3.rp3_terms(indptr, items, nu, ni, alpha, beta)
    assert shift == 40
    nb, sc = R3.fit(R3.weighted_sums(indptr, items, nu, ni, q), rs, cs, shift, 50)
    exact = R3.rp3_float64(indptr, items, nu, ni, alpha, beta).toarray()
    c = R.cooccurrence(indptr, items, nu, ni)[0].toarray()
    w_min = R3.neg_power(np.diff(indptr), alpha).min()                       # every user of the case has an item
    assert w_min > 0
    rows, cols = np.nonzero(nb >= 0)
    j = nb[rows, cols]
    assert rows.size > 5000
    got, want = sc[rows, cols].astype(D), exact[rows, j]
    bound = 2.0 ** -(shift + 1) / w_min + 2.0 ** -24 + (c[rows, j] + 8) * 2.0 ** -53
    rel = np.abs(got - want) / want
    worst = int(np.argmax(rel / bound))
    print("alpha %g beta %g: largest relative distance %.4g at a bound of %.4g" % (alpha, beta, rel[worst], bound[worst]))
    assert (rel <= bound).all()


def test_beta_zero_is_p3alpha():
    """P3alpha (Cooper et al. 2014): the two-step transition probability item -> user -> item with every probability raised to
    alpha: (1 / n_i)^alpha * sum over shared users of (1 / d_u)^alpha, and no factor of the target"""
    indptr, items, nu, ni = zipf_case(120, 80, seed=32)
    q, rs, cs, shift = R3.rp3_terms(indptr, items, nu, ni, 0.7, 0.0)
    n = np.bincount(items, minlength=ni)
    assert cs.tolist() == (n > 0).astype(D).tolist()                         # n^-0 = 1; an empty item stays 0
    nb, sc = R3.fit(R3.weighted_sums(indptr, items, nu, ni, q), rs, cs, shift, 10)
    x = R.pattern(indptr, items, nu, ni).toarray().astype(D)
    deg = np.diff(indptr).astype(D)
    p_iu = (x.T / np.maximum(n, 1)[:, None]) ** 0.7 * (x.T > 0)              # item -> user
    p_ui = (x / deg[:, None]) ** 0.7 * (x > 0)                               # user -> item
    p3 = p_iu @ p_ui
    for i in range(ni):
        kept = nb[i][nb[i] >= 0]
        assert np.allclose(sc[i, :kept.size], p3[i, kept], rtol=1e-6, atol=0)
        others = np.setdiff1d(np.flatnonzero(p3[i] > 0), [i])
        assert kept.size == min(10, others.size)
        if kept.size:
            assert p3[i, np.setdiff1d(others, kept)].max(initial=0.0) <= p3[i, kept].min() * (1 + 1e-6)


def test_shift_choice():
    for n_max, want in [(0, 40), (1, 40), (2 ** 22 - 1, 40), (2 ** 22, 39), (2 ** 31 - 1, 31)]:
        assert RP.pick_shift(n_max) == R3.shift_for(n_max) == want
        assert n_max * 2 ** want < 2 ** 62                                   # weights are at most 2^shift each
    assert 2 ** 22 * 2 ** 40 >= 2 ** 62                                      # why 2^22 users of one item step down
    q = RP.quantise([0.0, 1.0, 0.5, 1 / 3], 40)
    assert q.dtype == np.uint64 and q.tolist() == [0, 2 ** 40, 2 ** 39, 366503875925]
    for bad in ([-0.1], [1.5], [np.nan]):
        with pytest.raises(ValueError):
            RP.quantise(bad, 40)


def test_weighted_plan_is_consistent():
    seen = set()
    for n_items in (1, 100, 8191, 8192, 8193, 16383, 16384, 16385, 32771, 70000, 262144, 500000):
        for k in (1, 10, 20, 64, 65, 192, 193, 256):
            for n_rows in (0, 1, 3000, 70000, 10 ** 7):
                try:
                    p = RP.weighted_plan(n_items, k, n_rows)
                except T.TfrError as e:
                    assert e.code == L.ERR_ARG
                    assert -(-n_items // 8192) * k > 8192 or -(-n_items // 8192) > 256      # refused only past the merge
                    continue
                seen.add((p["width"], p["lds"]))
                assert p["width"] == 8192
                assert p["slices"] * p["width"] >= n_items > (p["slices"] - 1) * p["width"]
                assert p["slices"] * k <= 8192 and p["slices"] <= 256
                assert 8 * p["width"] < p["lds"] <= 163840                   # the uint64 sums and the queues
                assert p["chunk"] >= 1 and p["chunk"] * p["slices"] * k * 8 <= max(128 << 20, p["slices"] * k * 8)
                assert p["ahead"] >= 1
    assert len(seen) == 2                                                    # the two queue sizes
    assert RP.weighted_plan(70000, 10, 70000)["chunk"] < 70000               # the 70 000-item case takes two row chunks
    assert RP.weighted_plan(8192 * 32, 256, 1)["slices"] == 32               # the cap at K 256
    with pytest.raises(T.TfrError):
        RP.weighted_plan(8192 * 32 + 1, 256, 1)


def test_argument_errors_without_a_handle():
    lib = L.load()
    for bad in [(0, 10, 1), (100, 0, 1), (100, 257, 1), (100, 10, -1), (2 ** 31, 10, 1)]:
        assert lib.tfr_knn_weighted_plan(*bad, None, None, None, None, None) == L.ERR_ARG
        assert b"knn weighted plan" in lib.tfr_knn_last_error()
    assert lib.tfr_knn_weighted_plan(100, 10, 1, None, None, None, None, None) == L.OK
    assert lib.tfr_knn_plan(100, 10, 1, 2, None, None, None, None, None) == L.ERR_ARG       # tfr_knn_plan's which stays 0 or 1
    q = np.ones(3, np.uint64)
    s = np.ones(3, D)
    assert lib.tfr_knn_fit_weighted(None, q.ctypes.data_as(C.POINTER(C.c_uint64)), s.ctypes.data_as(L._f64p),
                                    s.ctypes.data_as(L._f64p), 0, None) == L.ERR_ARG
    assert b"null model" in lib.tfr_knn_last_error()
