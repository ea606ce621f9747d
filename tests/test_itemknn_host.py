"""ItemKNN without a GPU: the NumPy restatement (tests/itemknn_ref.py) against values worked out by hand, the launch plan's
consistency (tfr_knn_plan is host-only), the argument errors that need no handle, and the export.

tfr_knn_create refuses without a device after its argument checks, so everything that needs a handle - the checks of
tfr_knn_load and of the list, exclusion and target rows, and the calls in the wrong state - is in tests/test_gpu_itemknn.py
(test_argument_and_state_errors)."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import itemknn as IK
from tests import itemknn_ref as R

# 5 users x 4 items: users of item 0: {0,1,2,4}, of 1: {0,1,3}, of 2: {1,2}, of 3: {4}
ROWS = [[0, 1], [0, 1, 2], [0, 2], [1], [0, 3]]
INDPTR = np.cumsum([0] + [len(r) for r in ROWS]).astype(np.int64)
ITEMS = np.concatenate(ROWS).astype(np.int32)
F = np.float32


def test_itemknn_is_exported():
    assert T.ItemKNN is IK.ItemKNN and "ItemKNN" in T.__all__
    for name in ("fit", "neighbours", "set_neighbours", "similar_items", "recommend", "recommend_lists", "rank_items"):
        assert callable(getattr(T.ItemKNN, name))


def test_restatement_counts_and_metrics_by_hand():
    c, n = R.cooccurrence(INDPTR, ITEMS, 5, 4)
    assert n.tolist() == [4, 3, 2, 1]
    assert c.toarray().tolist() == [[4, 2, 2, 1], [2, 3, 1, 0], [2, 1, 2, 0], [1, 0, 0, 1]]
    s01, s02, s03, s12 = F(2 / np.sqrt(12.0)), F(2 / np.sqrt(8.0)), F(0.5), F(1 / np.sqrt(6.0))
    nb, sc = R.fit(c, n, 2, "cosine", 0.0)
    assert nb.tolist() == [[2, 1], [0, 2], [0, 1], [0, -1]]
    assert sc.view(np.uint32).tolist() == np.array([[s02, s01], [s01, s12], [s02, s12], [s03, -np.inf]], F).view(np.uint32).tolist()
    nb, sc = R.fit(c, n, 3, "cosine", 2.5)
    assert nb[3].tolist() == [0, -1, -1] and sc[3, 0] == F(1 / (2.0 + 2.5))
    assert nb[0].tolist() == [2, 1, 3] and sc[0, 1] == F(2 / (np.sqrt(12.0) + 2.5))
    nb, sc = R.fit(c, n, 2, "jaccard", 0.0)
    assert nb.tolist() == [[2, 1], [0, 2], [0, 1], [0, -1]]                  # (0,1) 2/5, (0,2) 2/4, (0,3) 1/4, (1,2) 1/4
    assert sc[0].tolist() == [F(0.5), F(0.4)] and sc[1].tolist() == [F(0.4), F(0.25)] and sc[3, 0] == F(0.25)
    nb, sc = R.fit(c, n, 2, "jaccard", 2.5)
    assert sc[0].tolist() == [F(2 / 6.5), F(2 / 7.5)]
    nb, sc = R.fit(c, n, 2, "count", 0.0)
    assert nb.tolist() == [[1, 2], [0, 2], [0, 1], [0, -1]]                  # item 0: 1 and 2 tie at 2 users, the id decides
    assert sc.tolist() == [[2, 2], [2, 1], [2, 1], [1, -np.inf]]


def test_restatement_user_scores_by_hand():
    c, n = R.cooccurrence(INDPTR, ITEMS, 5, 4)
    nb, sc = R.fit(c, n, 2, "cosine", 0.0)
    s01, s02, s12 = F(2 / np.sqrt(12.0)), F(2 / np.sqrt(8.0)), F(1 / np.sqrt(6.0))
    got = R.user_scores(ROWS[2], nb, sc, 4)                                  # items 0 then 2
    assert got.dtype == np.float32
    assert got.tolist() == [s02, F(s01 + s12), s02, F(0)]                    # item 3 is not among item 0's two kept
    assert R.user_scores([], nb, sc, 4).tolist() == [0, 0, 0, 0]
    items, scores = R.topk(got, 3, excl=ROWS[2])
    assert items.tolist() == [1, 3, -1] and scores.tolist() == [F(s01 + s12), 0.0, -np.inf]
    assert R.ranks(got, [0, 1, 3], excl=[0]).tolist() == [-1, 0, 2]          # 1 (s01 + s12 = 0.99) beats 2 (s02 = 0.71); 3 scores 0


def test_restatement_rank_is_the_position_in_topk():
    """rank < k exactly when top-k returns the item, at that position: every k <= 12 on a 12-item catalogue with tied
    scores, zeros, negative scores and exclusions"""
    rs = np.random.RandomState(3)
    n_items = 12
    for trial in range(40):
        scores = rs.choice(np.array([-1.5, 0.0, 0.0, 0.25, 0.25, 1.0, 2.5], F), n_items).astype(F)
        excl = rs.choice(n_items, rs.randint(0, 5), replace=False)
        rk = R.ranks(scores, np.arange(n_items), excl)
        assert sorted(rk[rk >= 0].tolist()) == list(range(n_items - excl.size))
        assert set(np.flatnonzero(rk < 0).tolist()) == set(excl.tolist())
        for k in range(1, n_items + 1):
            items, _ = R.topk(scores, k, excl)
            for t in range(n_items):
                assert (0 <= rk[t] < k) == (t in items.tolist())
                if 0 <= rk[t] < k:
                    assert items[rk[t]] == t


@pytest.mark.parametrize("which", [0, 1])
def test_plan_is_consistent(which):
    seen = set()
    for n_items in (1, 100, 8191, 8192, 8193, 16383, 16384, 16385, 32771, 70000, 262144, 500000):
        for k in (1, 10, 20, 64, 65, 192, 193, 256):
            for n_rows in (0, 1, 3000, 70000, 10 ** 7):
                try:
                    p = IK.plan(n_items, k, n_rows, which)
                except T.TfrError as e:
                    assert e.code == L.ERR_ARG
                    width = 8192 if which else 16384
                    assert -(-n_items // width) * k > 8192 or -(-n_items // width) > 256      # refused only past the merge
                    continue
                seen.add((p["width"], p["lds"]))
                assert p["slices"] * p["width"] >= n_items > (p["slices"] - 1) * p["width"]
                assert p["slices"] * k <= 8192 and p["slices"] <= 256
                assert 0 < p["lds"] <= 163840
                assert p["chunk"] >= 1 and p["chunk"] * p["slices"] * k * 8 <= max(128 << 20, p["slices"] * k * 8)
                assert p["ahead"] >= 1
    assert len(seen) >= 1
    assert IK.plan(70000, 10, 70000, 0)["chunk"] < 70000                       # the 70 000-item case takes two row chunks


def test_plan_and_create_argument_errors():
    lib = L.load()
    for bad in [(0, 10, 1, 0), (100, 0, 1, 0), (100, 257, 1, 1), (100, 10, -1, 0), (100, 10, 1, 2), (2 ** 31, 10, 1, 0)]:
        assert lib.tfr_knn_plan(*bad, None, None, None, None, None) == L.ERR_ARG
    assert lib.tfr_knn_plan(100, 10, 1, 1, None, None, None, None, None) == L.OK
    h = L._p()

    def create(n_users=10, n_items=10, K=5, metric=0, shrink=0.0, out=C.byref(h)):
        return lib.tfr_knn_create(out, n_users, n_items, K, metric, shrink, 0)
    assert create(K=0) == L.ERR_ARG and b"k must be" in lib.tfr_knn_last_error()
    assert create(K=257) == L.ERR_ARG
    assert create(metric=3) == L.ERR_ARG and create(metric=-1) == L.ERR_ARG
    assert b"metric" in lib.tfr_knn_last_error()
    assert create(shrink=-0.5) == L.ERR_ARG
    assert create(shrink=float("nan")) == L.ERR_ARG
    assert create(shrink=float("inf")) == L.ERR_ARG
    assert b"shrink" in lib.tfr_knn_last_error()
    assert create(metric=2, shrink=1.0) == L.ERR_ARG
    assert create(n_users=0) == L.ERR_ARG and create(n_items=0) == L.ERR_ARG
    assert create(n_items=16384 * 32 + 1, K=256) == L.ERR_ARG                    # 33 slices of 256 keys: past the merge
    assert create(out=None) == L.ERR_ARG
    assert not h
    assert lib.tfr_knn_destroy(None) == L.OK
    for call in (lambda: lib.tfr_knn_fit(None, None), lambda: lib.tfr_knn_load(None, None, None),
                 lambda: lib.tfr_knn_topk(None, None, 0, 1, None, None, None, None),
                 lambda: lib.tfr_knn_rank_items(None, None, 0, None, None, None, None, None)):
        assert call() == L.ERR_ARG
    with pytest.raises(ValueError):
        T.ItemKNN(10, 10, metric="dice")


def test_no_cpu_path():
    """without a HIP device a well-formed create is refused; with one it gives a handle"""
    if L.load().tfr_device_count() > 0:
        with T.ItemKNN(10, 10) as m:
            assert m._h
        return
    with pytest.raises(T.TfrError) as e:
        T.ItemKNN(10, 10)
    assert e.value.code == L.ERR_HIP and "no CPU path" in str(e.value)
