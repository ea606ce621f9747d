"""Held-out ranking, host side: the launch plan, argument checks before any device work, the target CSR helper, and
tfrecomm_amd.ranking's metrics against the brute-force statement of tests/rank_ref.py.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd.engine import target_csr
from tests.rank_ref import metrics_brute, rank_ref
from tests.topk_ref import ordered_u32

DIMS = [d for d in range(1, 257) if d % 4 == 0 or d <= 64]


def plan(dim, n, nt, items):
    lds, ppb, sl, cap, ch = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    rc = L.load().tfr_rank_plan(dim, n, nt, items, C.byref(lds), C.byref(ppb), C.byref(sl), C.byref(cap), C.byref(ch))
    return rc, lds.value, ppb.value, sl.value, cap.value, ch.value


def test_plan_fits_every_shape():
    for dim in DIMS:
        for n in (1, 7, 4096, 10 ** 6):
            for nt in (0, 1, 32 * n, 3000 * n):
                for items in (1, 3706, 10 ** 6, 10 ** 8):
                    rc, lds, ppb, sl, cap, ch = plan(dim, n, nt, items)
                    assert rc == L.OK, (dim, n, nt, items)
                    assert 0 < lds <= 160 * 1024 and ppb == 32 and cap == 128, (lds, ppb, cap)
                    assert 160 * 1024 // lds >= 3                  # three counting blocks per CU
                    assert ch > 0 and ch % ppb == 0 and ch <= 32768
                    assert 1 <= sl <= min(1024, max(1, -(-items // 128)))


def test_plan_refuses_bad_shapes():
    assert plan(64, -1, 10, 100)[0] == L.ERR_ARG
    assert plan(64, 10, -1, 100)[0] == L.ERR_ARG
    assert plan(64, 10, 10, 0)[0] == L.ERR_ARG
    for dim in (0, 65, 67, 260, 300):
        assert plan(dim, 10, 10, 100)[0] == L.ERR_ARG


def test_bad_arguments_rejected_before_device_work():
    lib = L.load()
    u = np.zeros(2, np.int32)
    ip = np.array([0, 1, 2], np.int64)
    it = np.array([3, 4], np.int32)
    out = np.full(2, 77, np.int32)
    assert lib.tfr_rank_items(None, L.ptr_i32(u), 2, L.ptr_i64(ip), L.ptr_i32(it), None, None, L.ptr_i32(out)) == L.ERR_ARG
    assert lib.tfr_fm_rank_items(None, L.ptr_i32(u), 2, 0, 10, L.ptr_i64(ip), L.ptr_i32(it), None, None,
                                 L.ptr_i32(out)) == L.ERR_ARG
    assert np.all(out == 77)


def test_target_csr_sorts_rows_and_refuses_repeats():
    ip = np.array([2, 5, 5, 7], np.int64)
    it = np.array([99, 99, 9, 1, 5, 4, 3], np.int32)
    indptr, items, order = target_csr((ip, it), [0, 1, 2])
    assert indptr.tolist() == [0, 3, 3, 5]
    assert items.tolist() == [1, 5, 9, 3, 4]
    assert it[2:][order].tolist() == items.tolist()
    with pytest.raises(ValueError):
        target_csr((np.array([0, 2], np.int64), np.array([3, 3], np.int32)), [0])
    with pytest.raises(ValueError):
        target_csr((np.array([0, 2, 1], np.int64), np.array([3, 4], np.int32)), [0, 1])
    import scipy.sparse as sp
    x = sp.csr_matrix((np.ones(3), ([1, 1, 0], [7, 2, 5])), shape=(2, 10))
    indptr, items, order = target_csr(x, [1, 0, 1])
    assert indptr.tolist() == [0, 2, 3, 5] and items.tolist() == [2, 7, 5, 2, 7] and order is None


def random_rows(rs, I, n):
    S = rs.choice(np.array([-1.0, -0.5, 0.25, 0.5, 1.0, np.inf, -np.inf, np.nan], np.float32), (n, I))
    Ts, Xs = [], []
    for r in range(n):
        Ts.append(np.sort(rs.choice(I, rs.randint(0, I + 1), replace=False)))
        Xs.append(np.sort(rs.choice(I, rs.randint(0, I + 1), replace=True)))
    return S, Ts, Xs


def check_against_brute(S, Ts, Xs, ks):
    n, I = S.shape
    ranks = rank_ref(S, Ts, Xs)
    indptr = np.concatenate([[0], np.cumsum([t.size for t in Ts])]).astype(np.int64)
    n_elig = np.array([I - np.unique(x).size for x in Xs], np.int64)
    t_elig = np.array([np.setdiff1d(t, x).size for t, x in zip(Ts, Xs)], np.int64)
    got = T.ranking_metrics(ranks, indptr, n_elig, ks, n_targets_eligible=t_elig)
    for r in range(n):
        want, wr = metrics_brute(S[r], Ts[r], Xs[r], ks)
        assert ranks[indptr[r]:indptr[r + 1]].tolist() == [wr[int(t)] for t in Ts[r]]
        for key, v in want.items():
            g = got[key][r]
            assert (np.isnan(v) and np.isnan(g)) or g == pytest.approx(v, rel=1e-12, abs=1e-12), (r, key, g, v)
    return got


def test_metrics_match_brute_force_with_ties_and_nans():
    rs = np.random.RandomState(0)
    for trial in range(60):
        I = rs.randint(1, 30)
        S, Ts, Xs = random_rows(rs, I, 5)
        check_against_brute(S, Ts, Xs, (1, 3, 10, 40))


def test_metrics_edge_cases():
    rs = np.random.RandomState(1)
    I = 12
    S = rs.choice(np.array([-1.0, 0.0, 0.5, 1.0], np.float32), (5, I))
    Ts = [np.zeros(0, np.int64),                        # empty target row
          np.array([1, 4, 7]),                          # all unranked (all excluded)
          np.arange(I),                                 # n_t > K, K > |E|
          np.array([0, 11]),
          np.array([3])]
    Xs = [np.array([2]), np.array([1, 4, 4, 7]), np.array([0, 0, 5]), np.zeros(0, np.int64), np.arange(I)]
    got = check_against_brute(S, Ts, Xs, (2, 5, 50))
    assert np.isnan(got["recall@5"][0]) and np.isnan(got["mrr"][0]) and np.isnan(got["auc"][0])
    assert got["recall@5"][1] == 0 and got["mrr"][1] == 0 and np.isnan(got["auc"][1])
    assert got["ndcg@5"][2] <= 1.0 and got["recall@50"][2] == (I - 2) / I
    assert np.isnan(got["auc"][4])                      # nothing eligible


def test_default_negatives_are_the_ranked_targets():
    ranks = np.array([0, 3, -1, 2], np.int64)
    indptr = np.array([0, 3, 4], np.int64)
    m = T.ranking_metrics(ranks, indptr, 10, ks=(1, 3))
    # row 0: ranked {0, 3}, |E - T| = 10 - 2 = 8; target 0 beats 8, target 3 (one target above) beats 8 - 2 = 6
    assert m["auc"][0] == pytest.approx(14 / 16)
    assert m["recall@1"][0] == pytest.approx(1 / 3) and m["hits@3"][0] == 1 and m["mrr"][1] == pytest.approx(1 / 3)


def test_auc_is_roc_auc_on_tie_free_scores():
    metrics = pytest.importorskip("sklearn.metrics")
    rs = np.random.RandomState(2)
    n, I = 20, 300
    S = rs.permutation(n * I).reshape(n, I).astype(np.float32) * np.float32(0.25) - 100
    S[3, 17] = np.nan
    Ts, Xs = [], []
    for r in range(n):
        Ts.append(np.sort(rs.choice(I, rs.randint(1, 40), replace=False)))
        Xs.append(np.sort(rs.choice(I, rs.randint(0, 60), replace=True)))
    ranks = rank_ref(S, Ts, Xs)
    indptr = np.concatenate([[0], np.cumsum([t.size for t in Ts])]).astype(np.int64)
    n_elig = np.array([I - np.unique(x).size for x in Xs])
    got = T.ranking_metrics(ranks, indptr, n_elig, (10,), n_targets_eligible=[np.setdiff1d(t, x).size for t, x in zip(Ts, Xs)])
    for r in range(n):
        E = np.ones(I, bool)
        E[Xs[r]] = False
        y = np.zeros(I, bool)
        y[Ts[r]] = True
        sel = E & ~np.isnan(S[r])
        if r != 3:
            want = metrics.roc_auc_score(y[sel], S[r][sel])
            assert got["auc"][r] == pytest.approx(want, rel=1e-12), r
    o = ordered_u32(S[0])
    assert np.all(np.diff(np.sort(o)) > 0)              # tie-free by construction
