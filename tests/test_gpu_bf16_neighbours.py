"""Nearest neighbours from the bf16 snapshot on the device (tfr_bf16_neighbours*, SvdModel.similar_items_bf16 /
similar_users_bf16 and their _dev twins): bit for bit against tests/neighbours_ref.py on tables where the dot and the norms
are exact in any order, against float64 on round-tripped random tables, the device twins against the host entries, and the
snapshot's own inverse-norm cache."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import bf16
from tests import bf16_rank_cases as RC
from tests import bf16_topk_cases as C
from tests.neighbours_ref import (dyadic_table, neighbour_scores, neighbours_from_scores, neighbours_ref, pow4_table,
                                  scores_f64)
from tests.test_gpu_neighbours import bits, random_excl, svd_model, with_ties

pytestmark = pytest.mark.gpu


def snap_model(P, Q, **kw):
    m = svd_model(P, Q, **kw)
    m.snapshot_bf16()
    return m


# ---------------------------------------------------------------- 1. bit for bit on exact tables
@pytest.mark.parametrize("D", C.WIDTHS)
def test_exact_on_dyadic_and_pow4_tables(D):
    """dyadic_table: entries k / 8, so every product, every partial sum of a dot and every partial sum of ss is exact in
    float32 whatever the order: the tile's sum is the reference's chain, ss the reference's, and rn and the cosine follow by
    the same correctly rounded operations.  pow4_table: rn is a power of two as well."""
    rs = np.random.RandomState(3000 + D)
    R, lo, hi = 300, 37, 229
    Q = with_ties(rs, dyadic_table(rs, R, D))
    P = with_ties(rs, pow4_table(rs, R, D))
    assert np.array_equal(bf16.round_trip(Q), Q) and np.array_equal(bf16.round_trip(P), P)
    allrows = np.arange(R, dtype=np.int32)
    q = np.concatenate([rs.randint(0, R, 40), [R - 1, 0, R // 3, 0]]).astype(np.int32)
    ex, xrows = random_excl(rs, q.size, R)
    ref = {}                                                                   # the reference scores, computed once each
    for item_abs in (False, True):
        m = snap_model(P, Q, item_abs=item_abs)
        for name, tab, fn, ab in (("Q", Q, m.similar_items_bf16, item_abs), ("P", P, m.similar_users_bf16, False)):
            for metric in ("dot", "cosine"):
                if (name, metric, ab) not in ref:
                    ref[name, metric, ab] = neighbour_scores(tab, allrows, metric, ab)
                S = ref[name, metric, ab]
                what = (D, item_abs, fn.__name__, metric)
                for k in (10, 129):                                            # both queue capacities
                    ids, sc = fn(allrows, k, metric)
                    wi, ws = neighbours_from_scores(S, allrows, k)
                    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), what + (k,)
                    assert not np.any(ids == allrows[:, None])                  # the query row is never its own neighbour
                for kw, rkw in ((dict(exclude=ex), dict(excl=xrows)), (dict(lo=lo, hi=hi), dict(lo=lo, hi=hi)),
                                (dict(exclude=ex, lo=3, hi=7), dict(excl=xrows, lo=3, hi=7))):
                    ids, sc = fn(q, 10, metric, **kw)
                    wi, ws = neighbours_from_scores(S[q], q, 10, **rkw)
                    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), what + tuple(kw)
                    assert not np.any(ids == q[:, None])
                    if "exclude" in kw:
                        assert all(not set(ids[r].tolist()) & set(xrows[r].tolist()) for r in range(q.size))
                    if "lo" in kw:
                        assert np.all((ids == -1) | ((ids >= kw["lo"]) & (ids < kw["hi"])))
        # a zero row (with_ties made row R // 3 one): every cosine is +0, so its neighbours are the lowest ids
        ids, sc = m.similar_items_bf16([R // 3], 5)
        assert ids[0].tolist() == [0, 1, 2, 3, 4] and np.all(bits(sc) == 0)
        ids, sc = m.similar_items_bf16([0, 7], 2, "cosine", lo=R // 3, hi=R // 3 + 1)
        assert np.array_equal(ids, [[R // 3, -1]] * 2) and np.all(bits(sc[:, 0]) == 0)      # and as the only candidate
        m.close()


# ---------------------------------------------------------------- 2. random tables against float64
@pytest.mark.parametrize("D", [64, 27])
def test_random_tables_against_float64(D):
    """scores within 1e-5 max|score| of float64 on the round-tripped table; an id may differ from the float64 top k only
    where its score is within that of the k-th (tests/test_gpu_topk.py check_oracle)"""
    rs = np.random.RandomState(20)
    R, k = 1200, 10
    Tab = rs.normal(0, .3, (R, D)).astype(np.float32)
    rt = bf16.round_trip(Tab)
    rows = np.arange(R, dtype=np.int32)
    for item_abs in (False, True):
        m = snap_model(Tab[:8].copy(), Tab, item_abs=item_abs)
        for metric in ("cosine", "dot"):
            S64 = scores_f64(rt, rows, metric, item_abs)
            tol = 1e-5 * np.abs(S64).max()
            ids, sc = m.similar_items_bf16(rows, k, metric)
            got64 = np.take_along_axis(S64, ids.astype(np.int64), 1)
            err = float(np.abs(sc - got64).max())
            print("D %d item_abs %d %s: largest score error %.3g = %.3f of the tolerance %.3g" % (D, item_abs, metric, err, err / tol, tol))
            assert np.all(ids >= 0) and not np.any(ids == rows[:, None])
            assert err <= tol
            for r in range(R):
                assert len(set(ids[r].tolist())) == k
                s = sc[r]
                assert np.all(s[:-1] >= s[1:])
                eq = s[:-1] == s[1:]
                assert np.all(ids[r][:-1][eq] < ids[r][1:][eq])
                elig = np.ones(R, bool)
                elig[r] = False
                kth = np.sort(S64[r][elig])[::-1][k - 1]
                assert np.all(S64[r, ids[r]] >= kth - tol)
        m.close()


# ---------------------------------------------------------------- 3. the device twins
def test_device_twins_equal_the_host_entries():
    import torch
    rs = np.random.RandomState(9)
    U, I, D = 500, 2000, 40
    P = rs.normal(0, .3, (U, D)).astype(np.float32)
    Q = rs.normal(0, .3, (I, D)).astype(np.float32)
    m = snap_model(P, Q, item_abs=True)
    dev = torch.device("cuda", 0)
    for R, host, twin in ((I, m.similar_items_bf16, m.similar_items_bf16_dev), (U, m.similar_users_bf16, m.similar_users_bf16_dev)):
        q = rs.randint(0, R, 300).astype(np.int32)
        ex, xrows = random_excl(rs, q.size, R)
        dq = torch.from_numpy(q).to(dev)
        dex = (torch.from_numpy(ex[0]).to(dev), torch.from_numpy(ex[1]).to(dev))
        for metric in ("cosine", "dot"):
            hi_, hs = host(q, 25, metric, exclude=ex, lo=5, hi=R - 7)
            di, ds = twin(dq, 25, metric, exclude=dex, lo=5, hi=R - 7)
            m.sync()
            assert np.array_equal(di.cpu().numpy(), hi_) and np.array_equal(bits(ds.cpu().numpy()), bits(hs))
            only = twin(dq, 25, metric, return_scores=False)
            m.sync()
            assert np.array_equal(only.cpu().numpy(), host(q, 25, metric, return_scores=False))
    with pytest.raises(L.OutOfRangeError):
        m.similar_items_bf16_dev(torch.tensor([0, I], dtype=torch.int32, device=dev), 4)
        m.sync()
    ids, _ = m.similar_items_bf16([0, 1], 4)
    assert np.all(ids >= 0)
    m.close()


# ---------------------------------------------------------------- 4. state, errors and the norm cache
def test_no_snapshot_is_a_state_error_also_for_zero_rows():
    rs = np.random.RandomState(41)
    Q = dyadic_table(rs, 30, 16)
    m = svd_model(dyadic_table(rs, 20, 16), Q)
    lib = L.load()
    out = np.full((2, 4), 77, np.int32)
    good = np.array([0, 1], np.int32)

    def refused():
        for n in (2, 0):
            for which, hi in ((L.NB_ITEMS, 30), (L.NB_USERS, 20)):
                assert lib.tfr_bf16_neighbours(m._h, which, 1, L.ptr_i32(good), n, 4, None, None, 0, hi, L.ptr_i32(out),
                                               None) == L.ERR_STATE
                assert "tfr_bf16_snapshot" in L.last_error()
                assert lib.tfr_bf16_neighbours_dev(m._h, which, 1, None, n, 4, None, None, 0, hi, None, None) == L.ERR_STATE
                assert "tfr_bf16_snapshot" in L.last_error()
        # before every other check: a bad table, metric, k or range is not looked at
        assert lib.tfr_bf16_neighbours(m._h, 2, 7, L.ptr_i32(good), 2, 0, None, None, 5, 5, L.ptr_i32(out), None) == L.ERR_STATE
        with pytest.raises(T.TfrError) as e:
            m.similar_items_bf16(good, 4)
        assert e.value.code == L.ERR_STATE and "tfr_bf16_snapshot" in str(e.value)
        assert np.all(out == 77)

    refused()
    m.snapshot_bf16()
    assert m.similar_items_bf16(np.zeros(0, np.int32), 3)[0].shape == (0, 3)
    wi, ws = neighbours_ref(Q, good, 4, "cosine")
    ids, sc = m.similar_items_bf16(good, 4)
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws))
    m.drop_bf16()
    refused()
    ids, sc = m.similar_items(good, 4)
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws))         # the float32 entry after the refusals
    m.close()


def test_errors_leave_outputs_untouched():
    rs = np.random.RandomState(42)
    Q = dyadic_table(rs, 30, 16)
    m = snap_model(dyadic_table(rs, 20, 16), Q)
    lib = L.load()
    out = np.full((2, 4), 77, np.int32)
    good, ip = np.array([0, 1], np.int32), np.array([0, 1, 2], np.int64)

    def call(rows=good, which=L.NB_ITEMS, metric=1, k=4, indptr=None, excl=None, lo=0, hi=30):
        return lib.tfr_bf16_neighbours(m._h, which, metric, L.ptr_i32(rows), 2, k, None if indptr is None else L.ptr_i64(indptr),
                                       None if excl is None else L.ptr_i32(excl), lo, hi, L.ptr_i32(out), None)
    assert call(rows=np.array([0, 30], np.int32)) == L.ERR_OOB
    assert call(rows=np.array([0, 20], np.int32), which=L.NB_USERS, hi=20) == L.ERR_OOB
    assert call(indptr=ip, excl=np.array([3, 30], np.int32)) == L.ERR_OOB
    assert call(indptr=np.array([0, 0, 2], np.int64), excl=np.array([5, 3], np.int32)) == L.ERR_ARG
    for bad in (dict(k=0), dict(k=257), dict(metric=2), dict(metric=-1), dict(which=2), dict(lo=-1), dict(lo=5, hi=5),
                dict(hi=31), dict(which=L.NB_USERS, hi=21)):
        assert call(**bad) == L.ERR_ARG, bad
    assert np.all(out == 77)
    with pytest.raises(ValueError):
        m.similar_items_bf16([0], 3, metric="euclid")
    ids, sc = m.similar_items_bf16(good, 4, "dot")
    wi, ws = neighbours_ref(Q, good, 4, "dot")
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws))
    m.close()


def test_a_new_snapshot_rebuilds_the_norms_and_nothing_else_does():
    """change a row and snapshot: the cosine follows.  Before the snapshot, set_table and training steps move nothing; the
    float32 entry's own cached norms see none of it."""
    rs = np.random.RandomState(51)
    U, I, D, k = 90, 260, 24, 10
    P, Q = pow4_table(rs, U, D), pow4_table(rs, I, D)
    m = snap_model(P, Q, optimizer="sgd", lr=0.05)
    qi, qu = np.arange(0, I, 3, dtype=np.int32), np.arange(0, U, 2, dtype=np.int32)

    def both():
        return m.similar_items_bf16(qi, k), m.similar_users_bf16(qu, k)

    def same(a, b):
        return all(np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1])) for x, y in zip(a, b))

    def want(P_, Q_):
        return neighbours_ref(Q_, qi, k, "cosine"), neighbours_ref(P_, qu, k, "cosine")

    first = both()
    assert same(first, want(P, Q))
    assert same(both(), first)                                 # served from the cached norms: the same bits
    f32 = (m.similar_items(qi, k), m.similar_users(qu, k))
    assert same(f32, first)                                    # exact tables: the float32 entry agrees
    # scale one item row by 4 and one user row by 1/4: every dot with them moves, the cosine of exact rows does not - unless
    # the norms are stale, which multiplies those cosines by 4
    Q2, P2 = Q.copy(), P.copy()
    Q2[qi[5]] *= 4
    P2[qu[7]] *= 0.25
    Q2[qi[9]] = pow4_table(rs, 1, D)[0]                        # and a row that really changes
    m.set_table(L.Q, Q2)
    m.set_table(L.P, P2)
    assert same(both(), first)                                 # the old snapshot still answers
    assert same((m.similar_items(qi, k), m.similar_users(qu, k)), want(P2, Q2))        # the float32 entry reads the new tables
    m.snapshot_bf16()
    second = both()
    assert same(second, want(P2, Q2))
    assert not same(second, first)
    assert np.all(np.abs(second[0][1][np.isfinite(second[0][1])]) <= 1) and np.all(np.abs(second[1][1]) <= 1)
    # a training step moves the float32 tables and their norms; the snapshot and its norms stay
    m.train_step(rs.randint(0, U, 2000), rs.randint(0, I, 2000), rs.randint(1, 6, 2000).astype(np.float32))
    assert same(both(), second)
    assert not same((m.similar_items(qi, k), m.similar_users(qu, k)), second)
    # drop and snapshot again: the cache does not outlive the buffers it was built from
    m.drop_bf16()
    m.snapshot_bf16()
    t = m.tables()
    got = both()
    snap_Q, snap_P = bf16.pack_rows(t[L.Q].reshape(I, D)), bf16.pack_rows(t[L.P].reshape(U, D))
    rn_q, rn_p = RC.packed_rnorm(snap_Q), RC.packed_rnorm(snap_P)
    for (ids, sc), rows, rn, q in ((got[0], bf16.from_bits(snap_Q)[:, :D], rn_q, qi), (got[1], bf16.from_bits(snap_P)[:, :D], rn_p, qu)):
        dot64 = np.einsum("nkd,nd->nk", rows[ids].astype(np.float64), rows[q].astype(np.float64))
        cos = dot64 * rn[q].astype(np.float64)[:, None] * rn[ids].astype(np.float64)
        assert np.all(np.abs(sc - cos) <= 1e-5)                # the trained tables' snapshot, with its own norms
    m.close()
