"""Held-out ranking from the bf16 snapshot on the device (tfr_bf16_rank_items, SvdModel.rank_items_bf16,
evaluate_ranking(bf16=True)): bit for bit against the contract (tests/rank_ref.py) where every score is exact, against
recommend_bf16 itself and a float64 bracket on random tables, at the edges of the pieces, tiles and slices, and the entry's
state and error handling.  The tile's width classes are those of tests/bf16_topk_cases.py."""
import ctypes as C_

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import bf16_cases
from tests import bf16_rank_cases as RC
from tests import bf16_topk_cases as C
from tests.rank_ref import rank_ref
from tests.test_gpu_rank import excl_with_repeats, random_targets, ref_ranks
from tests.test_gpu_topk import make

pytestmark = pytest.mark.gpu


def csr(rows, dtype=np.int32):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    items = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(dtype) if rows else np.zeros(0, dtype)
    return indptr, items


# ---------------------------------------------------------------- 1. bit for bit on dyadic tables
@pytest.mark.parametrize("D", C.WIDTHS)
def test_exact_on_dyadic_tables(D):
    rs = np.random.RandomState(100 + D)
    U, I = 70, 900
    for item_abs in (False, True):
        m, t = make(U, I, D, rs, item_abs=item_abs)
        assert C.dyadic_faults(t) == []
        m.snapshot_bf16()
        users = rs.randint(0, U, 40).astype(np.int32)
        tg, trows = random_targets(rs, users.size, I)
        for with_excl in (False, True):
            ex, xrows = excl_with_repeats(rs, users.size, I, trows) if with_excl else (None, None)
            got = m.rank_items_bf16(users, tg, exclude=ex)
            want = ref_ranks(m, t, users, trows, xrows)
            assert np.array_equal(got, want), (D, item_abs, with_excl)
            assert np.array_equal(got, m.rank_items(users, tg, exclude=ex)), (D, item_abs, with_excl)
        m.close()


# ---------------------------------------------------------------- 2. rank < K is the position in recommend_bf16
@pytest.mark.parametrize("D", [1, 17, 64, 100, 128, 256])
def test_rank_is_position_in_recommend_bf16_on_random_tables(D):
    rs = np.random.RandomState(200 + D)
    U, I, K = 50, 2000, 256
    for item_abs in (False, True):
        m, t = make(U, I, D, rs, dyad=False, item_abs=item_abs)
        m.snapshot_bf16()
        users = rs.randint(0, U, 30).astype(np.int32)
        items, _ = m.recommend_bf16(users, K)
        # targets: most of the top-K list, plus random items below it
        trows = [np.unique(np.concatenate([items[r][rs.rand(K) < 0.7], rs.randint(0, I, 40)])) for r in range(users.size)]
        indptr, titems = csr(trows)
        ex, xrows = excl_with_repeats(rs, users.size, I, trows, 0.05)
        for exclude in (None, ex):
            got = m.rank_items_bf16(users, (indptr, titems), exclude=exclude)
            rec, _ = m.recommend_bf16(users, K, exclude=exclude)
            for r in range(users.size):
                pos = {int(i): p for p, i in enumerate(rec[r])}
                xs = set() if exclude is None else set(xrows[r].tolist())
                for j, it in enumerate(trows[r]):
                    g = int(got[indptr[r] + j])
                    if int(it) in pos:
                        assert g == pos[int(it)], (D, item_abs, r, it)
                    elif int(it) in xs:
                        assert g == -1
                    else:
                        assert g >= K, (D, item_abs, r, it, g)
        m.close()


# ---------------------------------------------------------------- 3. bracket against float64 on the same random tables
@pytest.mark.parametrize("D", [1, 17, 64, 100, 128, 256])
def test_ranks_inside_the_float64_bracket_on_random_tables(D):
    """S64: the float64 scores of the round-tripped tables; tol = 1e-5 max|S64|, the tolerance tests/test_gpu_bf16_topk.py
    applies to these scores.  A rank by scores within tol of S64 lies in tests/bf16_rank_cases.rank_bracket.  The bracket
    says something: at least 75 % of the ranked targets have a single possible rank and no bracket is wider than 4."""
    rs = np.random.RandomState(200 + D)
    U, I = 50, 2000
    widths = []
    for item_abs in (False, True):
        m, t = make(U, I, D, rs, dyad=False, item_abs=item_abs)
        m.snapshot_bf16()
        snap = bf16_cases.snapshot_tables(t)
        users = rs.randint(0, U, 30).astype(np.int32)
        tg, trows = random_targets(rs, users.size, I)
        ex, xrows = excl_with_repeats(rs, users.size, I, trows, 0.05)
        got = m.rank_items_bf16(users, tg, exclude=ex)
        m.close()
        P, Q = snap["P"].astype(np.float64), snap["Q"].astype(np.float64)
        S64 = P[users] @ (np.abs(Q) if item_abs else Q).T + float(t["mu"]) + t["bu"].astype(np.float64)[users][:, None] \
            + t["bi"].astype(np.float64)[None, :]
        tol = 1e-5 * np.abs(S64).max()
        for r in range(users.size):
            elig = np.ones(I, bool)
            elig[xrows[r]] = False
            for j, it in enumerate(trows[r]):
                g = int(got[tg[0][r] + j])
                if not elig[it]:
                    assert g == -1
                    continue
                lo, hi = RC.rank_bracket(S64[r], elig, int(it), tol)
                assert lo <= g <= hi, (D, item_abs, r, it, g, lo, hi)
                widths.append(hi - lo)
    widths = np.asarray(widths)
    print("D %d: %d ranked targets, %.1f %% of the brackets have width 0, the widest %d" % (
        D, widths.size, 100 * np.mean(widths == 0), widths.max()))
    assert widths.size > 500
    assert np.mean(widths == 0) >= 0.75 and widths.max() <= 4


# ---------------------------------------------------------------- 4. edges of pieces, tiles and slices
@pytest.mark.parametrize("item_abs,planted", [(False, np.inf), (True, -np.inf)])
@pytest.mark.parametrize("D", [8, 17, 100])
def test_edges_and_planted_non_finite_values(D, item_abs, planted):
    """NF is odd: the upper half-wave's loads of the last step are aimed at the row's first fragment, which here holds an
    infinity or a NaN in some item rows; a lane past the piece, the exclusions or the slice loads a row inside it.  Item
    counts around the 32-row tile and the 128-item round, target rows around the 128-target piece, rows around the 32
    pieces of a counting block; rows without targets and rows with every target excluded."""
    assert C.tile_class(D)[0]
    rs = np.random.RandomState(400 + D)
    U = 40
    for I in (1, 31, 32, 33, 127, 128, 129):
        t = C.dyadic_tables(rs, U, I, D)
        t["P"][:, 0] = np.abs(t["P"][:, 0]) + np.float32(0.125)
        hot = np.sort(rs.choice(I, max(1, I // 9), replace=False)) if I > 1 else np.zeros(0, np.int64)
        nan = np.setdiff1d(np.sort(rs.choice(I, I // 16, replace=False)), hot)
        t["Q"][hot, 0] = planted
        t["Q"][nan, 0] = np.nan
        m = T.SvdModel(U, I, D, item_abs=item_abs)
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        m.snapshot_bf16()
        with np.errstate(invalid="ignore"):
            S_all = C.svd_scores(t["P"], t["Q"], t["bu"], t["bi"], t["mu"], np.arange(U), item_abs)
        if hot.size:
            assert np.all(S_all[:, hot] == np.inf) and np.all(np.isnan(S_all[:, nan]))
            assert np.all(np.isfinite(np.delete(S_all, np.concatenate([hot, nan]), axis=1)))
        for n in (1, 32, 33):
            for per in (1, 127, 128, 129, I):
                users = rs.randint(0, U, n).astype(np.int32)
                trows = [np.sort(rs.choice(I, min(per, I), replace=False)) for _ in range(n)]
                _, xrows = excl_with_repeats(rs, n, I, trows)
                for r in range(n):
                    if n > 1 and r % 5 == 1:
                        trows[r] = np.zeros(0, np.int64)                  # a row without targets
                    if n > 1 and r % 5 == 2:
                        xrows[r] = np.sort(np.concatenate([trows[r], trows[r][:3]]))    # every target excluded
                got = m.rank_items_bf16(users, csr(trows), exclude=csr(xrows))
                want = rank_ref(S_all[users], trows, xrows)
                assert np.array_equal(got, want), (D, I, n, per)
                ip = csr(trows)[0]
                for r in range(n):
                    if n > 1 and r % 5 == 2:
                        assert np.all(got[ip[r]:ip[r + 1]] == -1)
                if per == I and n == 1 and not len(xrows[0]):
                    ranked = got[got >= 0]                                # the whole catalogue: a permutation of the ranks
                    assert ranked.size == I - nan.size and np.array_equal(np.sort(ranked), np.arange(ranked.size))
        m.close()


# ---------------------------------------------------------------- 5. composition
def test_bit_identical_across_batches_chunks_and_order():
    rs = np.random.RandomState(4)
    U, I, D = 300, 500, 64
    m, t = make(U, I, D, rs, dyad=False)
    m.snapshot_bf16()
    lds, ppb, sl, cap, ch = C_.c_int64(), C_.c_int32(), C_.c_int32(), C_.c_int32(), C_.c_int64()
    n3 = 70000
    L.check(L.load().tfr_rank_plan(D, n3, n3, I, C_.byref(lds), C_.byref(ppb), C_.byref(sl), C_.byref(cap), C_.byref(ch)))
    assert n3 > 2 * ch.value
    u0 = np.int32(17)
    t0 = np.sort(rs.choice(I, 25, replace=False)).astype(np.int32)
    x0 = np.sort(rs.choice(I, 40, replace=False)).astype(np.int32)

    def alone_row(users, pos):
        n = users.size
        tl = [t0 if r in pos else rs.choice(I, 1).astype(np.int32) for r in range(n)]
        xl = [x0 if r in pos else np.zeros(0, np.int32) for r in range(n)]
        ti, xi = csr(tl)[0], csr(xl)[0]
        got = m.rank_items_bf16(users, (ti, np.concatenate(tl)), exclude=(xi, np.concatenate(xl)))
        return [got[ti[r]:ti[r + 1]] for r in pos]

    alone = m.rank_items_bf16([u0], (np.array([0, t0.size]), t0), exclude=(np.array([0, x0.size]), x0))
    assert np.any(alone >= 0)
    big = rs.randint(0, U, 5000).astype(np.int32)
    big[[5, 999, 4321]] = u0
    huge = rs.randint(0, U, n3).astype(np.int32)
    pos = [3, int(ch.value) + 11, 2 * int(ch.value) + 50]
    huge[pos] = u0
    for rows in (alone_row(big, {5, 999, 4321}), alone_row(huge, set(pos))):
        assert len(rows) == 3
        for g in rows:
            assert np.array_equal(g, alone)
    # row order: the same request reversed gives the same ranks per row
    users = rs.randint(0, U, 200).astype(np.int32)
    tg, trows = random_targets(rs, users.size, I, 1, 30)
    got = m.rank_items_bf16(users, tg)
    rev = users[::-1].copy()
    trev = trows[::-1]
    ip, ti = csr(trev)
    grev = m.rank_items_bf16(rev, (ip, ti))
    for r in range(users.size):
        rr = users.size - 1 - r
        assert np.array_equal(got[tg[0][r]:tg[0][r + 1]], grev[ip[rr]:ip[rr + 1]])
    # targets given in any order within a row come back aligned with the caller's order
    perm_items = tg[1].copy()
    for r in range(users.size):
        seg = perm_items[tg[0][r]:tg[0][r + 1]]
        rs.shuffle(seg)
    gperm = m.rank_items_bf16(users, (tg[0], perm_items))
    lut = {(r, int(i)): int(g) for r in range(users.size) for i, g in zip(trows[r], got[tg[0][r]:tg[0][r + 1]])}
    for r in range(users.size):
        for i, g in zip(perm_items[tg[0][r]:tg[0][r + 1]], gperm[tg[0][r]:tg[0][r + 1]]):
            assert lut[(r, int(i))] == g
    assert np.array_equal(m.rank_items_bf16(users, tg), got)         # and from run to run
    m.close()


# ---------------------------------------------------------------- 6. state and errors
def test_no_snapshot_is_a_state_error_also_for_zero_users():
    rs = np.random.RandomState(20)
    m, t = make(20, 30, 16, rs)
    lib = L.load()
    out = np.full(3, 77, np.int32)
    u = np.array([0, 1], np.int32)
    ip, tit = np.array([0, 2, 3], np.int64), np.array([1, 2, 3], np.int32)
    want = ref_ranks(m, t, u, [tit[:2], tit[2:]])
    f32 = m.rank_items(u, (ip, tit))

    def refused():
        for n in (2, 0):
            assert lib.tfr_bf16_rank_items(m._h, L.ptr_i32(u), n, L.ptr_i64(ip), L.ptr_i32(tit), None, None,
                                           L.ptr_i32(out)) == L.ERR_STATE
            assert "tfr_bf16_snapshot" in L.last_error()
        # before every other check: a bad user id is not looked at
        bad = np.array([0, 20], np.int32)
        assert lib.tfr_bf16_rank_items(m._h, L.ptr_i32(bad), 2, L.ptr_i64(ip), L.ptr_i32(tit), None, None,
                                       L.ptr_i32(out)) == L.ERR_STATE
        with pytest.raises(T.TfrError) as e:
            m.rank_items_bf16(u, (ip, tit))
        assert e.value.code == L.ERR_STATE and "tfr_bf16_snapshot" in str(e.value)
        assert np.all(out == 77)

    refused()
    m.snapshot_bf16()
    assert m.rank_items_bf16(np.zeros(0, np.int32), (np.array([0]), np.zeros(0, np.int32))).size == 0
    assert m.rank_items_bf16([1, 2], (np.array([0, 0, 0]), np.zeros(0, np.int32))).size == 0
    assert np.array_equal(m.rank_items_bf16(u, (ip, tit)), want)
    m.drop_bf16()
    refused()
    assert np.array_equal(m.rank_items(u, (ip, tit)), f32) and np.array_equal(f32, want)
    m.close()


def test_errors_leave_output_untouched():
    rs = np.random.RandomState(9)
    m, t = make(20, 30, 16, rs)
    m.snapshot_bf16()
    lib = L.load()
    out = np.full(3, 77, np.int32)
    u = np.array([0, 1], np.int32)
    ip = np.array([0, 2, 3], np.int64)

    def call(users, tip, tit, xip=None, xit=None):
        return lib.tfr_bf16_rank_items(m._h, L.ptr_i32(users), users.size, L.ptr_i64(tip), L.ptr_i32(tit),
                                       None if xip is None else L.ptr_i64(xip), None if xit is None else L.ptr_i32(xit),
                                       L.ptr_i32(out))
    assert call(np.array([0, 20], np.int32), ip, np.array([1, 2, 3], np.int32)) == L.ERR_OOB
    assert call(u, ip, np.array([1, 30, 3], np.int32)) == L.ERR_OOB
    assert call(u, ip, np.array([2, 1, 3], np.int32)) == L.ERR_ARG          # not increasing
    assert call(u, ip, np.array([2, 2, 3], np.int32)) == L.ERR_ARG          # a repeat
    assert call(u, np.array([0, 2, 1], np.int64), np.array([1, 2, 3], np.int32)) == L.ERR_ARG
    assert call(u, np.array([-1, 2, 3], np.int64), np.array([1, 2, 3], np.int32)) == L.ERR_ARG
    tit = np.array([1, 2, 3], np.int32)
    assert call(u, ip, tit, np.array([0, 1, 2], np.int64), np.array([4, 30], np.int32)) == L.ERR_OOB
    assert call(u, ip, tit, np.array([0, 2, 2], np.int64), np.array([5, 4], np.int32)) == L.ERR_ARG
    assert lib.tfr_bf16_rank_items(m._h, L.ptr_i32(u), -1, L.ptr_i64(ip), L.ptr_i32(tit), None, None, L.ptr_i32(out)) == L.ERR_ARG
    assert np.all(out == 77)
    with pytest.raises(L.OutOfRangeError):
        m.rank_items_bf16([0, 20], (ip, tit))
    with pytest.raises(ValueError):
        m.rank_items_bf16([0, 1], (ip, np.array([2, 2, 3], np.int32)))
    assert np.array_equal(m.rank_items_bf16(u, (ip, tit)), ref_ranks(m, t, u, [tit[:2], tit[2:]]))
    m.close()


def test_the_snapshot_answers_until_another_snapshot_and_float32_is_unchanged():
    rs = np.random.RandomState(21)
    U, I, D = 70, 900, 24
    m, t = make(U, I, D, rs, adam_mode="lazy")
    users = rs.randint(0, U, 40).astype(np.int32)
    tg, trows = random_targets(rs, users.size, I)
    ex, xrows = excl_with_repeats(rs, users.size, I, trows)
    first = ref_ranks(m, t, users, trows, xrows)
    f32_before = m.rank_items(users, tg, exclude=ex)
    assert np.array_equal(f32_before, first)
    m.snapshot_bf16()
    assert np.array_equal(m.rank_items_bf16(users, tg, exclude=ex), first)
    assert np.array_equal(m.rank_items(users, tg, exclude=ex), f32_before)      # the float32 entry: the same bits
    for _ in range(3):                                         # training moves the float32 tables only
        m.train_step(rs.randint(0, U, 500), rs.randint(0, I, 500), rs.randint(1, 6, 500).astype(np.float32))
    ids = [L.MU, L.BU, L.BI, L.P, L.Q] + [w | s for w in (L.MU, L.BU, L.BI, L.P, L.Q) for s in (L.SLOT_M, L.SLOT_V)]
    before = {w: m.get_table(w).copy() for w in ids}
    step = m.get_step()
    assert np.array_equal(m.rank_items_bf16(users, tg, exclude=ex), first)      # the old snapshot still answers
    for w in ids:
        assert np.array_equal(m.get_table(w).view(np.uint32), before[w].view(np.uint32)), w
    assert m.get_step() == step
    now = dict(mu=np.float32(m.get_table(L.MU).reshape(-1)[0]), bu=m.get_table(L.BU), bi=m.get_table(L.BI),
               P=m.get_table(L.P).reshape(U, D), Q=m.get_table(L.Q).reshape(I, D))
    f32_now = m.rank_items(users, tg, exclude=ex)
    assert not np.array_equal(f32_now, first)                  # the float32 entry reads the trained tables
    m.snapshot_bf16()
    second = m.rank_items_bf16(users, tg, exclude=ex)
    assert not np.array_equal(second, first)
    # the new snapshot: inside the float64 bracket of the trained tables, round-tripped
    snap = bf16_cases.snapshot_tables(now)
    S64 = snap["P"].astype(np.float64)[users] @ snap["Q"].astype(np.float64).T + float(now["mu"]) \
        + now["bu"].astype(np.float64)[users][:, None] + now["bi"].astype(np.float64)[None, :]
    tol = 1e-5 * np.abs(S64).max()
    for r in range(users.size):
        elig = np.ones(I, bool)
        elig[xrows[r]] = False
        for j, it in enumerate(trows[r]):
            g = int(second[tg[0][r] + j])
            if elig[it]:
                lo, hi = RC.rank_bracket(S64[r], elig, int(it), tol)
                assert lo <= g <= hi
            else:
                assert g == -1
    assert np.array_equal(m.rank_items(users, tg, exclude=ex), f32_now)         # unchanged by the snapshot calls
    m.close()


# ---------------------------------------------------------------- 7. evaluate_ranking(bf16=True)
def test_evaluate_ranking_bf16_end_to_end():
    rs = np.random.RandomState(12)
    U, I, D, N = 300, 400, 16, 20000
    m, t = make(U, I, D, rs)
    assert C.dyadic_faults(t) == []
    u = rs.randint(0, U, N)
    i = rs.randint(0, I, N)
    test = rs.rand(N) < 0.2
    train_x = T.rated_matrix(u[~test], i[~test], U, I)
    with pytest.raises(T.TfrError) as e:                       # no snapshot yet
        T.evaluate_ranking(m, u[test], i[test], exclude=train_x, ks=(10, 20), bf16=True)
    assert e.value.code == L.ERR_STATE
    m.snapshot_bf16()
    res = T.evaluate_ranking(m, u[test], i[test], exclude=train_x, ks=(10, 20), bf16=True)
    users = res["users"]
    tm = T.rated_matrix(u[test], i[test], U, I)
    assert np.array_equal(users, np.flatnonzero(np.diff(tm.indptr)))
    trows = [tm.indices[tm.indptr[x]:tm.indptr[x + 1]] for x in users]
    xrows = [train_x.indices[train_x.indptr[x]:train_x.indptr[x + 1]] for x in users]
    want = ref_ranks(m, t, users, trows, xrows)
    assert np.array_equal(res["ranks"], want)
    n_elig = np.array([I - np.unique(x).size for x in xrows])
    t_elig = np.array([np.setdiff1d(a, b).size for a, b in zip(trows, xrows)])
    wm = T.ranking_metrics(want, res["indptr"], n_elig, (10, 20), n_targets_eligible=t_elig)
    for k, v in wm.items():
        assert np.array_equal(np.nan_to_num(res[k], nan=-7), np.nan_to_num(v, nan=-7)), k
    f32 = T.evaluate_ranking(m, u[test], i[test], exclude=train_x, ks=(10, 20))
    assert np.array_equal(f32["ranks"], res["ranks"])      # exact tables: the same answer
    assert sorted(f32["mean"]) == sorted(res["mean"])
    assert all(f32["mean"][k] == res["mean"][k] or np.isnan(res["mean"][k]) for k in res["mean"])
    for k in ("recall@10", "ndcg@20", "mrr", "auc"):
        assert 0 <= res["mean"][k] <= 1
    m.close()
