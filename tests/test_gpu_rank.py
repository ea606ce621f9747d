"""Held-out ranking on the device (tfr_rank_items / tfr_fm_rank_items, SvdModel / FmModel.rank_items, evaluate_ranking)
against the NumPy statement of the contract (tests/rank_ref.py) and against tfr_topk itself."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests.rank_ref import rank_ref
from tests.topk_ref import svd_scores
from tests.test_gpu_topk import dyadic, make, random_excl
from tests import widths as W

pytestmark = pytest.mark.gpu

DIMS = [1, 5, 15, 16, 64, 128, 256]


def random_targets(rs, n, I, lo=0, hi=60):
    rows = [np.sort(rs.choice(I, min(I, rs.randint(lo, hi + 1)), replace=False)) for _ in range(n)]
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return (indptr, np.concatenate(rows).astype(np.int32)), rows


def excl_with_repeats(rs, n, I, trows, frac=0.2):
    """exclusion rows that repeat ids and take some of the row's targets"""
    rows = []
    for r in range(n):
        x = rs.randint(0, I, rs.randint(0, max(1, int(I * frac))))
        if trows[r].size:
            x = np.concatenate([x, rs.choice(trows[r], rs.randint(0, trows[r].size + 1))])
        x = np.sort(np.concatenate([x, x[: x.size // 3]]))
        rows.append(x)
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return (indptr, np.concatenate(rows).astype(np.int32)), rows


def ref_ranks(m, t, users, trows, xrows=None):
    S = svd_scores(t["P"], t["Q"], t["bu"], t["bi"], t["mu"], users, m.item_abs)
    return rank_ref(S, trows, xrows)


@pytest.mark.parametrize("D", sorted(set(DIMS) | set(W.RANK)))
def test_exact_on_dyadic_tables(D):
    rs = np.random.RandomState(100 + D)
    U, I = 70, 900
    for item_abs in (False, True):
        m, t = make(U, I, D, rs, item_abs=item_abs)
        users = rs.randint(0, U, 40).astype(np.int32)
        tg, trows = random_targets(rs, users.size, I)
        for with_excl in (False, True):
            ex, xrows = excl_with_repeats(rs, users.size, I, trows) if with_excl else (None, None)
            got = m.rank_items(users, tg, exclude=ex)
            want = ref_ranks(m, t, users, trows, xrows)
            assert np.array_equal(got, want), (D, item_abs, with_excl)
        m.close()


@pytest.mark.parametrize("D", sorted(set(DIMS) | set(W.RANK_RANDOM)))
def test_rank_is_position_in_recommend_on_random_tables(D):
    rs = np.random.RandomState(200 + D)
    U, I, K = 50, 2000, 256
    for item_abs in (False, True):
        m, t = make(U, I, D, rs, dyad=False, item_abs=item_abs)
        users = rs.randint(0, U, 30).astype(np.int32)
        items, _ = m.recommend(users, K)
        # targets: most of the top-K list, plus random items below it
        trows = [np.unique(np.concatenate([items[r][rs.rand(K) < 0.7], rs.randint(0, I, 40)])) for r in range(users.size)]
        indptr = np.concatenate([[0], np.cumsum([r.size for r in trows])]).astype(np.int64)
        ex, xrows = excl_with_repeats(rs, users.size, I, trows, 0.05)
        for exclude in (None, ex):
            got = m.rank_items(users, (indptr, np.concatenate(trows).astype(np.int32)), exclude=exclude)
            rec, _ = m.recommend(users, K, exclude=exclude)
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


def test_bit_identical_across_batches_chunks_and_order():
    rs = np.random.RandomState(4)
    U, I, D = 300, 500, 64
    m, t = make(U, I, D, rs, dyad=False)
    lds, ppb, sl, cap, ch = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    n3 = 70000
    L.check(L.load().tfr_rank_plan(D, n3, n3, I, C.byref(lds), C.byref(ppb), C.byref(sl), C.byref(cap), C.byref(ch)))
    assert n3 > 2 * ch.value
    u0 = np.int32(17)
    t0 = np.sort(rs.choice(I, 25, replace=False)).astype(np.int32)
    x0 = np.sort(rs.choice(I, 40, replace=False)).astype(np.int32)

    def alone_row(users, pos):
        n = users.size
        tl = [t0 if r in pos else rs.choice(I, 1).astype(np.int32) for r in range(n)]
        xl = [x0 if r in pos else np.zeros(0, np.int32) for r in range(n)]
        ti = np.concatenate([[0], np.cumsum([a.size for a in tl])]).astype(np.int64)
        xi = np.concatenate([[0], np.cumsum([a.size for a in xl])]).astype(np.int64)
        got = m.rank_items(users, (ti, np.concatenate(tl)), exclude=(xi, np.concatenate(xl)))
        return [got[ti[r]:ti[r + 1]] for r in pos]

    alone = m.rank_items([u0], (np.array([0, t0.size]), t0), exclude=(np.array([0, x0.size]), x0))
    big = rs.randint(0, U, 5000).astype(np.int32)
    big[[5, 999, 4321]] = u0
    huge = rs.randint(0, U, n3).astype(np.int32)
    pos = [3, int(ch.value) + 11, 2 * int(ch.value) + 50]
    huge[pos] = u0
    for rows in (alone_row(big, [5, 999, 4321]), alone_row(huge, pos)):
        for g in rows:
            assert np.array_equal(g, alone)
    # row order: the same request reversed gives the same ranks per row
    users = rs.randint(0, U, 200).astype(np.int32)
    tg, trows = random_targets(rs, users.size, I, 1, 30)
    got = m.rank_items(users, tg)
    rev = users[::-1].copy()
    trev = trows[::-1]
    ip = np.concatenate([[0], np.cumsum([r.size for r in trev])]).astype(np.int64)
    grev = m.rank_items(rev, (ip, np.concatenate(trev).astype(np.int32)))
    for r in range(users.size):
        rr = users.size - 1 - r
        assert np.array_equal(got[tg[0][r]:tg[0][r + 1]], grev[ip[rr]:ip[rr + 1]])
    # targets given in any order within a row come back aligned with the caller's order
    perm_items = tg[1].copy()
    for r in range(users.size):
        seg = perm_items[tg[0][r]:tg[0][r + 1]]
        rs.shuffle(seg)
    gperm = m.rank_items(users, (tg[0], perm_items))
    lut = {(r, int(i)): int(g) for r in range(users.size) for i, g in zip(trows[r], got[tg[0][r]:tg[0][r + 1]])}
    for r in range(users.size):
        for i, g in zip(perm_items[tg[0][r]:tg[0][r + 1]], gperm[tg[0][r]:tg[0][r + 1]]):
            assert lut[(r, int(i))] == g
    m.close()


def test_pieces_all_excluded_and_empty_rows():
    rs = np.random.RandomState(5)
    U, I, D = 20, 4000, 16
    m, t = make(U, I, D, rs)
    many = np.sort(rs.choice(I, 3000, replace=False))       # > RANK_CAP: 24 pieces
    some = np.sort(rs.choice(I, 30, replace=False))
    trows = [many, some, np.zeros(0, np.int64), some, np.arange(I)]
    xrows = [np.sort(rs.choice(I, 500)), some.copy(), np.arange(10), np.zeros(0, np.int64), np.zeros(0, np.int64)]
    users = np.array([3, 4, 5, 6, 7], np.int32)
    ti = np.concatenate([[0], np.cumsum([a.size for a in trows])]).astype(np.int64)
    xi = np.concatenate([[0], np.cumsum([a.size for a in xrows])]).astype(np.int64)
    got = m.rank_items(users, (ti, np.concatenate(trows).astype(np.int32)), exclude=(xi, np.concatenate(xrows).astype(np.int32)))
    want = ref_ranks(m, t, users, trows, xrows)
    assert np.array_equal(got, want)
    assert np.all(got[ti[1]:ti[2]] == -1)                   # every target excluded
    assert np.array_equal(np.sort(got[ti[4]:ti[5]]), np.arange(I))   # the whole catalogue: a permutation of ranks
    assert m.rank_items([1, 2], (np.array([0, 0, 0]), np.zeros(0, np.int32))).size == 0
    assert m.rank_items(np.zeros(0, np.int32), (np.array([0]), np.zeros(0, np.int32))).size == 0
    m.close()


def test_nan_rows():
    rs = np.random.RandomState(6)
    U, I, D = 10, 700, 16
    m, t = make(U, I, D, rs)
    P, Q = t["P"].copy(), t["Q"].copy()
    P[2] = np.nan
    Q[[7, 300]] = np.nan
    m.set_table(L.P, P)
    m.set_table(L.Q, Q)
    t = dict(t, P=P, Q=Q)
    users = np.array([0, 2, 5], np.int32)
    trows = [np.array([1, 7, 300, 650]), np.array([1, 7, 650]), np.arange(0, I, 3)]
    ti = np.concatenate([[0], np.cumsum([a.size for a in trows])]).astype(np.int64)
    got = m.rank_items(users, (ti, np.concatenate(trows).astype(np.int32)))
    assert np.array_equal(got, ref_ranks(m, t, users, trows))
    assert got[1] == -1 and got[2] == -1 and np.all(got[4:7] == -1)
    assert np.sort(got[7:][got[7:] >= 0]).max() < I - 2     # the NaN items are never counted
    m.close()


def test_after_two_table_step_and_state_untouched():
    rs = np.random.RandomState(8)
    U, I, D, B = 40000, 30000, 64, 20000              # the shape test_gpu_parity's two-table test trains at
    m = T.SvdModel(U, I, D, adam_mode="lazy", lr=3e-3)
    m.init_tables(seed=3, feature_stddev=0.3, bias_stddev=0.5)
    hot = rs.randint(0, I, 400)
    for _ in range(3):
        i = np.where(rs.rand(B) < 0.6, hot[rs.randint(0, 400, B)], rs.randint(0, I, B)).astype(np.int32)
        m.train_step(rs.randint(0, U, B), i, rs.randint(1, 6, B).astype(np.float32), want_logits=False)
    users = rs.randint(0, U, 33).astype(np.int32)
    rec, _ = m.recommend(users, 50)
    trows = [np.unique(np.concatenate([rec[r][:30], hot[:5]])) for r in range(users.size)]
    ti = np.concatenate([[0], np.cumsum([a.size for a in trows])]).astype(np.int64)
    ids = [L.MU, L.BU, L.BI, L.P, L.Q] + [w | s for w in (L.MU, L.BU, L.BI, L.P, L.Q) for s in (L.SLOT_M, L.SLOT_V)]
    m.sync()
    before = {w: m.get_table(w).copy() for w in ids}
    step = m.get_step()
    got = m.rank_items(users, (ti, np.concatenate(trows).astype(np.int32)))
    for w in ids:
        assert np.array_equal(m.get_table(w).view(np.uint32), before[w].view(np.uint32)), w
    assert m.get_step() == step
    for r in range(users.size):
        pos = {int(i): p for p, i in enumerate(rec[r])}
        for j, it in enumerate(trows[r]):
            g = int(got[ti[r] + j])
            assert g == pos[int(it)] if int(it) in pos else g >= 50
    m.close()


def test_errors_leave_output_untouched():
    rs = np.random.RandomState(9)
    m, t = make(20, 30, 16, rs)
    lib = L.load()
    out = np.full(3, 77, np.int32)
    u = np.array([0, 1], np.int32)
    ip = np.array([0, 2, 3], np.int64)

    def call(users, tip, tit, xip=None, xit=None):
        return lib.tfr_rank_items(m._h, L.ptr_i32(users), users.size, L.ptr_i64(tip), L.ptr_i32(tit),
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
    assert np.all(out == 77)
    with pytest.raises(L.OutOfRangeError):
        m.rank_items([0, 20], (ip, tit))
    with pytest.raises(ValueError):
        m.rank_items([0, 1], (ip, np.array([2, 2, 3], np.int32)))
    got = m.rank_items(u, (ip, tit))
    assert np.array_equal(got, ref_ranks(m, t, u, [tit[:2], tit[2:]]))
    m.close()


@pytest.mark.parametrize("dyad", [True, False])
def test_fm_rank_items(dyad):
    _check_fm_rank_items(dyad, 16)


@pytest.mark.parametrize("dyad", [True, False])
@pytest.mark.parametrize("D", W.FM_TOPK)
def test_fm_rank_items_at_other_widths(dyad, D):
    _check_fm_rank_items(dyad, D)


def _check_fm_rank_items(dyad, D):
    from tests.test_gpu_topk import fm_two_hot
    rs = np.random.RandomState(10)
    Un, In = 40, 500
    F = Un + In
    fm = T.FmModel(F, D)
    if dyad:
        W, V, mu = dyadic(rs, F, .25), dyadic(rs, (F, D), .125), 0.5
    else:
        W, V, mu = rs.normal(0, .3, F).astype(np.float32), rs.normal(0, .3, (F, D)).astype(np.float32), 0.1
    fm.set(mu, W, V)
    users = np.array([0, 7, 39, 7], np.int32)
    tg, trows = random_targets(rs, users.size, In, 1, 80)
    ex, xrows = excl_with_repeats(rs, users.size, In, trows)
    got = fm.rank_items(users, Un, Un + In, tg, exclude=ex)
    if dyad:
        S = np.stack([fm.fma(fm_two_hot(int(u), Un, In)) for u in users])
        assert np.array_equal(got, rank_ref(S, trows, xrows))
    items, _ = fm.topk(users, Un, Un + In, 256, exclude=ex)
    for r in range(users.size):
        pos = {int(i): p for p, i in enumerate(items[r])}
        for j, it in enumerate(trows[r]):
            g = int(got[tg[0][r] + j])
            if int(it) in pos:
                assert g == pos[int(it)]
            elif int(it) in set(xrows[r].tolist()):
                assert g == -1
            else:
                assert g >= 256
    m = T.evaluate_ranking(fm, users, np.array([tg[1][0], tg[1][-1], 3, 4]), ks=(5,), item_lo=Un, item_hi=Un + In)
    assert np.isfinite(m["mean"]["recall@5"])
    fm.close()


def test_evaluate_ranking_end_to_end():
    rs = np.random.RandomState(12)
    U, I, D, N = 300, 400, 16, 20000
    m, t = make(U, I, D, rs)
    u = rs.randint(0, U, N)
    i = rs.randint(0, I, N)
    test = rs.rand(N) < 0.2
    train_x = T.rated_matrix(u[~test], i[~test], U, I)
    res = T.evaluate_ranking(m, u[test], i[test], exclude=train_x, ks=(10, 20))
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
    for k in ("recall@10", "ndcg@20", "mrr", "auc"):
        assert 0 <= res["mean"][k] <= 1


def test_large_shape_against_float64():
    rs = np.random.RandomState(11)
    U, I, D = 5000, 1 << 20, 64
    m = T.SvdModel(U, I, D)
    t = dict(mu=np.float32(0.1), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
             P=rs.normal(0, .3, (U, D)).astype(np.float32), Q=rs.normal(0, .3, (I, D)).astype(np.float32))
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    users = rs.randint(0, U, 4096).astype(np.int32)
    tg, trows = random_targets(rs, users.size, I, 32, 32)
    ex, xrows = random_excl(rs, users.size, I, 200 / I)
    got = m.rank_items(users, tg, exclude=ex)
    P, Q = np.asarray(t["P"], np.float64), np.asarray(t["Q"], np.float64)
    for r in rs.choice(users.size, 16, replace=False):
        s64 = P[users[r]] @ Q.T + 0.1 + float(t["bu"][users[r]]) + np.asarray(t["bi"], np.float64)
        scale = np.abs(s64).max()
        elig = np.ones(I, bool)
        elig[xrows[r]] = False
        for j, it in enumerate(trows[r]):
            g = int(got[tg[0][r] + j])
            if not elig[it]:
                assert g == -1
                continue
            lo = np.count_nonzero(elig & (s64 > s64[it] + 1e-5 * scale))
            hi = np.count_nonzero(elig & (s64 >= s64[it] - 1e-5 * scale)) - 1
            assert lo <= g <= hi, (r, it, g, lo, hi)
    m.close()
