"""Top-K recommendation on the device (tfr_topk / tfr_topk_dev / tfr_fm_topk) against the NumPy statement of the contract."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests.topk_ref import svd_scores, topk_ref, csr_rows
from tests import widths as W

pytestmark = pytest.mark.gpu


def dyadic(rs, shape, step):
    return (rs.randint(-int(1 / step), int(1 / step) + 1, shape) * step).astype(np.float32)


def make(U, I, D, rs, dyad=True, **kw):
    m = T.SvdModel(U, I, D, **kw)
    if dyad:
        t = dict(mu=np.float32(0.25), bu=dyadic(rs, U, .25), bi=dyadic(rs, I, .25), P=dyadic(rs, (U, D), .125),
                 Q=dyadic(rs, (I, D), .125))
    else:
        t = dict(mu=np.float32(0.1), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
                 P=rs.normal(0, .3, (U, D)).astype(np.float32), Q=rs.normal(0, .3, (I, D)).astype(np.float32))
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    return m, t


def ref_for(m, t, users, k, excl=None):
    S = svd_scores(t["P"], t["Q"], t["bu"], t["bi"], t["mu"], users, m.item_abs)
    return topk_ref(S, k, excl)


def random_excl(rs, n, I, frac=0.2):
    rows = [np.unique(rs.randint(0, I, rs.randint(0, max(1, int(I * frac))))) for _ in range(n)]
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return (indptr, np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)), rows


@pytest.mark.parametrize("D", sorted({1, 5, 15, 16, 64, 128, 256} | set(W.TOPK)))
def test_exact_on_dyadic_tables(D):
    rs = np.random.RandomState(D)
    U, I = 70, 900
    for item_abs in (False, True):
        m, t = make(U, I, D, rs, item_abs=item_abs)
        users = rs.randint(0, U, 40).astype(np.int32)
        for k in W.TOPK_KS:
            for with_excl in (False, True):
                ex, rows = random_excl(rs, users.size, I) if with_excl else (None, None)
                items, scores = m.recommend(users, k, exclude=ex)
                wi, ws = ref_for(m, t, users, k, rows)
                assert np.array_equal(items, wi), (D, k, item_abs, with_excl)
                assert np.array_equal(scores.view(np.uint32), ws.view(np.uint32)), (D, k, item_abs, with_excl)
        m.close()


def check_oracle(m, t, users, items, scores, k, rows, tol=1e-5):
    P, Q = np.asarray(t["P"], np.float64), np.asarray(t["Q"], np.float64)
    S64 = P[users] @ (np.abs(Q) if m.item_abs else Q).T + float(t["mu"]) + np.asarray(t["bu"], np.float64)[users][:, None] \
        + np.asarray(t["bi"], np.float64)[None, :]
    scale = np.abs(S64).max()
    for r in range(users.size):
        it = items[r]
        assert len(set(it.tolist())) == k
        if rows is not None:
            assert not set(it.tolist()) & set(rows[r].tolist())
        s = scores[r]
        assert np.all(s[:-1] >= s[1:])
        eq = s[:-1] == s[1:]
        assert np.all(it[:-1][eq] < it[1:][eq])
        elig = np.ones(S64.shape[1], bool)
        if rows is not None:
            elig[rows[r]] = False
        kth = np.sort(S64[r][elig])[::-1][k - 1]
        assert np.all(S64[r, it] >= kth - tol * scale)
        assert np.all(np.abs(s - S64[r, it]) <= tol * scale)
    return True


def test_random_tables_ml1m_shape():
    rs = np.random.RandomState(3)
    U, I, D, k = 6040, 3706, 64, 10
    m, t = make(U, I, D, rs, dyad=False)
    users = np.arange(0, U, 7, dtype=np.int32)
    ex, rows = random_excl(rs, users.size, I, 0.05)
    items, scores = m.recommend(users, k, exclude=ex)
    check_oracle(m, t, users, items, scores, k, rows)
    fw = m.forward(np.repeat(users, k), items.reshape(-1)).reshape(users.size, k)
    scale = np.abs(scores).max()
    assert np.abs(fw - scores).max() <= 1e-5 * scale
    m.close()


def test_bit_identical_across_batches_and_chunks():
    rs = np.random.RandomState(4)
    U, I, D, k = 300, 200, 64, 10
    m, t = make(U, I, D, rs, dyad=False)
    lds, upb, sl, ch = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
    n3 = 2 * 65536 + 100
    L.check(L.load().tfr_topk_plan(D, k, n3, I, C.byref(lds), C.byref(upb), C.byref(sl), C.byref(ch)))
    assert n3 > 2 * ch.value
    u0 = np.int32(17)
    alone = m.recommend([u0], k)
    b7 = np.array([3, u0, 9, 250, u0, 0, 299], np.int32)
    in7 = m.recommend(b7, k)
    big = rs.randint(0, U, 5000).astype(np.int32)
    big[[5, 999, 4321]] = u0
    in5000 = m.recommend(big, k)
    huge = rs.randint(0, U, n3).astype(np.int32)
    pos = [3, ch.value + 11, 2 * ch.value + 50]
    huge[pos] = u0
    inhuge = m.recommend(huge, k)
    for it, sc in [(in7[0][[1, 4]], in7[1][[1, 4]]), (in5000[0][[5, 999, 4321]], in5000[1][[5, 999, 4321]]),
                   (inhuge[0][pos], inhuge[1][pos])]:
        for r in range(it.shape[0]):
            assert np.array_equal(it[r], alone[0][0])
            assert np.array_equal(sc[r].view(np.uint32), alone[1][0].view(np.uint32))
    # every row of the three-chunk request equals the same user asked alone in a small batch
    uniq = np.unique(huge[:64])
    ref = m.recommend(uniq, k)
    lut = {int(u): r for r, u in enumerate(uniq)}
    for r in range(64):
        assert np.array_equal(inhuge[0][r], ref[0][lut[int(huge[r])]])
    m.close()


def test_edges():
    rs = np.random.RandomState(5)
    m, t = make(20, 30, 16, rs)
    items, scores = m.recommend([0, 1], 40)
    wi, ws = ref_for(m, t, np.array([0, 1]), 40)
    assert np.array_equal(items, wi) and np.all(items[:, 30:] == -1) and np.all(scores[:, 30:] == -np.inf)
    allx = (np.array([0, 30, 30], np.int64), np.arange(30, dtype=np.int32))
    items, scores = m.recommend([2, 3], 5, exclude=allx)
    assert np.all(items[0] == -1) and np.all(scores[0] == -np.inf) and np.all(items[1] >= 0)
    items, scores = m.recommend(np.zeros(0, np.int32), 5)
    assert items.shape == (0, 5)
    bi = t["bi"].copy()
    Q = t["Q"].copy()
    Q[7] = np.nan
    bi[11] = np.inf
    m.set_table(L.Q, Q)
    m.set_table(L.BI, bi)
    items, scores = m.recommend(np.arange(20, dtype=np.int32), 30)
    assert np.all(items[:, 0] == 11) and np.all(scores[:, 0] == np.inf)
    assert not np.any(items == 7) and np.all(items[:, 29] == -1)
    m.close()
    m1, t1 = make(5, 1, 8, rs)
    items, scores = m1.recommend([0, 4], 3)
    assert np.all(items[:, 0] == 0) and np.all(items[:, 1:] == -1)
    m1.close()


def test_errors_and_model_still_works():
    rs = np.random.RandomState(6)
    m, t = make(20, 30, 16, rs)
    lib = L.load()
    items = np.full((2, 4), 77, np.int32)
    u = np.array([0, 20], np.int32)
    assert lib.tfr_topk(m._h, L.ptr_i32(u), 2, 4, None, None, L.ptr_i32(items), None) == L.ERR_OOB
    assert np.all(items == 77)
    u = np.array([0, 1], np.int32)
    ip, bad = np.array([0, 1, 2], np.int64), np.array([3, 30], np.int32)
    assert lib.tfr_topk(m._h, L.ptr_i32(u), 2, 4, L.ptr_i64(ip), L.ptr_i32(bad), L.ptr_i32(items), None) == L.ERR_OOB
    ip, uns = np.array([0, 0, 2], np.int64), np.array([5, 3], np.int32)
    assert lib.tfr_topk(m._h, L.ptr_i32(u), 2, 4, L.ptr_i64(ip), L.ptr_i32(uns), L.ptr_i32(items), None) == L.ERR_ARG
    assert np.all(items == 77)
    assert lib.tfr_topk(m._h, L.ptr_i32(u), 2, 0, None, None, L.ptr_i32(items), None) == L.ERR_ARG
    assert lib.tfr_topk(m._h, L.ptr_i32(u), 2, 257, None, None, L.ptr_i32(items), None) == L.ERR_ARG
    import torch
    dev = torch.device("cuda", 0)
    du = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    with pytest.raises(L.TfrError) as e:
        m.recommend_dev(du, 4, exclude=(torch.tensor([0, 0, 2], device=dev), torch.tensor([5, 3], dtype=torch.int32, device=dev)))
        m.sync()
    assert e.value.code == L.ERR_ARG
    with pytest.raises(L.OutOfRangeError):
        m.recommend_dev(du, 4, exclude=(torch.tensor([0, 1, 2], device=dev), torch.tensor([3, 30], dtype=torch.int32, device=dev)))
        m.sync()
    with pytest.raises(L.OutOfRangeError):
        m.recommend_dev(torch.tensor([0, 25], dtype=torch.int32, device=dev), 4)
        m.sync()
    items, scores = m.recommend([0, 1], 4)
    wi, ws = ref_for(m, t, np.array([0, 1]), 4)
    assert np.array_equal(items, wi) and np.array_equal(scores, ws)
    logits, _, _ = m.train_step([0, 1], [2, 3], [1.0, 2.0])
    assert np.all(np.isfinite(logits))
    m.close()


def test_state_untouched_and_training_unchanged():
    rs = np.random.RandomState(7)
    U, I, D = 200, 300, 32
    batches = [(rs.randint(0, U, 500), rs.randint(0, I, 500), rs.randint(1, 6, 500).astype(np.float32)) for _ in range(4)]
    res = []
    for interleave in (False, True):
        m, t = make(U, I, D, np.random.RandomState(70), dyad=False, adam_mode="lazy")
        for b, (u, i, r) in enumerate(batches):
            m.train_step(u, i, r)
            if interleave:
                ids = [L.MU, L.BU, L.BI, L.P, L.Q] + [w | s for w in (L.MU, L.BU, L.BI, L.P, L.Q) for s in (L.SLOT_M, L.SLOT_V)]
                before = {w: m.get_table(w).copy() for w in ids}
                step = m.get_step()
                m.recommend(np.arange(0, U, 3), 20, exclude=T.rated_matrix(u, i, U, I))
                for w in ids:
                    assert np.array_equal(m.get_table(w).view(np.uint32), before[w].view(np.uint32)), w
                assert m.get_step() == step
        res.append({w: m.get_table(w) for w in (L.MU, L.BU, L.BI, L.P, L.Q)})
        m.close()
    for w in res[0]:
        assert np.array_equal(res[0][w].view(np.uint32), res[1][w].view(np.uint32))


def test_sees_rows_of_the_fused_big_table_step():
    rs = np.random.RandomState(8)
    U, I, D, B = 40000, 30000, 64, 20000              # the shape test_gpu_parity's two-table test trains at
    m = T.SvdModel(U, I, D, adam_mode="lazy", lr=3e-3)
    m.init_tables(seed=3, feature_stddev=0.3, bias_stddev=0.5)
    hot = rs.randint(0, I, 400)
    for _ in range(3):
        i = np.where(rs.rand(B) < 0.6, hot[rs.randint(0, 400, B)], rs.randint(0, I, B)).astype(np.int32)
        m.train_step(rs.randint(0, U, B), i, rs.randint(1, 6, B).astype(np.float32), want_logits=False)
    users = rs.randint(0, U, 33).astype(np.int32)
    items, scores = m.recommend(users, 10)
    t = dict(mu=m.get_table(L.MU), bu=m.get_table(L.BU), bi=m.get_table(L.BI), P=m.get_table(L.P), Q=m.get_table(L.Q))
    check_oracle(m, t, users, items, scores, 10, None)
    m.close()


def test_device_variant_equals_host():
    import torch
    rs = np.random.RandomState(9)
    U, I = 500, 2000
    m, t = make(U, I, 64, rs, dyad=False)
    users = rs.randint(0, U, 300).astype(np.int32)
    ex, rows = random_excl(rs, users.size, I)
    hi, hs = m.recommend(users, 25, exclude=ex)
    dev = torch.device("cuda", 0)
    di, ds = m.recommend_dev(torch.from_numpy(users).to(dev), 25,
                             exclude=(torch.from_numpy(ex[0]).to(dev), torch.from_numpy(ex[1]).to(dev)))
    m.sync()
    assert np.array_equal(di.cpu().numpy(), hi)
    assert np.array_equal(ds.cpu().numpy().view(np.uint32), hs.view(np.uint32))
    m.close()


def fm_two_hot(user, user_num, item_num):
    rows = np.arange(item_num)
    data = np.ones(2 * item_num, np.float32)
    X = sp.csr_matrix((data, (np.concatenate([rows, rows]), np.concatenate([np.full(item_num, user), user_num + rows]))),
                      shape=(item_num, user_num + item_num))
    return X


@pytest.mark.parametrize("dyad", [True, False])
def test_fm_get_ranking(dyad):
    _check_fm_get_ranking(dyad, 16)


@pytest.mark.parametrize("dyad", [True, False])
@pytest.mark.parametrize("D", W.FM_TOPK)
def test_fm_get_ranking_at_other_widths(dyad, D):
    _check_fm_get_ranking(dyad, D)


def _check_fm_get_ranking(dyad, D):
    rs = np.random.RandomState(10)
    Un, In = 40, 500
    F = Un + In
    fm = T.FmModel(F, D)
    if dyad:
        W, V, mu = dyadic(rs, F, .25), dyadic(rs, (F, D), .125), 0.5
    else:
        W, V, mu = rs.normal(0, .3, F).astype(np.float32), rs.normal(0, .3, (F, D)).astype(np.float32), 0.1
    fm.set(mu, W, V)
    for user in (0, 7, 39):
        items, scores = fm.get_ranking(user, Un, In, k=50)
        y = fm.fma(fm_two_hot(user, Un, In))
        if dyad:
            wi, ws = topk_ref(y[None, :], 50)
            assert np.array_equal(items, wi[0]) and np.array_equal(scores, ws[0])
        else:
            y64 = np.sort(y.astype(np.float64))[::-1]
            assert np.all(y[items] >= y64[49] - 1e-5 * np.abs(y).max())
            assert np.abs(scores - y[items]).max() <= 1e-5 * np.abs(y).max()
    ex = sp.csr_matrix((np.ones(3), ([7, 7, 7], [1, 5, 9])), shape=(Un, In))
    items, _ = fm.topk([7], Un, Un + In, 20, exclude=ex)
    assert not set(items[0].tolist()) & {1, 5, 9}
    fm.close()


def test_large_shape():
    rs = np.random.RandomState(11)
    U, I, D, k = 5000, 1 << 20, 64, 100
    m = T.SvdModel(U, I, D)
    t = dict(mu=np.float32(0.1), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
             P=rs.normal(0, .3, (U, D)).astype(np.float32), Q=rs.normal(0, .3, (I, D)).astype(np.float32))
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    users = rs.randint(0, U, 4096).astype(np.int32)
    items, scores = m.recommend(users, k)
    sample = rs.choice(4096, 64, replace=False)
    check_oracle(m, t, users[sample], items[sample], scores[sample], k, None)
    m.close()
