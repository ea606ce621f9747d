"""SVD++ on the device (tfr_svdpp_*) against the float64 restatement in tests/svdpp_ref.py."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from oracle import svd_oracle as so
from tests import svdpp_ref as R
from tests import widths as W

pytestmark = pytest.mark.gpu

ORDER = (R.MU, R.BU, R.BI, R.PF, R.QF, R.YF)


def implicit(U, I, rs, long_users=(), long_len=0, empty=(0,), hot_item=None, hot_users=()):
    rows = []
    for u in range(U):
        if u in empty:
            s = np.zeros(0, np.int64)
        elif u in long_users:
            s = np.sort(rs.choice(I, long_len, replace=False))
        else:
            s = np.sort(rs.choice(I, rs.randint(1, 30), replace=False))
        if hot_item is not None:
            s = np.setdiff1d(s, [hot_item])
            if u in hot_users:
                s = np.union1d(s, [hot_item])
        rows.append(s)
    indptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def tables(U, I, D, rs, scale=0.3):
    f = lambda *s: rs.normal(0, scale, s).astype(np.float32)
    return {R.MU: np.float32(0.2), R.BU: f(U), R.BI: f(I), R.PF: f(U, D), R.QF: f(I, D), R.YF: f(I, D)}


def model(U, I, D, t, N, **kw):
    m = T.SvdppModel(U, I, D, **kw)
    m.set_tables(*(t[k] for k in ORDER))
    m.set_implicit(N)
    return m


def f64(t):
    return {k: np.array(v, np.float64) for k, v in t.items()}


def got_tables(m):
    g = m.tables()
    return {k: np.asarray(g[k], np.float64) for k in ORDER}


@pytest.mark.parametrize("D", sorted({1, 5, 16, 64, 128, 256} | set(W.SVDPP)))
@pytest.mark.parametrize("item_abs", [False, True])
def test_forward_matches_reference(D, item_abs):
    rs = np.random.RandomState(D + 7 * item_abs)
    U, I, B = 40, 3000, 500
    N = implicit(U, I, rs, long_users=(1, 2), long_len=2900)
    t = tables(U, I, D, rs)
    u = np.concatenate(([0, 1, 2], rs.randint(0, U, B - 3))).astype(np.int32)
    i = rs.randint(0, I, B).astype(np.int32)
    with model(U, I, D, t, N, item_abs=item_abs) as m:
        x = m.forward(u, i)
    want = R.forward(f64(t), N[0], N[1], u, i, item_abs)
    np.testing.assert_allclose(x, want, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(want).max()))


GRAD_CASES = [("mse", False, False), ("nll", True, True), ("mse", True, False)]


@pytest.mark.parametrize("loss,item_abs,reg_bias", GRAD_CASES)
def test_one_step_gradients_of_all_six_tables(loss, item_abs, reg_bias):
    """SGD with lr = 1: every table moves by exactly minus its gradient; hot Y rows (a column over several pieces) included."""
    _one_step_gradients(16, loss, item_abs, reg_bias)


@pytest.mark.parametrize("D", W.SVDPP)
def test_one_step_gradients_at_every_register_width(D):
    """the same at every NJ = ceil(D / 64), last register full and partial: k_pp_users (TRAIN), k_pp_items, k_pp_ygrad and
    k_pp_yapply at every instantiation; the loss form rotates across the widths"""
    _one_step_gradients(D, *GRAD_CASES[W.SVDPP.index(D) % len(GRAD_CASES)])


def _one_step_gradients(D, loss, item_abs, reg_bias):
    rs = np.random.RandomState(3)
    U, I, B = 600, 200, 3000
    N = implicit(U, I, rs, long_users=(5,), long_len=190, hot_item=11, hot_users=tuple(range(1, 600, 2)))
    t = tables(U, I, D, rs, 0.2)
    u = rs.randint(0, U, B).astype(np.int32)
    i = rs.randint(0, I, B).astype(np.int32)
    r = (rs.randint(0, 2, B) if loss == "nll" else rs.randint(1, 6, B)).astype(np.float32)
    lam = 0.05
    with model(U, I, D, t, N, loss=loss, item_abs=item_abs, reg_bias=reg_bias, optimizer="sgd", lr=1.0, reg=lam) as m:
        logits, lossv, regv = m.train_step(u, i, r)
        after = got_tables(m)
    t64 = f64(t)
    G = R.gradients(t64, N[0], N[1], u, i, r.astype(np.float64), loss, item_abs, reg_bias, lam)
    x = R.forward(t64, N[0], N[1], u, i, item_abs)
    np.testing.assert_allclose(logits, x, rtol=1e-5, atol=1e-5)
    assert lossv == pytest.approx(so.data_loss(x, r.astype(np.float64), loss), rel=1e-4)
    assert regv == pytest.approx(R.regularizer(t64, N[0], N[1], u, i, reg_bias), rel=1e-4)
    for k in ORDER:
        g = t64[k] - after[k]
        scale = max(1.0, np.abs(G[k]).max())
        np.testing.assert_allclose(g, G[k], rtol=1e-4, atol=1e-4 * scale, err_msg="table %d" % k)
    assert np.abs(G[R.YF][11]).max() > 0                        # the hot row was touched


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("loss,reg_bias", [("mse", False), ("nll", True)])
def test_trajectory_of_twenty_steps(optimizer, loss, reg_bias):
    _trajectory(32, optimizer, loss, reg_bias)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("D", W.SVDPP)
def test_trajectory_at_every_register_width(D, optimizer):
    """both optimisers at every NJ, last register full and partial; the loss alternates across the widths"""
    loss, reg_bias = [("mse", False), ("nll", True)][W.SVDPP.index(D) % 2]
    _trajectory(D, optimizer, loss, reg_bias)


def _trajectory(D, optimizer, loss, reg_bias):
    rs = np.random.RandomState(11)
    U, I, B = 300, 250, 800
    N = implicit(U, I, rs, long_users=(3,), long_len=200)
    t = tables(U, I, D, rs, 0.1)
    lr = 1e-4 if optimizer == "sgd" else 1e-3              # SGD sums the batch: lr * B stays below one
    kw = dict(loss=loss, reg_bias=reg_bias, optimizer=optimizer, lr=lr, reg=0.05)
    refs = {dt: R.SvdppRef(U, I, D, N[0], N[1], dtype=dt, **kw) for dt in (np.float64, np.float32)}
    for ref in refs.values():
        ref.set_tables(t)
    with model(U, I, D, t, N, **kw) as m:
        for s in range(20):
            u = rs.randint(0, U, B).astype(np.int32)
            i = rs.randint(0, I, B).astype(np.int32)
            r = (rs.randint(0, 2, B) if loss == "nll" else rs.randint(1, 6, B)).astype(np.float32)
            m.train_step(u, i, r, want_logits=False)
            for ref in refs.values():
                ref.train_step(u, i, r)
        got = got_tables(m)
        assert m.step == 20
    for k in ORDER:
        truth = np.asarray(refs[np.float64].t[k], np.float64)
        e_gpu = np.abs(got[k] - truth).max()
        e_f32 = np.abs(np.asarray(refs[np.float32].t[k], np.float64) - truth).max()
        assert e_gpu <= 2 * e_f32 + 1e-6 * max(1.0, np.abs(truth).max()), (k, e_gpu, e_f32)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_zero_frozen_y_matches_the_svd_model(optimizer):
    rs = np.random.RandomState(5)
    U, I, D, B = 400, 300, 64, 2000
    N = implicit(U, I, rs)
    t = tables(U, I, D, rs, 0.2)
    t[R.YF][...] = 0
    kw = dict(optimizer=optimizer, adam_mode="lazy", lr=1e-4 if optimizer == "sgd" else 1e-3, reg=0.05)
    with model(U, I, D, t, N, **kw) as m, T.SvdModel(U, I, D, **kw) as s:
        m.set_frozen(1 << L.Y)
        s.set_tables(*(t[k] for k in ORDER[:5]))
        for _ in range(5):
            u = rs.randint(0, U, B).astype(np.int32)
            i = rs.randint(0, I, B).astype(np.int32)
            r = rs.randint(1, 6, B).astype(np.float32)
            a = m.train_step(u, i, r)
            b = s.train_step(u, i, r)
            np.testing.assert_allclose(a[0], b[0], rtol=1e-5, atol=1e-5)
        ga, gb = m.tables(), s.tables()
    for k in ORDER[:5]:
        np.testing.assert_allclose(ga[k], gb[k], rtol=1e-5, atol=1e-6, err_msg="table %d" % k)
    assert not ga[L.Y].any()


def _isolation_run(t, N, dims, batch, dev=False):
    import torch
    U, I, D = dims
    with model(U, I, D, t, N, optimizer="adam", lr=1e-3, reg=0.05) as m:
        u, i, r = batch
        if dev:
            d = torch.device("cuda")
            logits = m.train_step_dev(torch.from_numpy(u).to(d), torch.from_numpy(i).to(d), torch.from_numpy(r).to(d),
                                      want_logits=True)
            m.sync()
            logits = logits.cpu().numpy()
        else:
            logits = m.train_step(u, i, r)[0]
        return logits, m.tables()


def test_determinism_and_isolation():
    rs = np.random.RandomState(17)
    U, I, D = 3000, 400, 64
    J, X = 7, 2                                                 # item J: column over several pieces; user X: long row
    N = implicit(U, I, rs, long_users=(X,), long_len=390, hot_item=J, hot_users=tuple(range(300)))
    t = tables(U, I, D, rs, 0.2)
    few_u = np.arange(300, dtype=np.int32)
    few_i = rs.randint(0, I, 300).astype(np.int32)
    few_r = rs.randint(1, 6, 300).astype(np.float32)
    few = (few_u, few_i, few_r)
    one = _isolation_run(t, N, (U, I, D), few)
    two = _isolation_run(t, N, (U, I, D), few)
    dev = _isolation_run(t, N, (U, I, D), few, dev=True)
    for a, b in ((one, two), (one, dev)):
        np.testing.assert_array_equal(a[0], b[0])
        for k in ORDER:
            np.testing.assert_array_equal(a[1][k], b[1][k])
    # the same 300 entries among 6000 of users outside J's column, interleaved
    n_other = 6000
    ou = rs.randint(300, U, n_other).astype(np.int32)
    oi = rs.randint(0, I, n_other).astype(np.int32)
    orr = rs.randint(1, 6, n_other).astype(np.float32)
    pos = np.sort(rs.choice(300 + n_other, 300, replace=False))
    mask = np.zeros(300 + n_other, bool)
    mask[pos] = True
    bu, bi, br = (np.empty(300 + n_other, a.dtype) for a in few)
    bu[mask], bi[mask], br[mask] = few
    bu[~mask], bi[~mask], br[~mask] = ou, oi, orr
    crowd = _isolation_run(t, N, (U, I, D), (bu, bi, br))
    np.testing.assert_array_equal(crowd[0][mask], one[0])
    np.testing.assert_array_equal(crowd[1][L.Y][J], one[1][L.Y][J])
    np.testing.assert_array_equal(crowd[1][L.P][X], one[1][L.P][X])
    np.testing.assert_array_equal(crowd[1][L.BU][X], one[1][L.BU][X])
    assert not np.array_equal(one[1][L.Y][J], t[R.YF][J])


def test_topk_and_rank_agree_with_the_forward():
    rs = np.random.RandomState(23)
    U, I, D = 200, 700, 32
    N = implicit(U, I, rs, long_users=(4,), long_len=600)
    t = tables(U, I, D, rs, 0.3)
    users = np.concatenate(([0, 4, 4], rs.randint(0, U, 60))).astype(np.int32)
    K = 20
    excl = T.rated_matrix(np.repeat(np.arange(U), 3), rs.randint(0, I, 3 * U), U, I)
    with model(U, I, D, t, N) as m:
        items, scores = m.recommend(users, k=K, exclude=excl)
        x = m.forward(np.repeat(users, K), items.reshape(-1))
        np.testing.assert_allclose(scores.reshape(-1), x, rtol=1e-5, atol=1e-5)
        ex_rows = excl.tocsr()[users]
        for r in range(users.size):
            assert not set(items[r]) & set(ex_rows[r].indices)
        targets = (np.arange(0, users.size * K + 1, K), items.reshape(-1))
        ranks = m.rank_items(users, targets, exclude=excl)
        np.testing.assert_array_equal(ranks.reshape(users.size, K), np.tile(np.arange(K), (users.size, 1)))
        # a target outside the top K ranks at K or beyond, and an excluded one is unranked
        out_items = np.array([np.setdiff1d(np.arange(I), np.union1d(items[r], ex_rows[r].indices))[0]
                              for r in range(users.size)], np.int32)
        ranks2 = m.rank_items(users, (np.arange(users.size + 1), out_items), exclude=excl)
        assert (ranks2 >= K).all()
        import torch
        d_items = m.recommend_dev(torch.from_numpy(users).cuda(), k=K, return_scores=False)
        ref_items = m.recommend(users, k=K, return_scores=False)
        np.testing.assert_array_equal(d_items.cpu().numpy(), ref_items)
        test_u = rs.randint(0, U, 400).astype(np.int32)
        test_i = rs.randint(0, I, 400).astype(np.int32)
        res = T.evaluate_ranking(m, test_u, test_i, exclude=excl, ks=(10,))
        assert res is not None


def test_errors_leave_the_tables_untouched():
    import torch
    rs = np.random.RandomState(29)
    U, I, D, B = 50, 40, 8, 100
    N = implicit(U, I, rs)
    t = tables(U, I, D, rs)
    u = rs.randint(0, U, B).astype(np.int32)
    i = rs.randint(0, I, B).astype(np.int32)
    r = rs.randint(1, 6, B).astype(np.float32)
    with model(U, I, D, t, N, optimizer="sgd", lr=0.1) as m:
        before = m.tables()
        bad = i.copy()
        bad[17] = I
        with pytest.raises(T.OutOfRangeError):
            m.train_step(u, bad, r)
        d = torch.device("cuda")
        badu = u.copy()
        badu[3] = -1
        m.train_step_dev(torch.from_numpy(badu).to(d), torch.from_numpy(i).to(d), torch.from_numpy(r).to(d))
        with pytest.raises(T.OutOfRangeError):
            m.sync()
        after = m.tables()
        for k in ORDER:
            np.testing.assert_array_equal(before[k], after[k])
        assert m.step == 1                                      # the _dev step was counted, as the SVD _dev step
        m.train_step(u, i, r)                                   # and the model goes on
    with model(U, I, D, t, N, optimizer="adam", adam_mode="tf1") as m:
        before = m.tables()
        with pytest.raises(T.TfrError) as e:
            m.train_step(u, i, r)
        assert e.value.code == L.ERR_STATE
        after = m.tables()
        for k in ORDER:
            np.testing.assert_array_equal(before[k], after[k])
    with T.SvdppModel(U, I, D) as m:
        m.set_tables(*(t[k] for k in ORDER))
        for call in (lambda: m.train_step(u, i, r), lambda: m.forward(u, i), lambda: m.recommend(u[:3], k=5)):
            with pytest.raises(T.TfrError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        after = m.tables()
        for k in ORDER:
            np.testing.assert_array_equal(t[k], after[k])


def test_driver_runs_and_train_error_falls(capsys):
    from tfrecomm_amd import svd_train_val
    svd_train_val.main(["--model", "svdpp", "--epochs", "2"])
    out = capsys.readouterr().out.splitlines()
    rows = [ln.split() for ln in out if ln.strip()[:1].isdigit()]
    assert len(rows) == 2 and out[-1] == "Done!"
    assert float(rows[1][1]) < float(rows[0][1])
