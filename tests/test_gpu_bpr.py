"""BPR steps on the device (tfr_bpr_*) against the float64 restatement and the NumPy sampler in tests/bpr_ref.py.

Tolerances.  One SGD step at lr = 1 moves every table by minus its gradient: the float32 gradient of a run is a sum of a few
float32 terms of size O(1), so it matches float64 to rtol 1e-4 / atol 1e-4 x the largest gradient (as tests/test_gpu_svdpp.py).
Over a trajectory the float32 rounding of the device and of a float32 oracle grow alike; the device's distance from the
float64 oracle must stay within four times the float32 oracle's, plus 1e-5 x the table's scale: the device sums a dot
product in another order than NumPy (lane fmaf chains and a butterfly), and Adam divides a gradient element by its own
running magnitude, so where an element is near zero a few ulps of it can move that element's step by more than the float32
oracle's own error.  A wrong or missing gradient term moves a table by O(lr) = 1e-3 per step, far above this bound."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import bpr_ref as R
from tests import widths as W

pytestmark = pytest.mark.gpu

# k_bpr_users / k_bpr_items are templated on NJ = ceil(D / 64) registers per lane, f = lane + 64 j guarded by f < D
# (csrc/wave_rows.h with_nj): one width per (NJ, last register full or partial), and D = 1 - widths.BPR, which
# tests/test_width_coverage.py holds against that rule.
WIDTHS = W.BPR


def registers(D):
    """(NJ, last register full) of the BPR kernels"""
    return -(-D // 64), D % 64 == 0


TABS = (R.MU, R.BU, R.BI, R.PF, R.QF)
FLAGS = [(False, False), (True, False), (False, True), (True, True)]     # (item_abs, reg_bias)


def csr(rows):
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    items = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return indptr, items


def positives(U, I, rs, lo=1, hi=30, full=(), empty=(), heavy=(), heavy_len=0):
    rows = []
    for u in range(U):
        if u in full:
            rows.append(np.arange(I))
        elif u in empty:
            rows.append(np.zeros(0, np.int64))
        elif u in heavy:
            rows.append(np.sort(rs.choice(I, heavy_len, replace=False)))
        else:
            rows.append(np.sort(rs.choice(I, rs.randint(lo, hi), replace=False)))
    return csr(rows)


def tables(U, I, D, rs, scale=0.3):
    f = lambda *s: rs.normal(0, scale, s).astype(np.float32)
    return {R.MU: np.float32(0.2), R.BU: f(U), R.BI: f(I), R.PF: f(U, D), R.QF: f(I, D)}


def model(U, I, D, t, pos=None, **kw):
    m = T.SvdModel(U, I, D, **kw)
    m.set_tables(*(t[k] for k in TABS))
    if pos is not None:
        m.set_positives(pos)
    return m


def f64(t):
    return {k: np.array(v, np.float64) for k, v in t.items()}


def got(m):
    g = m.tables()
    return {k: np.asarray(g[k], np.float64) for k in TABS}


def hazard_batch(U, I, rs, B):
    """random triples plus one user in many triples where one triple's negative is another's positive, and j == i"""
    u = rs.randint(0, U, B).astype(np.int32)
    i = rs.randint(0, I, B).astype(np.int32)
    j = rs.randint(0, I, B).astype(np.int32)
    n = 40
    u[:n] = 7
    i[:n] = np.arange(n) % 13
    j[:n] = (np.arange(n) + 1) % 13                                   # j of triple k is i of triple k + 1
    j[n - 1] = i[n - 1]                                               # an explicit j == i
    return u, i, j


# ---- 1. sampler -------------------------------------------------------------------------------------------------------
def test_sampler_matches_numpy_on_an_ml1m_shaped_csr():
    rs = np.random.RandomState(0)
    U, I = 6040, 3706
    HEAVY, FULL, EMPTY = 10, 11, 12
    pos = positives(U, I, rs, lo=20, hi=311, full=(FULL,), empty=(EMPTY,), heavy=(HEAVY,), heavy_len=int(0.62 * I))
    assert pos[0][-1] > 900000
    users = np.concatenate(([HEAVY] * 3000, [FULL] * 50, [EMPTY] * 50, rs.randint(0, U, 6900))).astype(np.int32)
    rs.shuffle(users)
    t = tables(U, I, 8, rs)
    with model(U, I, 8, t, pos, optimizer="adam", adam_mode="lazy") as m:
        for seed, attempts, step in ((0, 16, 0), (12345, 16, 99), (7, 64, 3), (2 ** 64 - 1, 1, 2 ** 40)):
            m.set_bpr_sampler(seed, attempts)
            want = R.sample(pos[0], pos[1], users, I, seed, step, attempts)
            assert np.array_equal(m.bpr_negatives(users, step), want), (seed, attempts, step)
        assert np.all(want[users == FULL] == -1)
        m.set_bpr_sampler()
        m.set_step(5, 0.9 ** 6, 0.999 ** 6)
        alone = m.bpr_negatives(users)                                # at the model's step counter
        assert np.array_equal(alone, m.bpr_negatives(users, 5))
        neg, _, _, skipped = m.train_bpr_step(users, rs.randint(0, I, users.size))
        assert np.array_equal(neg, alone)
        assert skipped == int(np.sum(alone < 0)) and skipped >= 50
        h = np.mean(alone[users == HEAVY] < 0)
        assert h < 0.01                                               # 0.62^16 ~ 5e-4


# ---- 2. parity --------------------------------------------------------------------------------------------------------
def _one_step(D, item_abs, reg_bias):
    rs = np.random.RandomState(D + 3)
    U, I, B = 300, 200, 1500
    t = tables(U, I, D, rs, 0.2)
    u, i, j = hazard_batch(U, I, rs, B)
    lam = 0.05
    pos = positives(U, I, rs)
    with model(U, I, D, t, pos, item_abs=item_abs, reg_bias=reg_bias, optimizer="sgd", lr=1.0, reg=lam) as m:
        neg, lossv, regv, skipped = m.train_bpr_step(u, i, j)
        after = got(m)
        assert m.step == 1
    assert np.array_equal(neg, j) and skipped == 0
    t64 = f64(t)
    _, data, reg = R.terms(t64, u, i, j, item_abs, reg_bias)
    assert lossv == pytest.approx(data, rel=1e-4)
    assert regv == pytest.approx(reg, rel=1e-4)
    G = R.gradients(t64, u, i, j, lam, item_abs, reg_bias)
    for k, (g, touched) in G.items():
        d = t64[k] - after[k]
        np.testing.assert_allclose(d, g, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(g).max()), err_msg="table %d" % k)
        assert not d[~touched].any()
    for k in (R.MU, R.BU):
        assert np.array_equal(after[k], t64[k])                       # never read or written


@pytest.mark.parametrize("item_abs,reg_bias", FLAGS)
def test_one_step_gradients(item_abs, reg_bias):
    _one_step(16, item_abs, reg_bias)


@pytest.mark.parametrize("D", WIDTHS)
def test_one_step_gradients_at_every_register_width(D):
    _one_step(D, *FLAGS[WIDTHS.index(D) % len(FLAGS)])


def _trajectory(D, optimizer, item_abs, reg_bias, frozen=0, steps=50):
    rs = np.random.RandomState(11 + D)
    U, I, B = 200, 150, 600
    t = tables(U, I, D, rs, 0.1)
    lr = 1e-3 if optimizer == "adam" else 2e-3
    kw = dict(item_abs=item_abs, reg_bias=reg_bias, optimizer=optimizer, lr=lr, reg=0.05)
    refs = {dt: R.BprRef(U, I, D, dtype=dt, **kw) for dt in (np.float64, np.float32)}
    for ref in refs.values():
        ref.set_tables(t)
        ref.frozen = frozen
    pos = positives(U, I, rs)
    with model(U, I, D, t, pos, adam_mode="lazy", **kw) as m:
        m.set_frozen(frozen)
        for s in range(steps):
            u, i, j = hazard_batch(U, I, rs, B) if s % 5 == 0 else (rs.randint(0, U, B), rs.randint(0, I, B), None)
            neg = m.train_bpr_step(u, i, j)[0]
            for ref in refs.values():
                ref.train_step(u, i, neg)
        out = got(m)
        assert m.step == steps
    for k in TABS:
        truth = np.asarray(refs[np.float64].t[k], np.float64)
        if (frozen >> k) & 1 or k in (R.MU, R.BU):
            assert np.array_equal(out[k], np.asarray(t[k], np.float64)), k
            continue
        e_gpu = np.abs(out[k] - truth).max()
        e_f32 = np.abs(np.asarray(refs[np.float32].t[k], np.float64) - truth).max()
        assert e_gpu <= 4 * e_f32 + 1e-5 * max(1.0, np.abs(truth).max()), (k, e_gpu, e_f32)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("item_abs,reg_bias", FLAGS)
def test_fifty_step_trajectory(optimizer, item_abs, reg_bias):
    _trajectory(32, optimizer, item_abs, reg_bias)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("D", WIDTHS)
def test_trajectory_at_every_register_width(D, optimizer):
    _trajectory(D, optimizer, *FLAGS[WIDTHS.index(D) % len(FLAGS)], steps=20)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("bit", [R.BI, R.PF, R.QF])
def test_frozen_tables(bit, optimizer):
    _trajectory(20, optimizer, False, True, frozen=1 << bit, steps=10)


# ---- 3. semantics -----------------------------------------------------------------------------------------------------
def test_skipped_triples_touch_nothing():
    """User FULL has every item positive, so its triples are skipped.  Item 0 is a positive of every user, so it is never
    sampled as a negative: it occurs only in the skipped triples.  Their rows and slots stay as they were, and the rest of
    the batch moves exactly as the float64 step of the batch without them (SGD at lr = 1: minus the gradient)."""
    rs = np.random.RandomState(4)
    U, I, D, B = 50, 40, 16, 400
    FULL = 3
    rows = [np.concatenate(([0], np.sort(rs.choice(np.arange(1, I), rs.randint(1, 20), replace=False)))) for _ in range(U)]
    rows[FULL] = np.arange(I)
    pos = csr(rows)
    t = tables(U, I, D, rs)
    u = rs.randint(0, U, B).astype(np.int32)
    u[u == FULL] = 4
    i = rs.randint(1, I, B).astype(np.int32)
    u[:5], i[:5] = FULL, 0
    with model(U, I, D, t, pos, optimizer="adam", adam_mode="lazy", lr=1e-2) as m:
        neg, _, _, skipped = m.train_bpr_step(u, i)
        g = m.tables()
        slots = {k: (m.get_table(k | L.SLOT_M), m.get_table(k | L.SLOT_V)) for k in (L.P, L.Q, L.BI)}
    assert skipped == 5 and np.all(neg[:5] == -1) and np.all(neg[5:] > 0)
    assert np.array_equal(g[L.P][FULL], t[R.PF][FULL]) and not slots[L.P][0][FULL].any() and not slots[L.P][1][FULL].any()
    assert np.array_equal(g[L.Q][0], t[R.QF][0]) and not slots[L.Q][0][0].any() and not slots[L.Q][1][0].any()
    assert g[L.BI][0] == t[R.BI][0] and slots[L.BI][0][0] == 0 and slots[L.BI][1][0] == 0
    lam = 0.05
    with model(U, I, D, t, pos, optimizer="sgd", lr=1.0, reg=lam) as m:
        neg2, lossv, regv, skipped2 = m.train_bpr_step(u, i)
        after = got(m)
    assert np.array_equal(neg2, neg) and skipped2 == 5                # the same step counter: the same draws
    t64 = f64(t)
    keep = neg >= 0
    _, data, reg = R.terms(t64, u[keep], i[keep], neg[keep])
    assert lossv == pytest.approx(data, rel=1e-4) and regv == pytest.approx(reg, rel=1e-4)
    for k, (gr, touched) in R.gradients(t64, u[keep], i[keep], neg[keep], lam).items():
        d = t64[k] - after[k]
        np.testing.assert_allclose(d, gr, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(gr).max()), err_msg="table %d" % k)
        assert not d[~touched].any()


def test_device_form_equals_the_host_form():
    """train_bpr_step_dev on torch tensors, sampled and explicit negatives: the negatives it reports and the tables are
    bit-identical to train_bpr_step on the same columns"""
    import torch
    rs = np.random.RandomState(12)
    U, I, D, B = 700, 400, 64, 3000
    pos = positives(U, I, rs, hi=60)
    t = tables(U, I, D, rs, 0.1)
    batches = [(rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32), None) for _ in range(3)]
    batches.append(hazard_batch(U, I, rs, B))
    dev = torch.device("cuda")
    res = []
    for on_device in (False, True):
        with model(U, I, D, t, pos, optimizer="adam", adam_mode="lazy", lr=1e-2) as m:
            negs = []
            for u, i, j in batches:
                if on_device:
                    cols = [torch.from_numpy(a).to(dev) for a in (u, i) + (() if j is None else (j,))]
                    n = m.train_bpr_step_dev(cols[0], cols[1], None if j is None else cols[2], want_negatives=True)
                    m.sync()
                    negs.append(n.cpu().numpy())
                else:
                    negs.append(m.train_bpr_step(u, i, j)[0])
            res.append((np.concatenate(negs).tobytes(), {k: v.tobytes() for k, v in m.tables().items()}, m.step))
    assert res[0] == res[1]


def test_tf1_adam_is_refused():
    rs = np.random.RandomState(0)
    t = tables(20, 10, 8, rs)
    with model(20, 10, 8, t, positives(20, 10, rs, hi=5), optimizer="adam", adam_mode="tf1") as m:
        with pytest.raises(L.TfrError) as e:
            m.train_bpr_step([0, 1], [2, 3])
        assert e.value.code == L.ERR_STATE
        with pytest.raises(L.TfrError) as e:
            m.rng_seed(1)
            m.train_bpr_steps_drawn(4, 2)
        assert e.value.code == L.ERR_STATE


def test_out_of_range_id_voids_the_step():
    import torch
    rs = np.random.RandomState(1)
    U, I, D = 30, 20, 8
    t = tables(U, I, D, rs)
    with model(U, I, D, t, positives(U, I, rs, hi=5), optimizer="adam", adam_mode="lazy") as m:
        for u, i, j in (([0, 30], [1, 2], None), ([0, 1], [1, 20], None), ([0, 1], [1, 2], [3, 20]), ([0, 1], [1, 2], [3, -1])):
            with pytest.raises(L.OutOfRangeError):
                m.train_bpr_step(u, i, j)
            assert m.step == 0
        d = torch.device("cuda")
        m.train_bpr_step_dev(torch.tensor([0, 1], dtype=torch.int32, device=d), torch.tensor([1, 25], dtype=torch.int32, device=d))
        with pytest.raises(L.OutOfRangeError):
            m.sync()
        after = got(m)
    for k in TABS:
        assert np.array_equal(after[k], np.asarray(t[k], np.float64)), k


def test_malformed_positives_are_refused_before_device_work():
    lib = L.load()
    rs = np.random.RandomState(2)
    t = tables(3, 5, 4, rs)
    cases = [([0, 1, 2, 3], [0, 9, 1], L.ERR_OOB), ([0, 1, 2, 3], [0, -1, 1], L.ERR_OOB),
             ([0, 2, 2, 3], [3, 1, 0], L.ERR_ARG), ([0, 2, 2, 3], [1, 1, 0], L.ERR_ARG),
             ([1, 1, 2, 3], [0, 1, 2], L.ERR_ARG), ([0, 2, 1, 3], [0, 1, 2], L.ERR_ARG)]
    with model(3, 5, 4, t, optimizer="sgd") as m:
        for ip, it, code in cases:
            ip, it = np.asarray(ip, np.int64), np.asarray(it, np.int32)
            assert lib.tfr_bpr_set_positives(m._h, L.ptr_i64(ip), L.ptr_i32(it)) == code, (ip, it)
        with pytest.raises(L.TfrError) as e:
            m.bpr_negatives([0])                                      # nothing was accepted
        assert e.value.code == L.ERR_STATE


def test_sampling_before_positives_is_refused():
    rs = np.random.RandomState(3)
    t = tables(10, 8, 4, rs)
    with model(10, 8, 4, t, optimizer="sgd") as m:
        m.rng_seed(0)
        for call in (lambda: m.bpr_negatives([0, 1]), lambda: m.train_bpr_step([0], [1]),
                     lambda: m.train_bpr_step([0], [1], [2]), lambda: m.train_bpr_steps_drawn(4, 1)):
            with pytest.raises(L.TfrError) as e:
                call()
            assert e.value.code == L.ERR_STATE


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    rs = np.random.RandomState(5)
    U, I, D = 2000, 1500, 64
    pos = positives(U, I, rs, hi=80)
    t = tables(U, I, D, rs, 0.1)
    out = []
    for _ in range(2):
        with model(U, I, D, t, pos, optimizer="adam", adam_mode="lazy", lr=1e-2) as m:
            m.rng_seed(9)
            loss = m.train_bpr_steps_drawn(3000, 10, want_loss=True)
            out.append((loss.tobytes(), {k: v.tobytes() for k, v in m.tables().items()}))
    assert out[0] == out[1]


def test_a_users_rows_do_not_depend_on_unrelated_users():
    rs = np.random.RandomState(6)
    U, I, D = 1100, 600, 64
    X = 1050
    t = tables(U, I, D, rs, 0.2)
    pos = positives(U, I, rs)
    mine_i = np.arange(500, 600)                                     # only user X's triples use these items
    xu = np.full(64, X, np.int32)
    xi, xj = rs.choice(mine_i, 64).astype(np.int32), rs.choice(mine_i, 64).astype(np.int32)
    ou = rs.randint(0, 1000, 20000).astype(np.int32)
    oi, oj = rs.randint(0, 500, 20000).astype(np.int32), rs.randint(0, 500, 20000).astype(np.int32)
    res = []
    for crowd in (False, True):
        with model(U, I, D, t, pos, optimizer="adam", adam_mode="lazy", lr=1e-2) as m:
            for s in range(3):
                if crowd:                                    # X's triples keep their order, at random positions
                    at = np.zeros(20064, bool)
                    at[rs.choice(20064, 64, replace=False)] = True
                    cu, ci, cj = (np.empty(20064, np.int32) for _ in range(3))
                    for c, a, b in ((cu, xu, ou), (ci, xi, oi), (cj, xj, oj)):
                        c[at], c[~at] = a, b
                    m.train_bpr_step(cu, ci, cj)
                else:
                    m.train_bpr_step(xu, xi, xj)
            g = m.tables()
            res.append((g[L.P][X].tobytes(), g[L.Q][mine_i].tobytes(), g[L.BI][mine_i].tobytes(),
                        m.get_table(L.P | L.SLOT_V)[X].tobytes()))
    assert res[0] == res[1]


# ---- 5. drawn form ----------------------------------------------------------------------------------------------------
def test_drawn_form_equals_the_explicit_form_of_numpys_draws():
    rs = np.random.RandomState(7)
    U, I, D, B, steps = 800, 500, 32, 2048, 6
    pos = positives(U, I, rs, hi=60)
    nnz = int(pos[0][-1])
    rowof = np.repeat(np.arange(U), np.diff(pos[0])).astype(np.int32)
    t = tables(U, I, D, rs, 0.1)
    res = []
    for drawn in (True, False):
        with model(U, I, D, t, pos, optimizer="adam", adam_mode="lazy", lr=1e-2) as m:
            m.set_bpr_sampler(42, 16)
            np.random.seed(2024)
            if drawn:
                m.rng_from_numpy()
                loss = np.concatenate([m.train_bpr_steps_drawn(B, 2, want_loss=True),
                                       m.train_bpr_steps_drawn(B, steps - 2, want_loss=True)])
                k, p = m.rng_get_state()
                np.random.randint(0, nnz, (steps, B))
                want = np.random.get_state()
                assert np.array_equal(k, want[1]) and p == want[2]
            else:
                loss = []
                for _ in range(steps):
                    e = np.random.randint(0, nnz, B)
                    loss.append(m.train_bpr_step(rowof[e], pos[1][e])[1])
                loss = np.asarray(loss, np.float32)
            res.append((loss.tobytes(), {k: v.tobytes() for k, v in m.tables().items()}))
    assert res[0] == res[1]


def test_the_svd_run_ahead_is_cancelled():
    """SVD drawn steps, BPR drawn steps, SVD drawn steps on one model: the same tables, bit for bit, as host-drawn ids
    consumed in that order (the SVD call's look-ahead draw must not leak into the BPR steps, nor the BPR draw into SVD's)"""
    rs = np.random.RandomState(8)
    U, I, D, N = 600, 400, 16, 20000
    su, si = rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32)
    sr = rs.randint(1, 6, N).astype(np.float32)
    pos = positives(U, I, rs, hi=40)
    nnz = int(pos[0][-1])
    rowof = np.repeat(np.arange(U), np.diff(pos[0])).astype(np.int32)
    t = tables(U, I, D, rs, 0.1)
    res = []
    for drawn in (True, False):
        with model(U, I, D, t, pos, optimizer="adam", adam_mode="lazy", lr=1e-3) as m:
            m.upload_triples(su, si, sr)
            np.random.seed(77)
            if drawn:
                m.rng_from_numpy()
                m.train_steps_drawn(1000, 9)                          # >= 8 steps: its run-ahead draw is left behind
                m.train_bpr_steps_drawn(700, 3)
                m.train_steps_drawn(1000, 9)
                m.rng_to_numpy()
            else:
                m.train_steps_resident(np.random.randint(0, N, (9, 1000)), 1000)
                for _ in range(3):
                    e = np.random.randint(0, nnz, 700)
                    m.train_bpr_step(rowof[e], pos[1][e])
                m.train_steps_resident(np.random.randint(0, N, (9, 1000)), 1000)
            tail = np.random.randint(0, 1 << 30, 4).tolist()
            res.append(({k: v.tobytes() for k, v in m.tables().items()}, tail))
    assert res[0] == res[1]


def test_bpr_step_between_staged_calls():
    """A staged SVD call with staged ids left over ends by sorting the next call's first batch into the model's sort
    scratch (the look-ahead of the small-table step).  A BPR step in between sorts into the same scratch: the next staged
    call must not take the look-ahead then.  The BPR step runs with its tables frozen, so the SVD steps must end bit for
    bit where the same calls without it end (SGD: the step counter the BPR step advances does not enter the update)."""
    rs = np.random.RandomState(13)
    U, I, D, N, B = 300, 200, 20, 5000, 1000
    su, si = rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32)
    sr = rs.randint(1, 6, N).astype(np.float32)
    pos = positives(U, I, rs)
    t = tables(U, I, D, rs, 0.1)
    ids = rs.randint(0, N, 6 * B).astype(np.int64)
    bu, bi_ = rs.randint(0, U, 400).astype(np.int32), rs.randint(0, I, 400).astype(np.int32)   # 2 x 400 keys: no regrowth
    res = []
    for with_bpr in (False, True):
        with model(U, I, D, t, pos, optimizer="sgd", lr=1e-3) as m:
            m.upload_triples(su, si, sr)
            m.stage_ids(ids)
            a = m.train_steps_staged(0, B, 3, want_loss=True)
            if with_bpr:
                m.set_frozen((1 << L.BI) | (1 << L.P) | (1 << L.Q))
                m.train_bpr_step(bu, bi_)
                m.set_frozen(0)
            b = m.train_steps_staged(3, B, 3, want_loss=True)
            res.append((a.tobytes(), b.tobytes(), {k: v.tobytes() for k, v in m.tables().items()}))
    assert res[0] == res[1]


# ---- 6. the point of it -----------------------------------------------------------------------------------------------
def planted(U=2000, I=1000, D=16, per=50, beta=4.0, seed=0):
    """each user's 50 items drawn from softmax(beta * a_u . b_i / sqrt(D)) of a rank-D truth; 40 train, 10 held out"""
    rs = np.random.RandomState(seed)
    A, Bm = rs.normal(0, 1, (U, D)), rs.normal(0, 1, (I, D))
    s = A @ Bm.T / np.sqrt(D)
    tr, te = [], []
    for u in range(U):
        p = np.exp(beta * (s[u] - s[u].max()))
        it = rs.choice(I, per, replace=False, p=p / p.sum())
        tr.append(np.sort(it[:int(0.8 * per)]))
        te.append(np.sort(it[int(0.8 * per):]))
    return tr, te


def test_bpr_learns_a_planted_ranking():
    U, I, D, B, epochs = 2000, 1000, 16, 2000, 10
    tr, te = planted(U, I, D)
    pos = csr(tr)
    nnz = int(pos[0][-1])
    rowof = np.repeat(np.arange(U), np.diff(pos[0])).astype(np.int32)
    tu = np.repeat(np.arange(U), [r.size for r in te]).astype(np.int32)
    ti = np.concatenate(te).astype(np.int32)
    rs = np.random.RandomState(1)
    t = {R.MU: np.float32(0), R.BU: np.zeros(U, np.float32), R.BI: np.zeros(I, np.float32),
         R.PF: rs.normal(0, .1, (U, D)).astype(np.float32), R.QF: rs.normal(0, .1, (I, D)).astype(np.float32)}
    kw = dict(optimizer="adam", lr=0.05, reg=0.005)
    ref = R.BprRef(U, I, D, **kw)
    ref.set_tables(t)
    excl = T.rated_matrix(rowof, pos[1], U, I)
    with model(U, I, D, t, pos, adam_mode="lazy", **kw) as m:
        auc0 = T.evaluate_ranking(m, tu, ti, exclude=excl)["mean"]["auc"]
        np.random.seed(3)
        for _ in range(epochs * (nnz // B)):
            e = np.random.randint(0, nnz, B)
            u, i = rowof[e], pos[1][e]
            neg = m.train_bpr_step(u, i)[0]
            ref.train_step(u, i, neg)
        auc1 = T.evaluate_ranking(m, tu, ti, exclude=excl)["mean"]["auc"]
    users = np.arange(U)
    auc_ref = R.auc(ref.t, users, te, tr)
    assert 0.45 < auc0 < 0.55, auc0
    assert auc1 >= 0.85, auc1
    assert abs(auc1 - auc_ref) <= 0.01, (auc1, auc_ref)


# ---- 7. no effect on the rest -----------------------------------------------------------------------------------------
def test_svd_step_is_unchanged_by_positives():
    rs = np.random.RandomState(9)
    U, I, D, B = 500, 300, 64, 4000
    t = tables(U, I, D, rs, 0.2)
    pos = positives(U, I, rs)
    u, i = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
    r = rs.randint(1, 6, B).astype(np.float32)
    out = []
    for with_pos in (False, True):
        with model(U, I, D, t, pos if with_pos else None, optimizer="adam", adam_mode="lazy") as m:
            if with_pos:
                m.set_bpr_sampler(5, 8)
            a = m.train_step(u, i, r)
            b = m.train_step(u, i, r)
            out.append((a[0].tobytes(), b[0].tobytes(), a[1], b[2], {k: v.tobytes() for k, v in m.tables().items()}))
    assert out[0] == out[1]


# ---- 8. driver --------------------------------------------------------------------------------------------------------
def test_driver_runs_two_epochs(capsys):
    from tfrecomm_amd import svd_train_val
    tr, te = planted(300, 200, 8, per=30)
    mk = lambda rows: {"user": np.repeat(np.arange(300), [r.size for r in rows]).astype(np.int32),
                       "item": np.concatenate(rows).astype(np.int32)}
    train, test = mk(tr), mk(te)
    train["outcome"] = np.ones(train["user"].size, np.float32)
    test["outcome"] = np.ones(test["user"].size, np.float32)
    rows = svd_train_val.bpr(train, test, user_num=300, item_num=200, dim=8, batch_size=500, epoch_max=2)
    out = capsys.readouterr().out
    assert "bpr_loss" in out and "auc" in out
    assert len(rows) == 2 and all(np.isfinite(x) for row in rows for x in row)
    assert rows[1][1] < rows[0][1] + 1e-3                             # the mean BPR loss does not rise
