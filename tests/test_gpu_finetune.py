"""Batched per-user fine-tuning on the device (tfr_finetune_users / SvdModel.finetune_users / tfrecomm_amd.finetune's drivers with
batched=True):
against the sequential HIP drivers and the float64 oracle, bit-exactness where it must hold (a user alone or among 1000
others, run to run, untouched rows), a user whose rows do not fit the LDS staging, the errors, and the ML-1M-shaped
adaptive run.  Tolerances as tests/test_adaptive.py's driver test: 2e-4 SGD, 5e-3 lazy Adam (scale-relative)."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import adaptive_test as AT
from tfrecomm_amd import finetune as FT
from tests.finetune_ref import OracleDriverModel, per_user_frame
from tests.finetune_step_ref import powers_at
from tests.util import assert_close, rand_tables
from tests import widths as W

pytestmark = pytest.mark.gpu


def _model(U, I, D, t, **kw):
    m = T.SvdModel(U, I, D, **kw)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    return m


def _user_state(m):
    st = [m.get_table(L.P), m.get_table(L.BU)]
    if m.optimizer == "adam":
        st += [m.get_table(L.P | L.SLOT_M), m.get_table(L.P | L.SLOT_V), m.get_table(L.BU | L.SLOT_M),
               m.get_table(L.BU | L.SLOT_V)]
    return st


def _kw(opt, loss, item_abs=False, reg_bias=False):
    lazy = opt == "lazy"
    return dict(loss=loss, item_abs=item_abs, reg_bias=reg_bias, optimizer="adam" if lazy else "sgd", adam_mode="lazy",
                lr=5e-3 if lazy else 0.05, reg=0.1), (5e-3 if lazy else 2e-4)


CASES = [  # driver, D, opt, loss, item_abs, reg_bias
    ("non_adaptive", 5, "sgd", "nll", False, False),
    ("non_adaptive", 20, "lazy", "mse", True, True),
    ("non_adaptive", 64, "sgd", "mse", False, True),
    ("adaptive", 20, "sgd", "nll", True, False),
    ("adaptive", 128, "lazy", "nll", False, True),
    ("adaptive", 256, "sgd", "mse", True, True),
    ("adaptive_all", 64, "lazy", "nll", True, False),
    ("non_adaptive", 256, "lazy", "nll", False, False),
]


@pytest.mark.parametrize("driver,D,opt,loss,item_abs,reg_bias", CASES)
def test_batched_drivers_match_the_sequential_hip_drivers_and_the_oracle(driver, D, opt, loss, item_abs, reg_bias):
    _check_batched_drivers(driver, D, opt, loss, item_abs, reg_bias)


# at each width both drivers, each with its own optimiser, the optimisers swapping from one width to the next
WIDTH_CASES = [(drv, D, ("sgd", "lazy")[(x + y) % 2], ("mse", "nll")[x % 2], bool(y), x % 3 == 0)
               for x, D in enumerate(W.FINETUNE) for y, drv in enumerate(("non_adaptive", "adaptive"))]


@pytest.mark.parametrize("driver,D,opt,loss,item_abs,reg_bias", WIDTH_CASES)
def test_batched_drivers_at_every_register_width(driver, D, opt, loss, item_abs, reg_bias):
    """k_finetune<NJ> at every NJ = ceil(D / 64), last register full and partial"""
    _check_batched_drivers(driver, D, opt, loss, item_abs, reg_bias)


def _check_batched_drivers(driver, D, opt, loss, item_abs, reg_bias):
    U, I = 40, 70
    rs = np.random.RandomState(D)
    t = rand_tables(rs, U, I, D, scale=0.3 / np.sqrt(D / 8.0))
    df = per_user_frame(rs, rs.permutation(U)[:9], I, 7, binary=loss == "nll")
    kw, tol = _kw(opt, loss, item_abs, reg_bias)
    if driver == "non_adaptive":
        run = lambda m, drv=AT, **b: drv.non_adaptive_test(m, df, epoch_max=12, **b)
    else:
        run = lambda m, drv=AT, **b: drv.adaptive_test(m, df, budget=5, epoch_max=15, max_users=None,
                                                       ask_everything=driver == "adaptive_all", **b)
    orc = OracleDriverModel(U, I, D, t, **kw)
    want = run(orc)
    with _model(U, I, D, t, **kw) as seq, _model(U, I, D, t, **kw) as bat:
        ref = run(seq)
        got = run(bat, drv=FT, batched=True)
        for other, what in ((ref, "sequential HIP"), (want, "oracle")):
            if driver == "non_adaptive":
                assert got["truth"] == other["truth"]
                assert_close(got["pred"], other["pred"], rtol=tol, what="predictions vs " + what)
            else:
                assert len(got) == len(other)
                for g, w in zip(got, other):
                    assert (g["user"], g["asked"], g["outcome"], g["size"]) == (w["user"], w["asked"], w["outcome"], w["size"])
                    assert_close(g["predicted"], w["predicted"], rtol=tol, what="predictions vs " + what)
                    assert abs(g["mcost"] - w["mcost"]) <= 10 * tol * max(1.0, abs(w["mcost"])), (what, g["mcost"], w["mcost"])
        for a, b, o in zip(_user_state(bat), _user_state(seq), orc.user_state()):
            assert_close(a, b, rtol=10 * tol, what="user tables / slots vs sequential HIP")
            assert_close(a, o, rtol=10 * tol, what="user tables / slots vs oracle")
        assert bat.get_step() == seq.get_step()                # step counter and beta powers bit for bit
        tb = bat.tables()
        assert np.array_equal(tb[L.Q], t["Q"]) and np.array_equal(tb[L.BI], t["bi"]) and tb[L.MU] == t["mu"]


def _schedule(rs, users, I, rows_per_user, E, max_rounds=4):
    """a direct schedule: every user its rows, a few rounds of growing prefixes"""
    row_ptr, items, rates, round_ptr, ask, prefix = [0], [], [], [0], [], []
    for u, n in zip(users, rows_per_user):
        items.append(rs.randint(0, I, n)); rates.append((rs.rand(n) < 0.5).astype(np.float32))
        row_ptr.append(row_ptr[-1] + n)
        k = min(max_rounds, n)
        pre = np.unique(np.linspace(1, n, k).astype(np.int64))
        prefix.extend(pre.tolist()); ask.extend(rs.randint(0, I, pre.size).tolist())
        round_ptr.append(round_ptr[-1] + pre.size)
    return (np.asarray(users, np.int32), np.asarray(row_ptr, np.int64), np.concatenate(items).astype(np.int32),
            np.concatenate(rates), np.asarray(round_ptr, np.int64), np.asarray(ask, np.int32), np.asarray(prefix, np.int32), E)


def _sub(s, x):
    users, row_ptr, items, rates, round_ptr, ask, prefix, E = s
    r0, r1, k0, k1 = row_ptr[x], row_ptr[x + 1], round_ptr[x], round_ptr[x + 1]
    return (users[x:x + 1], np.array([0, r1 - r0]), items[r0:r1], rates[r0:r1], np.array([0, k1 - k0]), ask[k0:k1],
            prefix[k0:k1], E)


@pytest.mark.parametrize("opt,D", [("sgd", 20), ("lazy", 5), ("lazy", 64), ("lazy", 256), ("lazy", 192)])
def test_a_user_alone_and_among_1000_others_is_bit_identical(opt, D):
    U, I = 1200, 500
    rs = np.random.RandomState(4)
    t = rand_tables(rs, U, I, D, scale=0.1)
    users = rs.permutation(U)[:1001]
    s = _schedule(rs, users, I, rs.randint(1, 40, users.size), 20)
    kw, _ = _kw(opt, "nll")
    x = 500
    u, r0, r1, k0, k1 = int(users[x]), int(s[1][x]), int(s[1][x + 1]), int(s[4][x]), int(s[4][x + 1])
    with _model(U, I, D, t, **kw) as a, _model(U, I, D, t, **kw) as b, _model(U, I, D, t, **kw) as c:
        for m in (a, b, c):
            m.set_frozen(AT.FROZEN_BUT_USER)
        before = a.tables()
        ra = a.finetune_users(*s)
        rb = b.finetune_users(*s)                                           # run to run
        for p, q in zip(ra, rb):
            assert np.array_equal(p, q, equal_nan=True)
        for p, q in zip(_user_state(a), _user_state(b)):
            assert np.array_equal(p, q)
        assert a.get_step() == b.get_step()
        # user x alone, started at the beta powers its first round had inside the big call (position k0 * E)
        st = c.get_step()
        c.set_step(st[0], *(powers_at(st[1], st[2], 0.9, 0.999, k0 * s[7]) if opt == "lazy" else st[1:]))
        rc = c.finetune_users(*_sub(s, x))
        assert np.array_equal(rc[0], ra[0][k0:k1]) and np.array_equal(rc[1], ra[1][k0:k1])
        assert np.array_equal(rc[2], ra[2][r0:r1], equal_nan=True)
        for p, q in zip(_user_state(c), _user_state(a)):
            assert np.array_equal(p[u], q[u])
        # mu, the item tables and every user outside the schedule: untouched
        after = a.tables()
        others = np.setdiff1d(np.arange(U), users)
        assert np.array_equal(after[L.P][others], before[L.P][others])
        assert np.array_equal(after[L.BU][others], before[L.BU][others])
        for w in (L.MU, L.BI, L.Q):
            assert np.array_equal(after[w], before[w])
        assert a.step == int(s[4][-1]) * s[7]
        if opt == "lazy":
            assert a.get_step()[1:] == powers_at(0.9, 0.999, 0.9, 0.999, a.step)


@pytest.mark.parametrize("opt", ["sgd", "lazy"])
def test_a_heavy_user_streamed_from_global_memory_matches_the_oracle(opt):
    _check_streamed(opt, 20, lambda staged: 12)


@pytest.mark.parametrize("opt", ["sgd", "lazy"])
@pytest.mark.parametrize("D", W.FINETUNE_STREAMED)
def test_staged_and_streamed_users_in_one_call_at_every_register_count(opt, D):
    """k_finetune<NJ> with STAGED true and false in one launch at every NJ; the staged user has exactly as many rows as
    tfr_finetune_plan stages at this width, the next user one more"""
    _check_streamed(opt, D, lambda staged: staged, lambda staged: staged + 1)


def _check_streamed(opt, D, light_rows, mid_rows=lambda staged: 500):
    U, I = 50, 4000
    rs = np.random.RandomState(12)
    t = rand_tables(rs, U, I, D, scale=0.05 * np.sqrt(20.0 / D))
    kw, tol = _kw(opt, "nll")
    kw["lr"] = kw["lr"] / 30                        # thousands of rows per step
    users = np.array([17, 3, 40], np.int32)
    lds, staged, wpb = C.c_int64(), C.c_int32(), C.c_int32()
    assert L.load().tfr_finetune_plan(D, 3000, C.byref(lds), C.byref(staged), C.byref(wpb)) == L.OK
    light, mid = light_rows(staged.value), mid_rows(staged.value)
    assert 1 <= light <= staged.value < mid < 3000  # users 17 and 40 stream, user 3 is staged
    s = _schedule(rs, users, I, [3000, light, mid], 3, max_rounds=3)
    orc = OracleDriverModel(U, I, D, t, **kw)
    orc.set_frozen(AT.FROZEN_BUT_USER)
    want = orc.finetune_users(*s)
    with _model(U, I, D, t, **kw) as m:
        m.set_frozen(AT.FROZEN_BUT_USER)
        got = m.finetune_users(*s)
        assert_close(got[0], want[0], rtol=tol, what="ask logits")
        assert_close(got[1], want[1], rtol=10 * tol, what="round losses")
        ok = ~np.isnan(want[2])
        assert np.array_equal(ok, ~np.isnan(got[2]))
        assert_close(got[2][ok], want[2][ok], rtol=tol, what="final logits")
        for a, o in zip(_user_state(m), orc.user_state()):
            assert_close(a[users], o[users], rtol=10 * tol, what="user tables / slots")


def test_errors_leave_the_model_unchanged():
    U, I, D = 30, 40, 8
    rs = np.random.RandomState(2)
    t = rand_tables(rs, U, I, D)
    s = _schedule(rs, [3, 9, 4], I, [5, 6, 2], 4)
    users, row_ptr, items, rates, round_ptr, ask, prefix, E = s
    kw, _ = _kw("lazy", "nll")
    with _model(U, I, D, t, **kw) as m:
        m.set_frozen(AT.FROZEN_BUT_USER)
        m.set_step(7, 0.5, 0.75)
        before, st0 = m.tables(), m.get_step()
        slots0 = _user_state(m)

        def expect(code, *args, **k):
            with pytest.raises(L.TfrError) as e:
                m.finetune_users(*args, **k)
            assert e.value.code == code
            after = m.tables()
            for w in before:
                assert np.array_equal(after[w], before[w])
            for p, q in zip(_user_state(m), slots0):
                assert np.array_equal(p, q)
            assert m.get_step() == st0

        bad = items.copy(); bad[3] = I
        expect(L.ERR_OOB, users, row_ptr, bad, rates, round_ptr, ask, prefix, E)
        bad = ask.copy(); bad[-1] = -1
        expect(L.ERR_OOB, users, row_ptr, items, rates, round_ptr, bad, prefix, E)
        bad = users.copy(); bad[1] = U
        expect(L.ERR_OOB, bad, row_ptr, items, rates, round_ptr, ask, prefix, E)
        bad = prefix.copy(); bad[0] = 0
        expect(L.ERR_ARG, users, row_ptr, items, rates, round_ptr, ask, bad, E)
        bad = prefix.copy(); bad[-1] = 3
        expect(L.ERR_ARG, users, row_ptr, items, rates, round_ptr, ask, bad, E)
        expect(L.ERR_ARG, users[[0, 0, 2]], row_ptr, items, rates, round_ptr, ask, prefix, E)      # a user twice
        expect(L.ERR_ARG, users, row_ptr, items, rates, round_ptr, ask, prefix, E,
               round_seq=np.full(ask.size, 10 ** 6, np.int64))
        expect(L.ERR_ARG, users, row_ptr, items, rates, round_ptr, ask, prefix, 0)
        m.set_frozen(AT.FROZEN_BUT_USER & ~(1 << L.Q))
        expect(L.ERR_ARG, users, row_ptr, items, rates, round_ptr, ask, prefix, E)
        m.set_frozen(AT.FROZEN_BUT_USER)
    kw["adam_mode"] = "tf1"
    with _model(U, I, D, t, **kw) as m:
        m.set_frozen(AT.FROZEN_BUT_USER)
        with pytest.raises(L.TfrError) as e:
            m.finetune_users(*s)
        assert e.value.code == L.ERR_ARG and m.step == 0
        assert np.array_equal(m.get_table(L.P), t["P"])


def test_ml1m_shaped_adaptive_run_in_one_call():
    """6040 x 3952, D 20, nll, SGD lr 5e-3; every user 20 seeded test items, budget 10, E 300, every user in one call;
    a 20-user sample against the sequential HIP driver"""
    U, I, D = 6040, 3952, 20
    rs = np.random.RandomState(1)
    t = rand_tables(rs, U, I, D, scale=0.1)
    df = per_user_frame(rs, np.arange(U), I, 20, binary=True, shuffle=False)
    kw = dict(loss="nll", optimizer="sgd", lr=5e-3, reg=0.05)
    sample = np.sort(rs.permutation(U)[:20])
    with _model(U, I, D, t, **kw) as bat:
        got = FT.adaptive_test(bat, df, budget=10, epoch_max=300, max_users=None, batched=True)
        assert len(got) == U and bat.step == U * 10 * 300
    with _model(U, I, D, t, **kw) as seq:
        want = AT.adaptive_test(seq, df[df["user"].isin(sample)], budget=10, epoch_max=300, max_users=None)
    by_user = {r["user"]: r for r in got}
    for w in want:
        g = by_user[w["user"]]
        assert g["asked"] == w["asked"] and g["outcome"] == w["outcome"]
        assert_close(g["predicted"], w["predicted"], rtol=2e-4, what="predictions of user %d" % w["user"])
        assert abs(g["mcost"] - w["mcost"]) <= 2e-3 * max(1.0, abs(w["mcost"]))
