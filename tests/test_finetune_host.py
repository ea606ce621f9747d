"""Batched per-user fine-tuning, host side (no GPU): the schedule the drivers reduce to, executed one user at a time on the
float64 oracle, gives bit for bit what the sequential drivers give on the same oracle; schedule and argument checks before
any device work; the refusals of the batched drivers (tfrecomm_amd.finetune); the launch plan of tfr_finetune_plan."""
import ctypes as C
import random

import numpy as np
import pytest

from tfrecomm_amd import _lib as L
from tfrecomm_amd import adaptive_test as AT
from tfrecomm_amd import finetune as FT
from tfrecomm_amd import cats
from tests.finetune_ref import OracleDriverModel, frame, per_user_frame
from tests.util import rand_tables

DIMS = [d for d in range(1, 257) if d % 4 == 0 or d <= 64]
OPTS = [dict(optimizer="sgd", lr=0.05, reg=0.1),
        dict(optimizer="adam", adam_mode="lazy", lr=0.02, reg=0.05)]


def _pair(U, I, D, seed, **kw):
    t = rand_tables(np.random.RandomState(seed), U, I, D)
    return OracleDriverModel(U, I, D, t, **kw), OracleDriverModel(U, I, D, t, **kw)


def _same_state(a, b):
    for x, y in zip(a.user_state(), b.user_state()):
        assert np.array_equal(x, y)
    assert (a.o.step, a.o.b1p, a.o.b2p) == (b.o.step, b.o.b1p, b.o.b2p)
    assert np.array_equal(a.o.Q, b.o.Q) and np.array_equal(a.o.bi, b.o.bi) and a.o.mu == b.o.mu


@pytest.mark.parametrize("opt", OPTS, ids=["sgd", "lazy"])
@pytest.mark.parametrize("loss,max_user", [("nll", None), ("mse", 9), ("nll", 4)])
def test_non_adaptive_schedule_is_the_sequential_driver_on_the_oracle(opt, loss, max_user):
    U, I, D, E = 14, 30, 5, 4
    rs = np.random.RandomState(3)
    df = per_user_frame(rs, rs.permutation(U)[:10], I, 6, binary=loss == "nll")     # users interleaved in the frame
    if max_user is not None:                                                         # grouped, so that max_user cuts late
        df = df.sort_values("user", kind="stable").reset_index(drop=True)
    seq, bat = _pair(U, I, D, 7, loss=loss, reg_bias=True, **opt)
    ls, lb = [], []
    want = AT.non_adaptive_test(seq, df, epoch_max=E, max_user=max_user, log=ls.append)
    got = FT.non_adaptive_test(bat, df, epoch_max=E, max_user=max_user, log=lb.append, batched=True)
    assert len(got["pred"]) > 0
    assert got["pred"] == want["pred"] and got["truth"] == want["truth"]
    assert got["accuracy"] == want["accuracy"] and (got["auc"] == want["auc"] or np.isnan(want["auc"]))
    assert lb == ls
    _same_state(seq, bat)


@pytest.mark.parametrize("opt", OPTS, ids=["sgd", "lazy"])
@pytest.mark.parametrize("selector,everything", [(cats.Next, False), (cats.Random, False), (cats.Popular, False),
                                                 (cats.Next, True), (cats.Random, True)])
def test_adaptive_schedule_is_the_sequential_driver_on_the_oracle(opt, selector, everything):
    U, I, D, E, B = 12, 40, 4, 3, 4
    rs = np.random.RandomState(5)
    df = per_user_frame(rs, [7, 2, 9, 0, 4], I, 7, binary=True)
    pop = rs.randint(0, 100, I)
    seq, bat = _pair(U, I, D, 11, loss="nll", item_abs=True, **opt)
    ls, lb = [], []
    random.seed(42)
    want = AT.adaptive_test(seq, df, budget=B, epoch_max=E, selector=selector, max_users=4, ask_everything=everything,
                            popularity=pop, log=ls.append)
    random.seed(42)
    got = FT.adaptive_test(bat, df, budget=B, epoch_max=E, selector=selector, max_users=4, ask_everything=everything,
                           popularity=pop, log=lb.append, batched=True)
    assert got == want and lb == ls
    assert [r["size"] for r in got] == [7 if everything else B] * 4
    _same_state(seq, bat)


def test_user_order_inside_the_schedule_does_not_matter():
    U, I, D = 10, 25, 3
    rs = np.random.RandomState(8)
    df = frame(rs, U, I, 60, binary=False)
    a, b = _pair(U, I, D, 2, loss="mse", optimizer="adam", adam_mode="lazy", lr=0.05)
    a.user_order, b.user_order = "reversed", "forward"
    ra = FT.non_adaptive_test(a, df, epoch_max=3, batched=True)
    rb = FT.non_adaptive_test(b, df, epoch_max=3, batched=True)
    assert ra["pred"] == rb["pred"] and ra["accuracy"] == rb["accuracy"]
    _same_state(a, b)


def test_unbatched_calls_are_the_sequential_drivers():
    U, I, D = 10, 25, 3
    df = frame(np.random.RandomState(6), U, I, 40, binary=True)
    a, b = _pair(U, I, D, 1, loss="nll", optimizer="adam", adam_mode="tf1", lr=0.05)
    ra, rb = AT.non_adaptive_test(a, df, epoch_max=3), FT.non_adaptive_test(b, df, epoch_max=3)
    assert ra["pred"] == rb["pred"]
    _same_state(a, b)
    a, b = _pair(U, I, D, 1, loss="nll", optimizer="sgd", lr=0.05)
    assert AT.adaptive_test(a, df, budget=2, epoch_max=3) == FT.adaptive_test(b, df, budget=2, epoch_max=3)


def test_schedule_ids_are_checked_before_any_narrowing():
    df = frame(np.random.RandomState(0), 6, 20, 25, binary=True)
    s, _ = FT.non_adaptive_schedule(df.assign(item=df["item"].astype(np.int64) + (1 << 32)), epoch_max=2)
    with pytest.raises(L.OutOfRangeError):                # an id past int32 is out of range, not wrapped around
        s.validate(6, 20)


def test_schedules():
    df = frame(np.random.RandomState(0), 6, 20, 25, binary=True)
    s, rr = FT.non_adaptive_schedule(df, epoch_max=5, max_user=3)
    kept = int(np.argmax(df["user"].values > 3)) if (df["user"] > 3).any() else len(df)
    assert s.n_rounds == kept == rr.size and s.validate(6, 20) is s
    assert np.array_equal(np.sort(s.seq), np.arange(kept) * 5)
    assert np.array_equal(s.ask[rr], df["item"].values[:kept]) and np.array_equal(s.items, s.ask)
    s, out = FT.adaptive_schedule(df, budget=2, epoch_max=7, max_users=None, ask_everything=True)
    assert s.users.size == df["user"].nunique() and s.prefix.tolist() == np.repeat(np.diff(s.row_ptr), 2).tolist()
    assert s.seq.tolist() == [7 * k for k in range(s.n_rounds)]


def test_bad_schedules_are_rejected_before_the_model_is_touched():
    U, I, D = 8, 12, 3
    rs = np.random.RandomState(1)
    df = per_user_frame(rs, [1, 5, 3], I, 4, binary=True)
    m, ref = _pair(U, I, D, 0, loss="nll", optimizer="sgd", lr=0.1)
    with pytest.raises(ValueError, match="budget"):              # the sequential driver trains users 1 and 5 first
        FT.adaptive_test(m, df, budget=5, epoch_max=2, max_users=None, batched=True)
    with pytest.raises(ValueError, match="freeze"):
        FT.non_adaptive_test(m, df, epoch_max=2, freeze=False, batched=True)
    with pytest.raises(L.OutOfRangeError):
        FT.non_adaptive_test(m, df.assign(item=df["item"] + I - 2), epoch_max=2, batched=True)
    with pytest.raises(L.OutOfRangeError):
        FT.adaptive_test(m, df.assign(user=df["user"] + U - 3), budget=2, epoch_max=2, batched=True)
    _same_state(m, ref)
    assert m.o.frozen == 0
    tf1, _ = _pair(U, I, D, 0, loss="nll", optimizer="adam", adam_mode="tf1")
    with pytest.raises(ValueError, match="tf1"):
        FT.adaptive_test(tf1, df, budget=2, epoch_max=2, batched=True)
    with pytest.raises(ValueError, match="tf1"):
        FT.non_adaptive_test(tf1, df, epoch_max=2, batched=True)
    s, _ = FT.non_adaptive_schedule(df, epoch_max=3)
    for field, bad in (("prefix", lambda p: p + 10), ("prefix", lambda p: p * 0), ("round_ptr", lambda p: p[::-1]),
                       ("seq", lambda q: q + 10 ** 6), ("users", lambda u: u * 0)):
        t, _ = FT.non_adaptive_schedule(df, epoch_max=3)
        setattr(t, field, bad(getattr(t, field)))
        with pytest.raises(ValueError):
            t.validate(U, I)
    s.validate(U, I)


def _plan(dim, rows):
    lds, staged, wpb = C.c_int64(), C.c_int32(), C.c_int32()
    rc = L.load().tfr_finetune_plan(dim, rows, C.byref(lds), C.byref(staged), C.byref(wpb))
    return rc, lds.value, staged.value, wpb.value


def test_plan_fits_every_shape():
    for dim in DIMS:
        for rows in (0, 1, 10, 20, 63, 64, 65, 300, 3000, 10 ** 6):
            rc, lds, staged, wpb = _plan(dim, rows)
            assert rc == L.OK, (dim, rows)
            assert 0 < lds <= 64 * 1024 and wpb >= 1 and 0 <= staged <= rows, (dim, rows, lds, staged, wpb)
            # the staged rows and the fixed per-wave arrays fit what is requested
            need = wpb * 4 * (2 * ((dim + 3) // 4 * 4) + 128 + staged * ((dim | 1) + 2))
            assert need <= lds <= 160 * 1024
        assert _plan(dim, 10)[2] == 10                     # the ML-1M adaptive shapes are staged at every dim


def test_plan_refuses_bad_dims():
    for dim in (0, -4, 65, 67, 260, 300):
        assert _plan(dim, 10)[0] == L.ERR_ARG
    assert _plan(20, -1)[0] == L.ERR_ARG


def test_entry_rejects_a_null_model():
    lib = L.load()
    z = np.zeros(2, np.int64)
    one = np.zeros(1, np.int32)
    f = np.zeros(1, np.float32)
    assert lib.tfr_finetune_users(None, 1, L.ptr_i32(one), L.ptr_i64(z), None, None, L.ptr_i64(z), None, None, None, 1,
                                  L.ptr_f32(f), None, None) == L.ERR_ARG
