"""k_finetune (tfr_finetune_users / SvdModel.finetune_users) per step: every user's gradient, Adam moments and apply, the
call's outputs and the state it must leave alone, each held to its own statement (tests/finetune_step_ref.py) around calls
of one step - at every register width, at the edges of the 64-row pass loop in the staged and in the streamed form, with
either half of the user side frozen and with saturated logits; and a launch of several rounds and steps tied to such
single steps bit for bit."""
import ctypes as C
import time

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import adaptive_test as AT
from oracle import svd_oracle as so
from tests import finetune_step_ref as FR
from tests import step_ref as R
from tests.util import rand_tables

pytestmark = pytest.mark.gpu

U_, I_ = 40, 200
LAM_ = 0.1
START = 500                                          # a late position: one step more or less moves sqrt(1 - b2p) by ~1e-3
B1, B2 = so.BETA1, so.BETA2


def _rows_staged(D, max_rows):
    """tfr_finetune_plan's rows_staged for a call whose longest user with rounds has max_rows rows: the kernel stages the
    users with at most that many rows and streams the others"""
    lds, staged, wpb = C.c_int64(), C.c_int32(), C.c_int32()
    assert L.load().tfr_finetune_plan(D, max_rows, C.byref(lds), C.byref(staged), C.byref(wpb)) == L.OK
    return staged.value


def _cap(D):
    """the most rows tfr_finetune_plan stages at this width"""
    return _rows_staged(D, 1 << 20)


PASS_EDGES = {1, 63, 64, 65, 128, 129}


def _forms(D, rows, calls):
    """(staged, streamed): the prefixes of the two calls by the form their user takes in its call.  A call stages the users
    with at most rows_staged = min(cap, the longest user with a round) rows"""
    staged, streamed = set(), set()
    for prefixes in calls:
        limit = _rows_staged(D, max(n for n, p in zip(rows, prefixes) if p))
        for n, p in zip(rows, prefixes):
            (staged if n <= limit else streamed).update(p)
    return staged, streamed


def _model(D, t, opt):
    lazy = opt == "lazy"
    m = T.SvdModel(U_, I_, D, optimizer="adam" if lazy else "sgd", adam_mode="lazy", lr=_lr(opt), reg=LAM_, **t["flags"])
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    return m


def _lr(opt):
    return 5e-3 if opt == "lazy" else 2.0 ** -8      # SGD: a power of two, so that lr * g is exact (step_ref.grad_from_sgd)


def _snapshot(m, adam):
    out = {}
    for name in R.NAMES:
        tid = R.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        out[name] = d
    return out


def _state_bits(m, adam):
    st = _snapshot(m, adam)
    return [st[name][slot] for name in FR.USER_TABLES for slot in sorted(st[name])]


def _same(a, b):
    return all(R.same_bits(p, q) for p, q in zip(a, b)) and len(a) == len(b)


# ----------------------------------------------------------------------------- (a), (b): one step per call, per row
def _check_two_calls(D, loss, opt, item_abs, reg_bias, frozen=AT.FROZEN_BUT_USER, tag="", start=START):
    """Five users (three idle waves in the second block), seven under nll with two users of saturated logits.  Schedule
    users: A 129 rows (prefix 129, then 128), B 70 rows (64, 65), C 63 rows (63, 1), D 5 rows (1, then no round: its
    moments must stay), E (no round, then 7 rows: a first step from zero moments beside second ones); under nll S+ and S-
    with bu = +-25 (4 rows; 4, 3).  Where the staging holds 129 rows (D = 20) A, B and C are staged, so every pass edge
    runs in the staged form, and E has one row more than the staging holds, so the call streams too; at every other width
    A, B and C are streamed, every pass edge in the streamed form, and E has 7 rows."""
    t0 = time.time()
    adam = opt == "lazy"
    cap = _cap(D)
    rs = np.random.RandomState(7 * D + 1)
    t = rand_tables(rs, U_, I_, D, scale=0.3 / np.sqrt(D / 8.0))
    t["flags"] = dict(loss=loss, item_abs=item_abs, reg_bias=reg_bias)
    rows = [129, 70, 63, 5, cap + 1 if cap >= 129 else 7]
    calls = [[[129], [64], [63], [1], []], [[128], [65], [1], [], [7]]]
    users = rs.permutation(U_)[:7]
    groups = [[0, 1, 2, 3, 4]]
    if loss == "nll":
        rows += [4, 4]
        calls = [calls[0] + [[4], [4]], calls[1] + [[3], [3]]]
        t["bu"][users[5]], t["bu"][users[6]] = 25.0, -25.0
        groups.append([5, 6])
    users = users[:len(rows)]
    # which form each user takes, by the plan of its own call: every pass edge staged at the narrow width, streamed at the
    # wide ones, and both forms in one launch everywhere
    assert {20: 170, 64: 57, 256: 13}.get(D, cap) == cap
    staged, streamed = _forms(D, rows, calls)
    assert PASS_EDGES <= (staged if D == 20 else streamed), (D, cap, sorted(staged), sorted(streamed))
    assert staged and streamed, (D, cap, sorted(staged), sorted(streamed))
    assert cap >= 129 if D == 20 else 7 <= cap < 63  # no width between: A, B and C take one form together
    drawn = FR.draw_rows(rs, I_, rows, loss == "nll")
    assert np.unique(drawn[1][:129]).size < 129      # row items repeat
    kw = dict(adam=adam, loss=loss, item_abs=item_abs, reg_bias=reg_bias, lam=LAM_, lr=_lr(opt), frozen=frozen)
    with _model(D, t, opt) as m:
        m.set_frozen(frozen)
        m.set_step(start, *FR.powers_at(B1, B2, B1, B2, start))
        before = _snapshot(m, adam)
        for call, prefixes in enumerate(calls):
            s = FR.schedule(rs, users, I_, drawn, prefixes)
            step0, b1p, b2p = m.get_step()
            outs = m.finetune_users(*s)
            after = _snapshot(m, adam)
            n_rounds = int(s[4][-1])
            assert m.get_step() == (step0 + n_rounds,) + (FR.powers_at(b1p, b2p, B1, B2, n_rounds) if adam else (b1p, b2p))
            report = {}
            bad = FR.check_call(before, after, s, outs, powers0=(b1p, b2p), fresh=call == 0, groups=groups, report=report, **kw)
            FR.print_ratios("%sD%d-%s-%s call%d" % (tag, D, loss, opt, call), report)
            assert not bad, "D %d, call %d:\n  %s" % (D, call, "\n  ".join(bad))
            before = after
    print("TIME %sD%d-%s-%s %.1f s" % (tag, D, loss, opt, time.time() - t0))


@pytest.mark.parametrize("D,loss,opt,item_abs,reg_bias", FR.STEP_CASES)
def test_one_step_per_call_per_row(D, loss, opt, item_abs, reg_bias):
    _check_two_calls(D, loss, opt, item_abs, reg_bias)


@pytest.mark.parametrize("D", [20, 132])
def test_one_step_per_call_at_an_early_position(D):
    """at position 500 beta1's power has vanished against 1 (1 - 0.9^501 == 1 in float32), so only beta2's is judged there;
    after two steps both move lr_t by tens of per cent from one position to the next"""
    _check_two_calls(D, "nll", "lazy", True, D == 20, tag="early-", start=2)


@pytest.mark.parametrize("half", ["P", "bu"])
@pytest.mark.parametrize("opt", ["sgd", "lazy"])
@pytest.mark.parametrize("D", [20, 132])             # NJ = 1 and NJ = 3
def test_a_frozen_half_keeps_its_bits_and_the_other_half_trains(D, opt, half):
    _check_two_calls(D, "nll" if half == "P" else "mse", opt, True, True, frozen=AT.FROZEN_BUT_USER | 1 << R.TID[half],
                     tag="frozen-%s-" % half)


# ----------------------------------------------------------------------------- (c), (d): a launch composes its steps
E_ = 3
START_C = 2                                          # an early position: both beta powers still move lr_t from step to step


def _rounds_schedule(D):
    """five users with 2 to 4 rounds, prefixes that shrink and grow; user 0 is streamed, user 2 staged at the cap (two
    passes at D = 20), the others staged"""
    cap = _cap(D)
    rs = np.random.RandomState(3 * D)
    n0, n2 = cap + 1, min(cap, 66)
    rows = [n0, 3, n2, 9, 2]
    prefixes = [[n0, n0 // 2, 1, n0 - 1], [1, 3], [n2, 2, n2 - 1], [9, 4, 9, 1], [2, 1]]
    users = rs.permutation(U_)[:5]
    drawn = FR.draw_rows(rs, I_, rows, True)
    return rs, FR.schedule(rs, users, I_, drawn, prefixes, nsteps=E_)


def _within_user(round_ptr):
    """the index of every round within its user"""
    return np.concatenate([np.arange(b - a) for a, b in zip(round_ptr[:-1], round_ptr[1:])]).astype(np.int64)


@pytest.mark.parametrize("opt", ["sgd", "lazy"])
@pytest.mark.parametrize("D", [20, 132])
def test_a_launch_of_rounds_and_steps_equals_its_single_steps_bit_for_bit(D, opt):
    """A: one launch, E steps a round.  B: one launch, every round written as E rounds of one step.  C: one call per (round,
    step) with the beta powers set by the host's recurrence.  The same bits throughout: what a wave carries in registers from
    step to step and from round to round equals what goes through memory, and the kernel's b1p *= b1 equals the replay.
    A fourth model runs A without the optional outputs: the same ask logits and state."""
    adam = opt == "lazy"
    rs, sA = _rounds_schedule(D)
    users, row_ptr, items, rates, round_ptr, ask, prefix, E = sA
    t = rand_tables(rs, U_, I_, D, scale=0.3 / np.sqrt(D / 8.0))
    t["flags"] = dict(loss="nll", item_abs=True, reg_bias=True)
    j_of = _within_user(round_ptr)
    p0 = FR.powers_at(B1, B2, B1, B2, START_C)
    with _model(D, t, opt) as a, _model(D, t, opt) as b, _model(D, t, opt) as c, _model(D, t, opt) as d:
        for m in (a, b, c, d):
            m.set_frozen(AT.FROZEN_BUT_USER)
            m.set_step(START_C, *p0)
        askA, lossA, finalA = a.finetune_users(*sA, round_seq=j_of * E)
        bitsA = _state_bits(a, adam)
        assert all(np.isfinite(x).all() for x in bitsA) and np.isfinite(askA).all() and np.isfinite(lossA).all()
        # (d) the optional outputs off: the same ask logits and state
        askD, lossD, finalD = d.finetune_users(*sA, round_seq=j_of * E, want_loss=False, want_final=False)
        assert lossD is None and finalD is None
        assert R.same_bits(askD, askA) and _same(_state_bits(d, adam), bitsA) and d.get_step() == a.get_step()
        # B
        rep = lambda x: np.repeat(x, E)
        sB = (users, row_ptr, items, rates, round_ptr * E, rep(ask), rep(prefix), 1)
        seqB = rep(j_of * E) + np.tile(np.arange(E), j_of.size)
        askB, lossB, finalB = b.finetune_users(*sB, round_seq=seqB)
        assert _same(_state_bits(b, adam), bitsA)
        assert b.get_step() == a.get_step()
        assert R.same_bits(askB[::E], askA)
        assert R.same_bits(lossB[E - 1::E], lossA)
        assert np.array_equal(finalB, finalA, equal_nan=True) and np.isnan(finalA).any() and not np.isnan(finalA).all()
        # C
        n_rounds_of = np.diff(round_ptr)
        for pos in range(int(n_rounds_of.max()) * E):
            j, e = divmod(pos, E)
            xs = np.flatnonzero(n_rounds_of > j)
            ks = round_ptr[xs] + j
            rp = np.concatenate(([0], np.cumsum(row_ptr[xs + 1] - row_ptr[xs])))
            pick = np.concatenate([np.arange(row_ptr[x], row_ptr[x + 1]) for x in xs])
            if adam:
                c.set_step(START_C + pos, *FR.powers_at(p0[0], p0[1], B1, B2, pos))
            askC, lossC, finalC = c.finetune_users(users[xs], rp, items[pick], rates[pick], np.arange(xs.size + 1), ask[ks],
                                                   prefix[ks], 1, round_seq=np.zeros(xs.size, np.int64))
            if e == 0:
                assert R.same_bits(askC, askA[ks]), (pos, askC, askA[ks])
            if e == E - 1:
                assert R.same_bits(lossC, lossA[ks]), (pos, lossC, lossA[ks])
                for y, x in enumerate(xs):
                    if n_rounds_of[x] == j + 1:            # the user's last round: A's final logits are this step's
                        assert np.array_equal(finalC[rp[y]:rp[y + 1]], finalA[row_ptr[x]:row_ptr[x + 1]], equal_nan=True), (pos, x)
        assert _same(_state_bits(c, adam), bitsA)
