"""The per-step statements of tests/finetune_step_ref.py, themselves tested on the CPU: a float32 NumPy restatement of two
successive one-step calls in k_finetune's operation order passes every statement at the pass edges of the 64-row loop, and
the same restatement with one planted error is reported under the statement that error belongs to."""
import numpy as np
import pytest

from oracle import svd_oracle as so
from tests import finetune_step_ref as FR
from tests import step_ref as R
from tests import widths as W
from tests.util import rand_tables

U_, I_ = 8, 400
LAM_ = 0.1
START = 500                                          # the calls start at the beta powers after 500 steps
FROZEN_BUT_USER = 1 << so.MU | 1 << so.BI | 1 << so.QF
USERS = (5, 2, 7)                                    # schedule order; users 0, 1, 3, 4, 6 stay outside the call


def _two_calls(D, L, loss, opt, fault=None, frozen=FROZEN_BUT_USER, spoil=None, report=None):
    """user 5 trains on the first L of its L + 3 rows, user 2 has rows and no round, user 7 trains on all of its 9 rows (the
    round at position 1); then a second call from the moments the first left, user 2 now with a round.  Returns the violated
    statements of both calls."""
    adam = opt == "lazy"
    lr = 5e-3 if adam else 2.0 ** -9
    rs = np.random.RandomState(1000 * D + L)
    t = rand_tables(rs, U_, I_, D, scale=0.3)
    st = FR.zero_state(t, adam)
    drawn = FR.draw_rows(rs, I_, [L + 3, 4, 9], loss == "nll")
    powers = FR.powers_at(so.BETA1, so.BETA2, so.BETA1, so.BETA2, START)
    kw = dict(adam=adam, loss=loss, item_abs=True, reg_bias=True, lam=LAM_, lr=lr, frozen=frozen)
    bad = []
    for call, prefixes in enumerate(([[L], [], [9]], [[L], [2], [8]])):
        s = FR.schedule(rs, USERS, I_, drawn, prefixes)
        new, outs, end = FR.execute(st, s, powers0=powers, fault=fault, **kw)
        if spoil is not None:
            spoil(new)
        rep = {} if report is not None else None
        got = FR.check_call(st, new, s, outs, powers0=powers, fresh=call == 0, report=rep, **kw)
        if report is not None:
            report["call%d" % call] = rep
        bad += ["call %d: %s" % (call, b) for b in got]
        st, powers = new, end
    return bad


@pytest.mark.parametrize("opt", ["sgd", "lazy"])
@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 129, 300])
@pytest.mark.parametrize("D", [5, 20, 68])
def test_the_executor_passes_every_statement(D, L, loss, opt):
    report = {}
    bad = _two_calls(D, L, loss, opt, report=report)
    for call, rep in sorted(report.items()):
        FR.print_ratios("D%d-L%d-%s-%s %s" % (D, L, loss, opt, call), rep)
    assert not bad, "\n  ".join(bad)


def _other_users_float(new):
    new["P"]["w"][3, 1] = np.nextafter(new["P"]["w"][3, 1], np.float32(9))      # user 3 is outside the call


def _frozen_p(new):
    new["P"]["w"][5, 0] = np.nextafter(new["P"]["w"][5, 0], np.float32(9))      # user 5 trains in both calls


# planted error -> (optimisers it is planted under, executor fault, change of the result, extra frozen bits, the words
# every violated statement must contain)
PLANTED = {
    "row 64 of a 129-row prefix dropped": (("sgd", "lazy"), "drop_row64", None, 0, "gradient"),
    "lam * p once per step": (("sgd", "lazy"), "lam_once", None, 0, "P gradient"),
    "beta powers one step late": (("lazy",), "late_powers", None, 0, "w does not follow from m and v"),
    "reg_bias ignored on bu": (("sgd", "lazy"), "no_reg_bias", None, 0, "bu gradient"),
    "b1 used for v": (("lazy",), "v_with_b1", None, 0, "v does not follow from g and the previous v"),
    "item_abs ignored for the asked row": (("sgd", "lazy"), "ask_no_abs", None, 0, "ask logit"),
    "one float of another user's row changed": (("sgd", "lazy"), None, _other_users_float, 0, "users outside the call changed"),
    "a frozen P changed": (("sgd", "lazy"), None, _frozen_p, 1 << so.PF, "P.w: a frozen table changed"),
}


@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("planted,opt", [(p, o) for p in sorted(PLANTED) for o in PLANTED[p][0]])
def test_planted_errors_are_reported_by_name(planted, opt, loss):
    """Each error, planted in the executor's two calls at D = 20 and a 129-row prefix (item_abs and reg_bias on), violates
    the statement it belongs to and no other: a wrong gradient sum leaves moments and apply consistent with it, wrong
    powers leave gradient and moments alone."""
    _, fault, spoil, extra, words = PLANTED[planted]
    bad = _two_calls(20, 129, loss, opt, fault=fault, frozen=FROZEN_BUT_USER | extra, spoil=spoil)
    print("%s (%s, %s): %d statements violated, first: %s" % (planted, loss, opt, len(bad), bad[:1]))
    assert bad, "%s passes every statement" % planted
    assert all(words in b for b in bad), "\n  ".join(bad)


def test_frozen_halves_pass_and_keep_their_bits():
    for opt in ("sgd", "lazy"):
        for half in (so.PF, so.BU):
            assert not _two_calls(20, 65, "nll", opt, frozen=FROZEN_BUT_USER | 1 << half)


def test_the_gpu_cases_reach_every_flag_at_several_widths():
    cases = FR.STEP_CASES
    assert {c[0] for c in cases} == set(W.FINETUNE)
    for D in W.FINETUNE:
        assert {c[2] for c in cases if c[0] == D} == {"sgd", "lazy"}
    for col, values in ((1, ("mse", "nll")), (3, (False, True)), (4, (False, True))):
        for v in values:
            assert sum(c[col] == v for c in cases) >= 2, (col, v)
    for loss in ("mse", "nll"):
        for opt in ("sgd", "lazy"):
            assert sum(c[1] == loss and c[2] == opt for c in cases) >= 2, (loss, opt)


def test_powers_at_is_the_float32_recurrence():
    b1p, b2p = np.float32(so.BETA1), np.float32(so.BETA2)
    for _ in range(7):
        b1p, b2p = np.float32(b1p * R.B1F), np.float32(b2p * R.B2F)
    assert FR.powers_at(so.BETA1, so.BETA2, so.BETA1, so.BETA2, 7) == (float(b1p), float(b2p))
    assert FR.powers_at(0.5, 0.75, so.BETA1, so.BETA2, 0) == (0.5, 0.75)
