"""The conjugate-gradient restatements against each other on the CPU (tests/ials_cg_ref.py, tests/ials_cg_cases.py): float64
in the kernels' order against the longdouble iterate at the same step count (this measures K_CG), the converged run against
the exact minimiser (K_CONV), the wide loss (K_LOSS_WIDE), the planted faults, the loss going down along the trajectory, the
width lists, and the argument checks of tfr_ials_create_cg, which come before any device work."""
import ctypes as C_
import functools
import math

import numpy as np
import pytest

from tests import ials_cases as C0
from tests import ials_cg_cases as C
from tests import ials_cg_ref as G
from tests import ials_ref as R

BY_ID = {c["id"]: c for c in C.CASES + C.CONV_CASES}


def _sides(case):
    return ((0, "user half", R.lists(case, 0)), (1, "item half", R.lists(case, 1)))


# ----------------------------------------------------------------------------- the lists reach every edge
def test_the_widths_reach_both_ends_of_every_lane_and_tile_count():
    for widths, count in ((C.WIDTHS, G.lane_components), (C.GRAM_WIDTHS, G.gram_tiles)):
        assert all(1 <= d <= G.MAXD for d in widths)
        for k in range(1, 5):
            ends = {min(d for d in range(1, G.MAXD + 1) if count(d) == k), max(d for d in range(1, G.MAXD + 1) if count(d) == k)}
            assert ends <= set(widths), (k, ends)
    assert {1, R.GRAM_NARROW, R.GRAM_NARROW + 1} <= set(C.GRAM_WIDTHS)       # both Gram kernels at their ends
    assert {c["d"] for c in C.CASES if c["id"].startswith("cg-widths")} == set(C.WIDTHS)
    assert {c["d"] for c in C.CASES if c["id"].startswith("cg-long")} == set(C.LONG_WIDTHS)
    assert {0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65} <= set(C.LENGTHS)
    assert set(np.diff(BY_ID["cg-widths-d65"]["indptr"])) == set(C.LENGTHS)
    assert {511, 512, 513, 1024, 1025, 1100} <= set(np.diff(BY_ID["cg-long-d65"]["indptr"]))
    assert all(d <= 33 for d in C.CONV_WIDTHS)


def test_the_longdouble_iterate_converges_to_the_exact_minimiser():
    """the reference of K_CG is the algorithm of the header: run to 3 d steps it is ials_ref.half's solution"""
    case = BY_ID["cg-conv-d9"]
    for side, what, lst in _sides(case):
        own, other = (case["X"], case["Y"]) if side == 0 else (case["Y"], case["X"])
        ref = R.half(other, lst, case["lam"], case["alpha"])
        got = G.cg_half(own, other, lst, case["lam"], case["alpha"], 27)
        assert not R.check_half(G.against_exact(own, ref), got["x"], 1.0, what)
        assert got["used"].max() <= 27 and (got["x"][got["N"] == 0] == 0).all()


# ----------------------------------------------------------------------------- float64 against longdouble: the three K
@functools.lru_cache(maxsize=None)
def _measured_cg():
    """(max ratio, where) of cg_half_f64 against cg_half at the same steps, over every case, both halves from the case's own
    tables, each restatement with its own Gram (computed once per half, like cond2(A), and shared by the step counts)"""
    best = (0.0, "")
    for case in C.CASES:
        for side, what, lst in _sides(case):
            own, other = (case["X"], case["Y"]) if side == 0 else (case["Y"], case["X"])
            g64, gld = G.gram_f64(other), R.gram(other)
            cond = G.conds(other, lst, case["lam"], case["alpha"], g64)
            for steps in C.STEPS:
                got = G.cg_half_f64(own, other, lst, case["lam"], case["alpha"], steps, G=g64)
                ref = G.cg_half(own, other, lst, case["lam"], case["alpha"], steps, G=gld, cond=cond)
                rho = float(R.ratios(ref, got).max())
                assert (got[ref["N"] == 0] == 0).all()
                if rho > best[0]:
                    best = (rho, "%s, %s, %d steps" % (case["id"], what, steps))
    return best


@functools.lru_cache(maxsize=None)
def _measured_conv():
    best = (0.0, "")
    for case in C.CONV_CASES:
        tabs = [case["X"], case["Y"]]
        for side, what, lst in _sides(case):
            own, other = tabs[side], tabs[1 - side]
            got = G.cg_half_f64(own, other, lst, case["lam"], case["alpha"], 3 * case["d"])
            ref = G.against_exact(own, R.half(other, lst, case["lam"], case["alpha"]))
            rho = float(R.ratios(ref, got).max())
            if rho > best[0]:
                best = (rho, "%s, %s" % (case["id"], what))
            tabs[side] = got
    return best


@functools.lru_cache(maxsize=None)
def _measured_loss():
    best = (0.0, "")
    for cid in C.LOSS_IDS:
        case = {c["id"]: c for c in C.CASES}[cid]
        X, Y = case["X"], case["Y"]
        for when in ("as set", "after one sweep of 3 steps"):
            rl = float(abs(R.LD(G.loss_f64(X, Y, case)) - R.loss(X, Y, case)) / (R.EPS * R.loss_terms(X, Y, case)))
            if rl > best[0]:
                best = (rl, "%s, %s" % (cid, when))
            if when == "as set":
                X, Y = G.sweep_f64(case, X, Y, 3)
    return best


@pytest.mark.parametrize("which", ["cg", "conv", "loss"])
def test_each_K_is_eight_times_what_the_float64_restatement_needs(which):
    measure, k, figure = {"cg": (_measured_cg, G.K_CG, G.MEASURED_RHO_CG), "conv": (_measured_conv, G.K_CONV, G.MEASURED_RHO_CONV),
                          "loss": (_measured_loss, G.K_LOSS_WIDE, G.MEASURED_RHO_LOSS_WIDE)}[which]
    rho, where = measure()
    print("MEASURED %s rho %.3f (%s)" % (which, rho, where))
    assert k >= 8 * rho, "K = %g < 8 * %.3f (%s)" % (k, rho, where)
    assert k == math.ceil(8 * figure) and abs(rho - figure) <= 0.02 * figure, rho


# ----------------------------------------------------------------------------- planted faults
@pytest.mark.parametrize("fault,cid,steps", [("no_ridge_in_Ap", "cg-widths-d65", 1), ("c_for_w", "cg-widths-d65", 1),
                                             ("no_beta", "cg-widths-d65", 2), ("cold_start", "cg-widths-d65", 3),
                                             ("drop_last_wave", "cg-widths-d65", 1), ("drop_last_tile", "cg-widths-d65", 1),
                                             ("drop_last_wave", "cg-long-d256-normal", 3), ("drop_last_tile", "cg-long-d256-normal", 3)])
def test_a_planted_fault_leaves_the_bound(fault, cid, steps):
    case = BY_ID[cid]
    lu = R.lists(case, 0)
    ref = G.cg_half(case["X"], case["Y"], lu, case["lam"], case["alpha"], steps)
    assert not R.check_half(ref, G.cg_half_f64(case["X"], case["Y"], lu, case["lam"], case["alpha"], steps), G.K_CG, cid)
    bad = G.cg_half_f64(case["X"], case["Y"], lu, case["lam"], case["alpha"], steps, fault=fault)
    assert R.check_half(ref, bad, G.K_CG, cid)


def test_no_beta_is_invisible_at_one_step():
    """(rn / rs) first enters the second direction: the one-step iterates are the same bits"""
    case = BY_ID["cg-widths-d65"]
    lu = R.lists(case, 0)
    a = G.cg_half_f64(case["X"], case["Y"], lu, case["lam"], case["alpha"], 1)
    assert a.tobytes() == G.cg_half_f64(case["X"], case["Y"], lu, case["lam"], case["alpha"], 1, fault="no_beta").tobytes()


def test_the_wide_gram_restatement_is_symmetric_and_within_its_bound():
    assert G.gram_f64 is R.gram_f64                        # nothing else restates the Gram
    rs = np.random.RandomState(3)
    for n, d in ((129, 65), (300, 129), (5, 256)):
        T = rs.uniform(-1.0, 1.0, (n, d))
        got = G.gram_f64(T)
        assert got.tobytes() == got.T.copy().tobytes()
        assert (np.abs(got.astype(R.LD) - R.gram(T)).astype(np.float64) <= R.gram_bound(T)).all()
        err = np.abs(G.gram_f64(T, "drop_last_tile").astype(R.LD) - R.gram(T)).astype(np.float64)
        assert not (err <= R.gram_bound(T)).all()


# ----------------------------------------------------------------------------- the stop rule
def test_the_stop_rule_ends_a_long_run_and_keeps_it_finite():
    """3 d steps asked: the rule ends every row once its residual is at the rounding level of its start; without any exit
    the longdouble recurrence is the one that the header's note describes"""
    worst = 0
    for case in C.CONV_CASES:
        for side, what, lst in _sides(case):
            own, other = (case["X"], case["Y"]) if side == 0 else (case["Y"], case["X"])
            got = G.cg_half_f64(own, other, lst, case["lam"], case["alpha"], 3 * case["d"])
            assert np.isfinite(got).all(), (case["id"], what)
            ref = G.cg_half(own, other, lst, case["lam"], case["alpha"], 3 * case["d"])
            assert np.isfinite(ref["x"].astype(np.float64)).all()
            worst = max(worst, int(ref["used"].max()))
    print("longest run: %d steps" % worst)
    assert worst < 3 * 33


# ----------------------------------------------------------------------------- the loss goes down
def test_the_loss_does_not_rise_over_any_half_of_the_trajectory():
    """ten iterations at d = 8, lambda = 0.1, alpha = 40, 3 steps: a CG step from the row as it stands never raises that
    row's quadratic, so no half raises the loss"""
    case = C0.trajectory()
    X, Y = case["X"], case["Y"]
    lu, li = R.lists(case, 0), R.lists(case, 1)
    last = first = R.loss(X, Y, case)
    for it in range(10):
        for side in (0, 1):
            if side == 0:
                X = G.cg_half_f64(X, Y, lu, case["lam"], case["alpha"], 3)
            else:
                Y = G.cg_half_f64(Y, X, li, case["lam"], case["alpha"], 3)
            now = R.loss(X, Y, case)
            assert now <= last + R.K_LOSS * R.EPS * R.loss_terms(X, Y, case), (it, side, float(last), float(now))
            last = now
    ex, ey = R.sweep_f64(case, case["X"], case["Y"], 10)
    exact = R.loss(ex, ey, case)
    print("trajectory loss: %.1f -> %.1f over twenty halves; ten exact iterations reach %.1f" % (first, last, exact))
    assert exact <= last < 1.1 * exact


# ----------------------------------------------------------------------------- argument checks (no device work)
def test_bad_arguments_to_create_cg_are_refused_before_any_device_work():
    from tfrecomm_amd import _lib as L
    lib = L.load()
    good = dict(nu=4, ni=4, d=128, lam=0.1, alpha=40.0, steps=3)
    for bad in (dict(d=0), dict(d=257), dict(d=-1), dict(steps=0), dict(steps=1025), dict(steps=-3), dict(lam=0.0), dict(lam=-1.0),
                dict(lam=float("nan")), dict(alpha=-0.5), dict(alpha=float("inf")), dict(nu=0), dict(ni=0), dict(nu=2 ** 31)):
        a = dict(good, **bad)
        h = L._p()
        rc = lib.tfr_ials_create_cg(C_.byref(h), a["nu"], a["ni"], a["d"], a["lam"], a["alpha"], a["steps"], 0)
        assert rc == L.ERR_ARG and not h.value, bad
        assert lib.tfr_ials_last_error()
    assert lib.tfr_ials_create_cg(None, 4, 4, 8, 0.1, 40.0, 3, 0) == L.ERR_ARG
    assert lib.tfr_version() == 3


def test_the_python_class_takes_the_solver():
    import inspect
    import tfrecomm_amd as T
    sig = inspect.signature(T.ImplicitALS.__init__).parameters
    assert sig["solver"].default == "cholesky" and sig["cg_steps"].default == 3
    with pytest.raises(ValueError):
        T.ImplicitALS(4, 4, factors=8, solver="lu")
