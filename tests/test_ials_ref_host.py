"""The iALS restatements against each other on the CPU (tests/ials_ref.py, tests/ials_cases.py): the decomposed form against
the definition, the float64 kernel-order form against the longdouble reference (this measures K and K_LOSS), the loss going
down, the planted faults, the width list, and the argument checks of tfr_ials_create, which come before any device work."""
import ctypes as C_
import functools
import math

import numpy as np
import pytest

from tests import ials_cases as C
from tests import ials_ref as R

BY_ID = {c["id"]: c for c in C.CASES}
DENSE = [BY_ID[i] for i in C.DENSE_IDS]


# ----------------------------------------------------------------------------- widths
def slot_class(d):
    """(live A-entry slots, end of the range): ials_accumulate keeps entry t = tid + 256 q of A in acc[q], so
    ceil(d * d / 256) of its 16 slots are live (csrc/ials.hip).  A range of widths with the same count is run at its lowest
    and at its highest d."""
    key = lambda x: -(-x * x // 256)
    first = d == 1 or key(d - 1) != key(d)
    last = d == R.MAXD or key(d + 1) != key(d)
    return key(d), "lowest d" if first else "highest d" if last else "inside"


def test_the_widths_reach_both_ends_of_every_slot_count():
    assert all(1 <= d <= R.MAXD for d in C.WIDTHS)
    reachable = {slot_class(d) for d in range(1, R.MAXD + 1)}
    assert {c[0] for c in reachable} == set(range(1, 17))
    wanted = {c for c in reachable if c[1] != "inside"}
    missing = sorted(wanted - {slot_class(d) for d in C.WIDTHS})
    assert not missing, "WIDTHS: no width reaches %s" % missing
    assert {1, 32, 33, 63, 64} <= set(C.WIDTHS)
    assert {c["d"] for c in C.CASES if c["id"].startswith("widths")} == set(C.WIDTHS)


def test_the_cases_are_what_the_kernels_expect():
    for c in C.CASES + [C.trajectory()]:
        N = np.diff(c["indptr"])
        assert c["indptr"][0] == 0 and (N >= 0).all() and (c["vals"] > 0).all() and c["items"].max() < c["ni"]
        inner = np.ones(c["items"].size, bool)
        inner[c["indptr"][:-1][N > 0]] = False
        assert (np.diff(c["items"].astype(np.int64))[inner[1:]] > 0).all(), c["id"]
    for ch, d in C.CHUNK_CASES:
        for cid in ("chunk%d-d%d" % (ch, d), "chunk%d-d%d-swapped" % (ch, d)):
            got = set(R.n_chunks(BY_ID[cid]["indptr"], ch))
            assert got >= ({0, 2, 3, 4} if not cid.endswith("swapped") else {0, 2}), (cid, got)
    long_ = BY_ID["long-d9"]
    assert set(R.n_chunks(long_["indptr"], 512)) == {0, 2, 3}
    assert R.gram_slice_rows(131072) == 128 and R.gram_slice_rows(131073) == 160 and R.gram_slice_rows(1) == 128


# ----------------------------------------------------------------------------- the decomposition is the definition
@pytest.mark.parametrize("case", DENSE, ids=lambda c: c["id"])
def test_the_decomposed_half_equals_the_definition(case):
    lu = R.lists(case, 0)
    a, b = R.half(case["Y"], lu, case["lam"], case["alpha"]), R.dense_half(case["Y"], lu, case["lam"], case["alpha"])
    # both are longdouble Cholesky solves of the same system, summed in another order: eps_LD cond |x| with a margin of 64
    tol = 64 * float(np.finfo(R.LD).eps) * b["cond"] * b["xmax"]
    err = np.abs(a["x"] - b["x"]).max(1).astype(np.float64)
    assert (err <= tol).all(), (case["id"], float((err / np.maximum(tol, 1e-300)).max()))
    assert (a["x"][a["N"] == 0] == 0).all() and (b["x"][b["N"] == 0] == 0).all()


@pytest.mark.parametrize("case", DENSE, ids=lambda c: c["id"])
def test_the_loss_formula_equals_the_definition(case):
    a, b = R.loss(case["X"], case["Y"], case), R.loss_dense(case["X"], case["Y"], case)
    n_terms = case["nu"] * case["ni"] * case["d"]
    assert abs(a - b) <= n_terms * float(np.finfo(R.LD).eps) * R.loss_terms(case["X"], case["Y"], case)


# ----------------------------------------------------------------------------- float64 against longdouble: K and K_LOSS
@functools.lru_cache(maxsize=None)
def _measured():
    """(max rho_x, where, max rho_loss, where) over every small case, one sweep, half by half (the item half fed the
    float64 X), and over two iterations of the dense cases"""
    best_x, best_l = (0.0, ""), (0.0, "")
    for case in C.CASES:
        iters = 2 if case["id"] in C.DENSE_IDS else 1
        X, Y = case["X"], case["Y"]
        lu, li = R.lists(case, 0), R.lists(case, 1)
        for it in range(iters):
            for what, lst, side in (("user half", lu, 0), ("item half", li, 1)):
                other = Y if side == 0 else X
                got = R.half_f64(other, lst, case["lam"], case["alpha"], case["chunk"])
                ref = R.half(other, lst, case["lam"], case["alpha"])
                rho = float(R.ratios(ref, got).max())
                if rho > best_x[0]:
                    best_x = (rho, "%s, %s, iteration %d" % (case["id"], what, it))
                if side == 0:
                    X = got
                else:
                    Y = got
                if case["id"] in C.DENSE_IDS:
                    rl = abs(R.LD(R.loss_f64(X, Y, case)) - R.loss(X, Y, case)) / (R.EPS * R.loss_terms(X, Y, case))
                    if rl > best_l[0]:
                        best_l = (float(rl), "%s, after the %s of iteration %d" % (case["id"], what, it))
    return best_x + best_l


def test_K_is_eight_times_what_the_float64_restatement_needs():
    rho_x, where_x, rho_l, where_l = _measured()
    print("MEASURED rho_x %.3f (%s), rho_loss %.3f (%s)" % (rho_x, where_x, rho_l, where_l))
    assert R.K >= 8 * rho_x, "K = %g < 8 * %.3f (%s)" % (R.K, rho_x, where_x)
    assert R.K_LOSS >= 8 * rho_l, "K_LOSS = %g < 8 * %.3f (%s)" % (R.K_LOSS, rho_l, where_l)
    assert R.K == math.ceil(8 * R.MEASURED_RHO_X) and abs(rho_x - R.MEASURED_RHO_X) <= 0.02 * R.MEASURED_RHO_X, rho_x
    assert R.K_LOSS == math.ceil(8 * R.MEASURED_RHO_LOSS) and abs(rho_l - R.MEASURED_RHO_LOSS) <= 0.02 * R.MEASURED_RHO_LOSS, rho_l


@pytest.mark.parametrize("fault,cid", [("drop_partial_tile", "widths-d33"), ("skip_slot15", "widths-d64"),
                                       ("drop_last_chunk", "chunk32-d9"), ("unit_confidence", "widths-d17"),
                                       ("no_ridge", "conditioning-lam0.1-alpha40"), ("drop_last_slice", "long-d9")])
def test_a_planted_fault_leaves_the_bound(fault, cid):
    case = BY_ID[cid]
    lu = R.lists(case, 0)
    ref = R.half(case["Y"], lu, case["lam"], case["alpha"])
    assert not R.check_half(ref, R.half_f64(case["Y"], lu, case["lam"], case["alpha"], case["chunk"]), R.K, cid)
    assert R.check_half(ref, R.half_f64(case["Y"], lu, case["lam"], case["alpha"], case["chunk"], fault=fault), R.K, cid)


# ----------------------------------------------------------------------------- the loss goes down
@pytest.mark.parametrize("case", [c for c in DENSE if c["lam"] >= 1e-3], ids=lambda c: c["id"])
def test_the_loss_does_not_increase_over_either_half_of_five_iterations(case):
    X, Y = case["X"], case["Y"]
    lu, li = R.lists(case, 0), R.lists(case, 1)
    last = R.loss(X, Y, case)
    for it in range(5):
        for side, lst in ((0, lu), (1, li)):
            if side == 0:
                X = R.half_f64(Y, lst, case["lam"], case["alpha"], case["chunk"])
            else:
                Y = R.half_f64(X, lst, case["lam"], case["alpha"], case["chunk"])
            now = R.loss(X, Y, case)
            assert now <= last + R.K_LOSS * R.EPS * R.loss_terms(X, Y, case), (case["id"], it, side, float(last), float(now))
            last = now


def test_the_trajectory_case_is_well_conditioned():
    """the GPU trajectory test compares at 1e-9 relative: over its ten iterations cond2(A) stays below 1e4"""
    case = C.trajectory()
    X, Y = case["X"], case["Y"]
    lu, li = R.lists(case, 0), R.lists(case, 1)
    worst = 0.0
    for _ in range(10):
        ref = R.half(Y, lu, case["lam"], case["alpha"])
        X = R.half_f64(Y, lu, case["lam"], case["alpha"], case["chunk"])
        worst = max(worst, float(ref["cond"].max()))
        ref = R.half(X, li, case["lam"], case["alpha"])
        Y = R.half_f64(X, li, case["lam"], case["alpha"], case["chunk"])
        worst = max(worst, float(ref["cond"].max()))
    assert worst <= 1e4, worst


# ----------------------------------------------------------------------------- argument checks (no device work)
def test_bad_arguments_to_create_are_refused_before_any_device_work():
    from tfrecomm_amd import _lib as L
    lib = L.load()
    good = dict(nu=4, ni=4, d=8, lam=0.1, alpha=40.0)
    for bad in (dict(d=0), dict(d=65), dict(d=-1), dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(alpha=-0.5),
                dict(alpha=float("inf")), dict(nu=0), dict(ni=0), dict(nu=2 ** 31)):
        a = dict(good, **bad)
        h = L._p()
        rc = lib.tfr_ials_create(C_.byref(h), a["nu"], a["ni"], a["d"], a["lam"], a["alpha"], 0)
        assert rc == L.ERR_ARG and not h.value, bad
        assert lib.tfr_ials_last_error()
    assert lib.tfr_ials_create(None, 4, 4, 8, 0.1, 40.0, 0) == L.ERR_ARG
    assert lib.tfr_ials_destroy(None) == L.OK
    for fn, args in ((lib.tfr_ials_half, (None, 0, None)), (lib.tfr_ials_sweep, (None, 1, None)), (lib.tfr_ials_loss, (None, None)),
                     (lib.tfr_ials_load, (None, None, None, None, 0)), (lib.tfr_ials_gram, (None, 0, None))):
        assert fn(*args) == L.ERR_ARG


def test_the_python_class_is_exported():
    import tfrecomm_amd as T
    assert T.ImplicitALS.__module__.endswith("ials") and "ImplicitALS" in T.__all__
