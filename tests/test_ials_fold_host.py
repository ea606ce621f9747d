"""Fold-in on the CPU (tests/ials_fold_cases.py; include/tfrecomm.h tfr_ials_fold_in): the null-handle checks of the two entry
points, fold-in as one more row of the weighted problem, the float64 restatements within an eighth of the project's constants
on every new list, and the planted faults.  No kernels are launched here."""
import numpy as np
import pytest

from tests import ials_cases as C0
from tests import ials_cg_ref as G
from tests import ials_fold_cases as F
from tests import ials_ref as R


def _tables(case, side):
    """(own, other) of a half of ``side``"""
    return (case["X"], case["Y"]) if side == 0 else (case["Y"], case["X"])


# ----------------------------------------------------------------------------- argument checks (no device work)
def test_a_null_handle_is_refused_by_both_entry_points():
    from tfrecomm_amd import _lib as L
    lib = L.load()
    assert lib.tfr_ials_fold_in(None, 0, 0, None, None, None, 0, None, None, None, None) == L.ERR_ARG
    assert lib.tfr_ials_last_error()
    assert lib.tfr_ials_export_f32(None, 0, 0, 0, None) == L.ERR_ARG


def test_the_cases_are_what_the_kernels_expect():
    for c in F.CASES:
        assert c["nu"] == F.NU and c["ni"] == F.NI
        for side in (0, 1):
            res = R.lists(c, side)
            Nres = np.diff(res[0])
            assert (Nres == 0).any() and (Nres > c["chunk"]).any(), (c["id"], side)      # an empty and a chunked resident list
            ptr, ids, vals, n_other = c["new"][side]
            N = np.diff(ptr)
            assert tuple(N) == F.lengths(c["chunk"]) and n_other == (c["ni"], c["nu"])[side]
            assert ptr[0] == 0 and (vals > 0).all() and ids.min() >= 0 and ids.max() < n_other
            for e in range(N.size):
                assert (np.diff(ids[ptr[e]:ptr[e + 1]].astype(np.int64)) > 0).all(), (c["id"], side, e)
            assert set(R.n_chunks(ptr, c["chunk"])) == {0, 2, 3}
            assert c["start"][side].shape == (N.size, c["d"])
    assert {c["d"] for c in F.CHOL_CASES} == set(F.CHOL_WIDTHS) <= set(C0.WIDTHS)
    assert {c["chunk"] for c in F.CHOL_CASES} == set(F.CHUNKS)
    assert {c["d"] for c in F.CG_CASES} == set(F.CG_WIDTHS)


# ----------------------------------------------------------------------------- one more row of the weighted problem
@pytest.mark.parametrize("cid", ["fold-chol-d1-chunk32", "fold-chol-d33-chunk32", "fold-chol-d64-chunk64"])
def test_fold_in_is_the_appended_entity_s_row_of_the_definition(cid):
    """the resident lists with the new ones appended as entities n .. n + 12: rows n .. of the definition over ALL partners
    (dense_half) are what half gives the new lists alone"""
    case = F.BY_ID[cid]
    for side in (0, 1):
        _, other = _tables(case, side)
        rp, ri, rv, n_other = R.lists(case, side)
        ptr, ids, vals, _ = new = case["new"][side]
        both = (np.concatenate((rp, rp[-1] + ptr[1:])), np.concatenate((ri, ids)), np.concatenate((rv, vals)), n_other)
        n = rp.size - 1
        a, b = R.half(other, new, case["lam"], case["alpha"]), R.dense_half(other, both, case["lam"], case["alpha"])
        tol = 64 * float(np.finfo(R.LD).eps) * b["cond"][n:] * b["xmax"][n:]
        err = np.abs(a["x"] - b["x"][n:]).max(1).astype(np.float64)
        assert (err <= tol).all(), (cid, side, float((err / np.maximum(tol, 1e-300)).max()))
        assert (a["x"][a["N"] == 0] == 0).all() and (b["x"][n:][a["N"] == 0] == 0).all()


# ----------------------------------------------------------------------------- the restatements need an eighth of the constants
@pytest.mark.parametrize("case", F.CHOL_CASES, ids=lambda c: c["id"])
def test_the_float64_half_of_the_new_lists_stays_within_an_eighth_of_K(case):
    for side in (0, 1):
        _, other = _tables(case, side)
        lst = case["new"][side]
        got = R.half_f64(other, lst, case["lam"], case["alpha"], case["chunk"])
        ref = R.half(other, lst, case["lam"], case["alpha"])
        rho = float(R.ratios(ref, got).max())
        print("RATIO %s side %d: %.3f of K / 8 = %.3f" % (case["id"], side, rho, R.K / 8.0))
        assert not R.check_half(ref, got, R.K / 8.0, "%s side %d" % (case["id"], side))


@pytest.mark.parametrize("case", F.CG_CASES, ids=lambda c: c["id"])
def test_the_float64_cg_of_the_new_lists_stays_within_an_eighth_of_K_CG(case):
    for side in (0, 1):
        _, other = _tables(case, side)
        lst = case["new"][side]
        for name, start in (("zero", np.zeros_like(case["start"][side])), ("given", case["start"][side])):
            got = G.cg_half_f64(start, other, lst, case["lam"], case["alpha"], case["steps"])
            ref = G.cg_half(start, other, lst, case["lam"], case["alpha"], case["steps"])
            rho = float(R.ratios(ref, got).max())
            print("RATIO %s side %d start %s: %.3f of K_CG / 8 = %.3f" % (case["id"], side, name, rho, G.K_CG / 8.0))
            assert not R.check_half(ref, got, G.K_CG / 8.0, "%s side %d start %s" % (case["id"], side, name))


def test_the_converged_float64_cg_stays_within_an_eighth_of_K_CONV():
    case = F.CONV_CASE
    for side in (0, 1):
        _, other = _tables(case, side)
        lst = case["new"][side]
        exact = R.half(other, lst, case["lam"], case["alpha"])
        for name, start in (("zero", np.zeros_like(case["start"][side])), ("given", case["start"][side])):
            got = G.cg_half_f64(start, other, lst, case["lam"], case["alpha"], case["steps"])
            ref = G.against_exact(start, exact)
            rho = float(R.ratios(ref, got).max())
            print("CONV side %d start %s: %.3f of K_CONV / 8 = %.3f" % (side, name, rho, G.K_CONV / 8.0))
            assert not R.check_half(ref, got, G.K_CONV / 8.0, "side %d start %s" % (side, name))


# ----------------------------------------------------------------------------- planted faults
def test_a_dropped_last_chunk_leaves_the_bound():
    case = F.BY_ID["fold-chol-d33-chunk32"]
    lst, Y = case["new"][0], case["Y"]
    ref = R.half(Y, lst, case["lam"], case["alpha"])
    assert not R.check_half(ref, R.half_f64(Y, lst, case["lam"], case["alpha"], case["chunk"]), R.K)
    bad = R.check_half(ref, R.half_f64(Y, lst, case["lam"], case["alpha"], case["chunk"], fault="drop_last_chunk"), R.K)
    assert bad, "a fold-in without the last chunk of its long lists passed"


def test_a_cold_start_where_one_was_given_leaves_the_bound():
    case = F.BY_ID["fold-cg3-d128-chunk32"]
    lst, Y, start = case["new"][0], case["Y"], case["start"][0]
    ref = G.cg_half(start, Y, lst, case["lam"], case["alpha"], case["steps"])
    assert not R.check_half(ref, G.cg_half_f64(start, Y, lst, case["lam"], case["alpha"], case["steps"]), G.K_CG)
    assert R.check_half(ref, G.cg_half_f64(start, Y, lst, case["lam"], case["alpha"], case["steps"], fault="cold_start"), G.K_CG)


def test_the_gram_of_the_wrong_side_leaves_the_bound():
    """new users are solved from G = Y^T Y: handed X^T X, as a stale Gram of the other table would be, the rows leave both
    bounds"""
    case = F.BY_ID["fold-chol-d17-chunk64"]
    lst, X, Y = case["new"][0], case["X"], case["Y"]
    ref = R.half(Y, lst, case["lam"], case["alpha"])
    assert not R.check_half(ref, R.half_f64(Y, lst, case["lam"], case["alpha"], case["chunk"], G=R.gram_f64(Y)), R.K)
    assert R.check_half(ref, R.half_f64(Y, lst, case["lam"], case["alpha"], case["chunk"], G=R.gram_f64(X)), R.K)
    cg = F.BY_ID["fold-cg3-d33-chunk32"]
    lst, X, Y, start = cg["new"][0], cg["X"], cg["Y"], cg["start"][0]
    ref = G.cg_half(start, Y, lst, cg["lam"], cg["alpha"], cg["steps"])
    assert not R.check_half(ref, G.cg_half_f64(start, Y, lst, cg["lam"], cg["alpha"], cg["steps"], G=G.gram_f64(Y)), G.K_CG)
    assert R.check_half(ref, G.cg_half_f64(start, Y, lst, cg["lam"], cg["alpha"], cg["steps"], G=G.gram_f64(X)), G.K_CG)
