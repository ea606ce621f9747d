"""Top-K from the bf16 snapshot, host side: the bindings, the width list of the GPU tests held to the tile's paths, the
exactness of the bit-for-bit cases shown on the CPU, and the tile's fragment indexing restated in NumPy.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import bf16
from tests import bf16_topk_cases as C
from tests import sliced_cases as SC
from tests import widths as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "tfrecomm.h")).read()
    for name in ("tfr_bf16_topk", "tfr_bf16_topk_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in tfrecomm.h" % name
        assert name in L.SIGNATURES, "binding missing for %s" % name
    assert len(L.SIGNATURES["tfr_bf16_topk"][1]) == len(L.SIGNATURES["tfr_topk"][1]) == 8
    assert len(L.SIGNATURES["tfr_bf16_topk_dev"][1]) == len(L.SIGNATURES["tfr_topk_dev"][1]) == 8
    for method in ("recommend_bf16", "recommend_bf16_dev"):
        assert callable(getattr(T.SvdModel, method, None)), "SvdModel.%s is missing" % method
    assert re.search(r"#define\s+TFR_ABI_VERSION\s+3\b", header)


def test_null_model_is_refused_before_device_work():
    lib = L.load()
    u, out = np.zeros(3, np.int32), np.zeros(30, np.int32)
    assert lib.tfr_bf16_topk(None, L.ptr_i32(u), 3, 10, None, None, L.ptr_i32(out), None) == L.ERR_ARG
    assert lib.tfr_bf16_topk_dev(None, None, 3, 10, None, None, None, None) == L.ERR_ARG


# ---------------------------------------------------------------- the width list
def test_tile_classes_restated():
    assert [C.fragments(D) for D in (1, 8, 9, 17, 24, 64, 100, 256)] == [1, 1, 2, 3, 3, 8, 13, 32]
    assert [C.k_steps(D) for D in (1, 8, 9, 17, 24, 64, 100, 256)] == [1, 1, 1, 2, 2, 4, 7, 16]
    assert C.tile_class(8) == (True, "1 steps, one group") and C.tile_class(9) == (False, "1 steps, one group")
    assert C.tile_class(56) == (True, "4 steps, one group") and C.tile_class(64) == (False, "4 steps, one group")
    assert C.tile_class(100) == (True, "last group ends at 3") and C.tile_class(256) == (False, "last group ends at 0")


def test_widths_reach_every_tile_class():
    supported = [D for D in range(1, 257) if C.supported(D)]
    reachable = {C.tile_class(D) for D in supported}
    assert len(reachable) == 16                            # odd / even x (1, 2, 3, 4 steps; last group ends at 0, 1, 2, 3)
    assert all(C.supported(D) for D in C.WIDTHS), [D for D in C.WIDTHS if not C.supported(D)]
    missing = sorted(reachable - {C.tile_class(D) for D in C.WIDTHS}, key=str)
    assert not missing, "no width reaches %s" % missing
    assert set(C.WIDTHS) >= {1, 8, 9, 16, 17, 24, 33, 64, 100, 128, 132, 200, 252, 256}
    # a pad inside the last fragment, a whole row of fragments, and the widest row
    assert any(D % 8 for D in C.WIDTHS) and any(D % 8 == 0 for D in C.WIDTHS) and max(C.WIDTHS) == 256


def test_the_gpu_tests_read_this_list():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_bf16_topk.py")).read())
    used = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "C"}
    assert "WIDTHS" in used


# ---------------------------------------------------------------- exactness of the bit-for-bit cases
def test_dyadic_generator_is_the_float32_tests_own():
    from tests.test_gpu_topk import dyadic
    for step in (.25, .125):
        assert np.array_equal(C.dyadic(np.random.RandomState(3), (7, 9), step), dyadic(np.random.RandomState(3), (7, 9), step))


@pytest.mark.parametrize("D", C.WIDTHS)
def test_dyadic_tables_are_exact_in_any_order(D):
    rs = np.random.RandomState(D)
    t = C.dyadic_tables(rs, 70, 900, D)
    assert C.dyadic_faults(t) == []
    users = np.arange(70)
    for item_abs in (False, True):
        Qp = np.abs(t["Q"]) if item_abs else t["Q"]
        S = C.svd_scores(t["P"], t["Q"], t["bu"], t["bi"], t["mu"], users, item_abs)
        S64 = t["P"].astype(np.float64) @ Qp.astype(np.float64).T + 0.25 + t["bu"].astype(np.float64)[:, None] \
            + t["bi"].astype(np.float64)[None, :]
        assert np.array_equal(S.astype(np.float64), S64)
        # the float32 sum of the products in descending feature order: another order, the same bits
        rev = np.zeros((70, 900), np.float32)
        for f in range(D - 1, -1, -1):
            rev = (rev + t["P"][:, f:f + 1] * Qp[None, :, f]).astype(np.float32)
        assert np.array_equal(rev.astype(np.float64), t["P"].astype(np.float64) @ Qp.astype(np.float64).T)


def test_a_fault_in_the_dyadic_tables_is_named():
    t = C.dyadic_tables(np.random.RandomState(0), 5, 6, 8)
    P = t["P"].copy()
    P[0, 0] = np.float32(1.0 + 2.0 ** -9)
    assert "rows are bf16-exact" in C.dyadic_faults(dict(t, P=P))


@pytest.mark.parametrize("c", SC.CASES, ids=repr)
def test_sliced_cases_stay_exact_after_the_round_trip(c):
    """a user's row has one non-zero feature, so a score is one bf16 product (exact in float32) plus three small dyadics;
    the float32 chain of the reference then has to equal float64 on the round-tripped tables as it does on the originals"""
    S, S64 = C.sliced_scores(c.name), C.sliced_scores_f64(c.name)
    assert S.shape == S64.shape == (SC.NU, c.I)
    nan = np.isnan(S64)
    assert np.array_equal(np.isnan(S), nan)
    assert np.array_equal(S[~nan].astype(np.float64), S64[~nan])
    t = C.sliced_tables(c.name)
    assert np.array_equal(bf16.round_trip(t["Q"]), t["Q"]) and np.array_equal(t["P"], c.tables()["P"])
    assert c.D in (8, 9)                                   # one fragment with the upper half zero, and two fragments
    assert C.tile_class(c.D) == ((True, "1 steps, one group") if c.D == 8 else (False, "1 steps, one group"))


def test_sliced_cases_still_order_by_their_patterns():
    """the round trip moves values (4 i above 256 is no bf16 number), so the reference is recomputed on the round-tripped
    tables; it still differs from user to user and fills k places where the original does"""
    for c in SC.CASES:
        wi, _ = C.sliced_reference(c.name)
        oi, _ = c.reference()
        assert np.array_equal(wi >= 0, oi >= 0), c.name
        assert len({tuple(r) for r in wi.tolist()}) > 4, c.name


# ---------------------------------------------------------------- fragment indexing
@pytest.mark.parametrize("D", C.WIDTHS)
def test_fragment_walk_sums_to_the_plain_dot(D):
    rs = np.random.RandomState(500 + D)
    P = rs.randint(-8, 9, (6, D)).astype(np.float32)
    Q = rs.randint(-8, 9, (5, D)).astype(np.float32)
    pp, qq = bf16.pack_rows(P), bf16.pack_rows(Q)
    assert pp.shape[1] == 8 * C.fragments(D) and not pp[:, D:].any() and not qq[:, D:].any()
    want = P.astype(np.float64) @ Q.astype(np.float64).T
    got = np.array([[C.fragment_dot(pp[u], qq[i], D) for i in range(5)] for u in range(6)])
    assert np.array_equal(got, want)
    assert 2 * C.k_steps(D) - C.fragments(D) == (1 if C.tile_class(D)[0] else 0)   # the fragments the walk zeroes
