"""Ranking and neighbours from the bf16 snapshot, host side: the three entries are declared, bound with the argument lists of
their float32 twins and wrapped; evaluate_ranking refuses bf16=True for an FM; a null model is refused before device work;
and the inverse norms of packed snapshot rows, restated in float32 NumPy (tests/bf16_rank_cases.py), are those of
tests/neighbours_ref.row_rnorm on the round-tripped table.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import bf16
from tests import bf16_rank_cases as RC
from tests import bf16_topk_cases as C
from tests import neighbours_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWINS = {"tfr_bf16_rank_items": "tfr_rank_items", "tfr_bf16_neighbours": "tfr_neighbours",
         "tfr_bf16_neighbours_dev": "tfr_neighbours_dev"}


def test_entries_are_declared_bound_and_wrapped():
    header = open(os.path.join(ROOT, "include", "tfrecomm.h")).read()
    for name, twin in TWINS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in tfrecomm.h" % name
        assert name in L.SIGNATURES, "binding missing for %s" % name
        assert L.SIGNATURES[name][0] is L.SIGNATURES[twin][0]
        assert L.SIGNATURES[name][1] == L.SIGNATURES[twin][1], "%s does not take the arguments of %s" % (name, twin)
    for method in ("rank_items_bf16", "similar_items_bf16", "similar_users_bf16", "similar_items_bf16_dev",
                   "similar_users_bf16_dev"):
        assert callable(getattr(T.SvdModel, method, None)), "SvdModel.%s is missing" % method
        twin = method.replace("_bf16", "")
        assert list(inspect.signature(getattr(T.SvdModel, method)).parameters) == \
            list(inspect.signature(getattr(T.SvdModel, twin)).parameters), method
    assert re.search(r"#define\s+TFR_ABI_VERSION\s+3\b", header)


def test_evaluate_ranking_keyword_defaults_to_float32():
    p = inspect.signature(T.evaluate_ranking).parameters
    assert "bf16" in p and p["bf16"].default is False


def test_evaluate_ranking_bf16_refuses_an_fm():
    class Fm:                                              # what evaluate_ranking reads of an FmModel before it ranks
        n_features = 50

        def rank_items(self, *a, **k):
            raise AssertionError("ranked before the refusal")

    with pytest.raises(ValueError, match="bf16"):
        T.evaluate_ranking(Fm(), [0, 1], [2, 3], item_lo=10, item_hi=50, bf16=True)

    class NoSnapshot(Fm):                                  # a model without rank_items_bf16, given without an item range
        user_num, item_num = 10, 40

    with pytest.raises(ValueError, match="bf16"):
        T.evaluate_ranking(NoSnapshot(), [0, 1], [2, 3], bf16=True)


def test_null_model_is_refused_before_device_work():
    lib = L.load()
    u = np.zeros(2, np.int32)
    ip = np.array([0, 1, 2], np.int64)
    it = np.array([3, 4], np.int32)
    out = np.full(20, 77, np.int32)
    assert lib.tfr_bf16_rank_items(None, L.ptr_i32(u), 2, L.ptr_i64(ip), L.ptr_i32(it), None, None, L.ptr_i32(out)) == L.ERR_ARG
    for which in (L.NB_ITEMS, L.NB_USERS):
        assert lib.tfr_bf16_neighbours(None, which, L.NB_METRIC["cosine"], L.ptr_i32(u), 2, 10, None, None, 0, 5, L.ptr_i32(out),
                                       None) == L.ERR_ARG
        assert lib.tfr_bf16_neighbours_dev(None, which, L.NB_METRIC["dot"], None, 2, 10, None, None, 0, 5, None, None) == L.ERR_ARG
    assert np.all(out == 77)


# ---------------------------------------------------------------- the inverse norms of packed rows
@pytest.mark.parametrize("D", C.WIDTHS)
def test_packed_rnorm_is_row_rnorm_of_the_round_tripped_table(D):
    rs = np.random.RandomState(900 + D)
    Tb = rs.normal(0, .3, (130, D)).astype(np.float32)
    Tb[3] = 0                                              # a zero row: rn 0
    Tb[5, 0] = np.float32(1 + 2.0 ** -9)                   # no bf16 number: the round trip moves it
    Tb[7] = -Tb[6]                                         # signs do not enter
    packed = bf16.pack_rows(Tb)
    rt = bf16.round_trip(Tb)
    assert packed.shape == (130, bf16.row_stride(D)) and not packed[:, D:].any()
    assert not np.array_equal(rt, Tb)
    ss, rn = RC.packed_ss(packed), RC.packed_rnorm(packed)
    assert ss.dtype == np.float32 and rn.dtype == np.float32
    want = NR.row_rnorm(rt)
    assert np.array_equal(rn.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(NR.row_rnorm(np.abs(rt)).view(np.uint32), want.view(np.uint32))     # item_abs: the same squares
    assert rn[3] == 0 and ss[3] == 0 and rn[6] == rn[7]
    # the squares of widened bf16 values are exact in float32: the float64 product is the float32 product
    x = bf16.from_bits(packed)
    assert np.array_equal((x * x).astype(np.float64), x.astype(np.float64) * x.astype(np.float64))


def test_packed_rnorm_on_exact_tables():
    rs = np.random.RandomState(7)
    for D in (8, 17, 64, 100):
        for Tb in (NR.dyadic_table(rs, 60, D), NR.pow4_table(rs, 60, D)):
            assert np.array_equal(bf16.round_trip(Tb), Tb)
            rn = RC.packed_rnorm(bf16.pack_rows(Tb))
            assert np.array_equal(rn.view(np.uint32), NR.row_rnorm(Tb).view(np.uint32))
        p4 = NR.pow4_table(rs, 60, D)
        rn = RC.packed_rnorm(bf16.pack_rows(p4))
        m, e = np.frexp(rn[rn > 0])
        assert np.all(m == 0.5)                            # powers of two: the cosine of pow4 rows is exact


def test_rank_bracket_counts():
    s = np.array([5.0, 4.0, 4.0 + 1e-7, 3.0, 1.0])
    elig = np.array([True, True, True, False, True])
    assert RC.rank_bracket(s, elig, 0, 1e-6) == (0, 0)
    assert RC.rank_bracket(s, elig, 1, 1e-6) == (1, 2)      # tied with item 2 inside the tolerance
    assert RC.rank_bracket(s, elig, 4, 1e-6) == (3, 3)      # item 3 is not eligible
