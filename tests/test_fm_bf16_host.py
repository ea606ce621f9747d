"""The FM on the bf16 snapshot, host side: the entries, bindings and wrappers against their float32 twins, the width list of
the GPU tests held to the kernel's lane classes, the kernel's order of operations restated in float32 NumPy and held to the
project's per-row bound, the quantisation statement run in float64 on the GPU tests' own inputs, and the exactness of the
bit-for-bit cases shown on the CPU.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import bf16
from tests import bf16_topk_cases as TC
from tests import fm_bf16_cases as C
from tests import fm_ref as FR
from tests import step_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWINS = {"tfr_fm_bf16_forward": "tfr_fm_forward", "tfr_fm_bf16_forward_dev": "tfr_fm_forward_dev",
         "tfr_fm_bf16_predict_resident": "tfr_fm_predict_resident",
         "tfr_fm_bf16_eval_binary_resident": "tfr_fm_eval_binary_resident", "tfr_fm_bf16_topk": "tfr_fm_topk"}
OWN = ("tfr_fm_bf16_snapshot", "tfr_fm_bf16_drop", "tfr_fm_bf16_get_rows")
WRAPPERS = {"forward_csr_bf16": "forward_csr", "fma_bf16": "fma", "forward_bf16_dev": "forward_dev",
            "predict_resident_bf16": "predict_resident", "eval_binary_resident_bf16": "eval_binary_resident",
            "topk_bf16": "topk", "get_ranking_bf16": "get_ranking"}


def _declaration(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, "%s is not declared in tfrecomm.h" % name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def _types(args):
    """the parameter types of a declaration, names dropped"""
    return [re.sub(r"\s*\b\w+$", "", a) for a in args]


def test_entries_are_declared_bound_and_wrapped_like_their_twins():
    header = open(os.path.join(ROOT, "include", "tfrecomm.h")).read()
    for name in OWN + tuple(TWINS):
        args = _declaration(header, name)
        assert args[0].startswith("tfr_fm*"), "%s must take the FM handle first" % name
        assert name in L.SIGNATURES, "binding missing for %s" % name
    for name, twin in TWINS.items():
        assert _types(_declaration(header, name)) == _types(_declaration(header, twin)), name
        assert L.SIGNATURES[name] == L.SIGNATURES[twin], name
    assert L.SIGNATURES["tfr_fm_bf16_snapshot"][1] == L.SIGNATURES["tfr_fm_bf16_drop"][1] == [L._p]
    assert len(L.SIGNATURES["tfr_fm_bf16_get_rows"][1]) == 3
    for method, twin in WRAPPERS.items():
        assert callable(getattr(T.FmModel, method, None)), "FmModel.%s is missing" % method
        assert str(inspect.signature(getattr(T.FmModel, method))) == str(inspect.signature(getattr(T.FmModel, twin))), method
    for method in ("snapshot_bf16", "drop_bf16", "bf16_rows"):
        assert list(inspect.signature(getattr(T.FmModel, method)).parameters) == ["self"], method
    assert re.search(r"#define\s+TFR_ABI_VERSION\s+3\b", header)


def test_null_handle_is_refused_before_device_work():
    lib = L.load()
    z64, z32, zf = np.zeros(2, np.int64), np.zeros(1, np.int32), np.zeros(1, np.float32)
    h16 = np.zeros(8, np.uint16)
    assert lib.tfr_fm_bf16_snapshot(None) == L.ERR_ARG
    assert lib.tfr_fm_bf16_drop(None) == L.ERR_ARG
    assert lib.tfr_fm_bf16_get_rows(None, h16.ctypes.data_as(L.SIGNATURES["tfr_fm_bf16_get_rows"][1][1]), 8) == L.ERR_ARG
    assert lib.tfr_fm_bf16_forward(None, L.ptr_i64(z64), L.ptr_i32(z32), L.ptr_f32(zf), 1, L.ptr_f32(zf)) == L.ERR_ARG
    assert lib.tfr_fm_bf16_forward_dev(None, None, None, None, 0, None) == L.ERR_ARG
    assert lib.tfr_fm_bf16_predict_resident(None, 1, L.ptr_f32(zf)) == L.ERR_ARG
    assert lib.tfr_fm_bf16_eval_binary_resident(None, None, None, None, None) == L.ERR_ARG
    assert lib.tfr_fm_bf16_topk(None, L.ptr_i32(z32), 1, 0, 1, 1, None, None, L.ptr_i32(z32), None) == L.ERR_ARG
    assert b"null" in lib.tfr_fm_last_error()


def test_the_switch_is_listed_with_the_others():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    api = open(os.path.join(ROOT, "tf-recomm_amd", "csrc", "api.hip")).read()
    assert "TFR_FM_BF16_NTV" in api and "`TFR_FM_BF16_NTV" in design


# ---------------------------------------------------------------- the width list
def test_widths_reach_every_lane_class():
    from tests.test_width_coverage import SUPPORTED, bf16_class
    reachable = {bf16_class(D) for D in SUPPORTED}
    assert len(reachable) == 10
    assert {bf16_class(D) for D in C.WIDTHS} == reachable
    assert all(D in SUPPORTED for D in C.WIDTHS + C.TOPK_WIDTHS)
    assert {D % 8 == 0 for D in C.TOPK_WIDTHS} == {True, False} and max(C.TOPK_WIDTHS) > 128


def test_the_gpu_tests_read_this_list():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_fm_bf16.py")).read())
    used = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "C"}
    assert {"WIDTHS", "TOPK_WIDTHS", "design", "stride_design"} <= used


def test_the_grid_cap_is_the_launchers():
    src = open(os.path.join(ROOT, "tf-recomm_amd", "csrc", "fm_bf16.hip")).read()
    m = re.search(r"fm_bf16_grid\(.*?blocks_for\(n_rows, 256 / G, (\d+)\)", src, flags=re.S)
    assert m and int(m.group(1)) == C.GRID_CAP
    for G in (1, 32):
        indptr, _, _ = C.stride_design(G)
        assert indptr.size - 1 > C.GRID_CAP * (256 // G)


# ---------------------------------------------------------------- the kernel's order of operations
@pytest.mark.parametrize("D", C.WIDTHS)
def test_the_kernels_order_holds_the_per_row_bound(D):
    """float32 in the kernel's lane geometry (8 elements per lane, G lanes, spare lanes) on round-tripped V, against float64
    on the same V: inside fm_ref.forward_excess's limit, which the float32 restatement in CSR order sets"""
    mu, Wt, V = C.tables(D)
    Vrt = bf16.round_trip(V)
    indptr, indices, data = C.design()
    y = C.kernel_f32(mu, Wt, Vrt, indptr, indices, data)
    rep = {}
    bad = FR.forward_excess(y, mu, Wt, Vrt, indptr, indices, data, report=rep)
    print("RATIO kernel order D%d dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
        D, rep["forward"]["dev"]["short"], rep["forward"]["dev"]["long"], rep["forward"]["c_ref"]["short"], rep["forward"]["c_ref"]["long"]))
    assert not bad, bad
    assert y[0] == mu                                     # the empty row
    # a planted fault is seen: a spare lane that is not zeroed, a pad that is not +0
    if bf16.lanes(D) * 8 > bf16.row_stride(D):
        t = FR.forward_terms(mu, Wt, Vrt, indptr, indices, data)
        extra = 0.5 * (t["S"][:, :8] ** 2).sum(1)
        assert FR.forward_excess(y + extra.astype(np.float32), mu, Wt, Vrt, indptr, indices, data)


def test_the_kernels_order_differs_from_csr_order_only_in_rounding():
    """on the dyadic inputs both orders give the float64 value exactly"""
    D = 100
    mu, Wt, V = C.dyadic_model(D)
    indptr, indices, data = C.dyadic_design()
    y = C.kernel_f32(mu, Wt, V, indptr, indices, data)
    want = FR.forward_terms(mu, Wt, V, indptr, indices, data)["y"]
    assert np.array_equal(y.astype(np.float64), want)
    assert np.array_equal(FR.f32_fm(mu, Wt, V, indptr, indices, data)["y"].astype(np.float64), want)


# ---------------------------------------------------------------- exactness of the bit-for-bit cases
@pytest.mark.parametrize("D", C.WIDTHS)
def test_dyadic_inputs_are_exact_in_any_order(D):
    mu, Wt, V = C.dyadic_model(D)
    indptr, indices, data = C.dyadic_design()
    assert C.dyadic_faults(mu, Wt, V, indptr, indices, data) == []
    assert np.array_equal(bf16.pack_rows(V)[:, :D], bf16.to_bits(V))
    want = FR.forward_terms(mu, Wt, V, indptr, indices, data)["y"]
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)          # the float64 prediction is a float32
    assert np.unique(want).size > 300                                                # and the rows differ
    # the guard sees inputs that are not exact
    assert C.dyadic_faults(mu, Wt, V + np.float32(1 / 3), indptr, indices, data)
    assert C.dyadic_faults(mu, Wt, V, indptr, indices, data * np.float32(300))


@pytest.mark.parametrize("D", C.TOPK_WIDTHS)
def test_dyadic_topk_tables_are_exact(D):
    t = C.topk_tables(D)
    assert TC.dyadic_faults(dict(P=t["V"], Q=t["V"], bu=t["W"], bi=t["W"], mu=t["mu"])) == []
    assert TC.dyadic_faults(dict(P=t["V"] + np.float32(0.001), Q=t["V"], bu=t["W"], bi=t["W"], mu=t["mu"]))


# ---------------------------------------------------------------- what rounding V to bf16 may move
@pytest.mark.parametrize("D", C.WIDTHS)
def test_quantisation_statement_in_float64(D):
    """|fm(round_trip(V)) - fm(V)| per row, both in float64, against the two terms of fm_bf16_cases.quantisation_bound on the
    GPU test's own inputs"""
    mu, Wt, V = C.tables(D)
    indptr, indices, data = C.design()
    first, second = C.quantisation_bound(mu, Wt, V, indptr, indices, data)
    y = FR.forward_terms(mu, Wt, V, indptr, indices, data)["y"]
    yq = FR.forward_terms(mu, Wt, bf16.round_trip(V), indptr, indices, data)["y"]
    diff = np.abs(yq - y)
    two = np.diff(indptr) >= 2                            # 0.5 (s^2 - q) vanishes on a row of one entry, whatever V
    assert np.all(diff[~two] <= 1e-15)
    frac = diff[two] / first[two]
    print("QUANT D%d: max |diff| / first term %.3f, mean %.3f, max second / first %.2e" % (
        D, frac.max(), frac.mean(), (second[two] / first[two]).max()))
    assert np.all(diff <= first + second)
    assert frac.max() > 0.01                              # the statement is not vacuous: rounding moves these rows
