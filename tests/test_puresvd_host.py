"""PureSVD without a device: the restatement (tests/puresvd_ref.py) against np.linalg.svd and the exact block answer, the
float64-against-long-double ratios the constants of the GPU tests come from, the reference's own pivots and sweeps, the case
shapes against tfr_psvd_plan, and the argument checks the library makes before any device work."""
import ctypes as C

import numpy as np
import pytest

from tfrecomm_amd import _lib as L
from tfrecomm_amd import puresvd
from tests import puresvd_cases as PC
from tests import puresvd_ref as R


def test_plan_and_the_case_shapes_hit_its_edges():
    p = PC.plan()
    assert p["r"] == 80 and p["lanes"] == 64 and p["chunk"] % 64 == 0 and 64 % p["ahead"] == 0 and p["lds_bytes"] <= 160 * 1024
    assert puresvd.plan(10, 10, 100, 28)["lds_bytes"] <= 160 * 1024
    edges = PC.lane_edges()
    assert edges == {64: (1, 128)}                                              # a whole wave per row at every width
    assert all(2 * lanes >= hi for lanes, (_, hi) in edges.items())          # two columns per lane cover the width
    w = PC.product_widths()
    assert {1, 32, 33, 64, 65, 128}.issubset(w) and any(v % 2 for v in w if v > 1) and all(lo in w and hi in w for lo, hi in edges.values())
    lengths = PC.product_lengths()
    ch, ah = p["chunk"], p["ahead"]
    assert {0, 1, 63, 64, 65, ah - 1, ah + 1, ch - 1, ch, ch + 1, 2 * ch + 1} == set(lengths)
    indptr, ids, n_rows, n_cols = PC.product_lists()
    assert np.diff(indptr)[:len(lengths)].tolist() == lengths and ids.max() < n_cols
    assert all((np.diff(ids[indptr[e]:indptr[e + 1]]) > 0).all() for e in range(n_rows))
    for name, (n, r) in PC.ORTH_SHAPES.items():
        assert n >= r
    assert {r for _, r in PC.ORTH_SHAPES.values()} >= {1, 5, 24, 128}          # narrow Gram, tiled, two tiles per side
    for bad in ((0, 5), (5, -1), (100, 29)):
        with pytest.raises(L.TfrError) as e:
            puresvd.plan(10, 10, *bad)
        assert e.value.code == L.ERR_ARG and "r = factors + oversample" in str(e.value)


def test_the_gram_partial_buffer_holds_the_slices_of_both_sides():
    """tfr_psvd_plan's gram_slices is the figure the fit reserves (csrc/puresvd.h psvd_gram_slices, the one function both
    call).  The ALS slice rule is not monotonic in n - 128 rows per slice up to 131072 rows, then steps of 32 - so the side with
    more rows can have fewer slices, and the buffer must hold the larger count of the two, not the count of the larger side."""
    from tests import ials_ref

    def slices(n):
        return -(-n // ials_ref.gram_slice_rows(n))
    assert slices(131072) == 1024 and slices(131073) == 820 and slices(120000) == 938 and slices(200000) == 893
    for nu, ni in ((200000, 120000), (120000, 200000), (131073, 131072), (131072, 131073), (131073, 10), (6040, 3706), (70, 90),
                   (2 ** 31 - 1, 1), (1, 2 ** 31 - 1), (2 ** 31 - 1, 131072)):
        got = puresvd.plan(nu, ni, 64, 16)["gram_slices"]
        assert got == max(slices(nu), slices(ni)) and got >= slices(nu) and got >= slices(ni) and got <= 1024, (nu, ni, got)


def test_the_product_s_order_shows_in_the_bits():
    """the planted orders (each list backwards, long lists unchunked) change bits of the cases' products: the GPU test's
    equality is a statement about the order"""
    indptr, ids, n_rows, n_cols = PC.product_lists()
    ch = PC.plan()["chunk"]
    B = PC.product_block(n_cols, 7)
    want = R.spmm(indptr, ids, B, ch)
    assert np.isfinite(want).all() and (want[0] == 0).all()
    rev, flat = R.spmm(indptr, ids, B, ch, "reversed"), R.spmm(indptr, ids, B, ch, "unchunked")
    n = np.diff(indptr)
    assert (R.bits(rev) != R.bits(want)).any(1)[n >= 63].all()
    # (a chunk of one entry after a full one adds up as the unchunked list does: only a second chunk of several entries shows)
    assert (R.bits(flat) != R.bits(want)).any(1)[n >= 2 * ch].all() and np.array_equal(R.bits(flat)[n <= ch + 1], R.bits(want)[n <= ch + 1])
    dense = np.zeros((n_rows, n_cols))
    dense[np.repeat(np.arange(n_rows), n), ids] = 1
    ones = np.ones((n_cols, 3))
    assert np.array_equal(R.spmm(indptr, ids, ones, ch), dense @ ones)


def test_orth_ratios_are_the_recorded_ones():
    rho, orthogonal = [], []
    for name in PC.ORTH_SHAPES:
        Z = PC.orth_block(name)
        V, S, Rr = R.orth(Z)                               # never meets a failed pivot
        a, b = R.orth_ratios(Z, V, Rr[0])
        rho.append(a)
        orthogonal.append(b)
        assert np.allclose(np.triu(Rr[0]).T @ np.triu(Rr[0]), S[0], rtol=1e-12)
        print("RATIO orth %s cond %.3g rho %.3f orthogonal %.3f" % (name, R.cond2(S[0]), a, b))
    f = PC.fit_ref("random")
    orthogonal.append(float(np.abs(f["Q"].T @ f["Q"] - np.eye(f["Q"].shape[1])).max()) / (R.EPS * f["V"].shape[1]))
    print("RATIO orthogonality of Q, random fit %.3f" % orthogonal[-1])
    assert max(rho) == pytest.approx(R.MEASURED_RHO_ORTH, rel=2e-3) and max(rho) <= R.K / 8
    assert max(orthogonal) == pytest.approx(R.MEASURED_RHO_ORTHOGONAL, rel=2e-3) and max(orthogonal) <= R.K_ORTH / 8
    with pytest.raises(R.PivotError) as e:
        R.orth(PC.repeated_column_block())
    assert (e.value.pass_, e.value.col) == (1, 9)


def test_eig_ratios_are_the_recorded_ones():
    cap = PC.plan()["sweep_cap"]
    rho = []
    inputs = [("%s-%d" % (kind, r), PC.eig_input(kind, r)) for r in PC.EIG_SIZES for kind in ("diagonal", "planted")]
    inputs += [("fit-%s" % w, PC.fit_ref(w)["T"]) for w in ("block", "random")]
    for name, T in inputs:
        lam, Qe, sweeps = R.jacobi(T, cap=cap)             # never reaches the cap
        assert not R.eig_rules(lam, Qe) and sweeps < cap
        rho.append(R.eig_ratio(T, lam, Qe))
        print("RATIO eig %s sweeps %d rho %.3f" % (name, sweeps, rho[-1]))
        if name.startswith("diagonal"):
            assert sweeps == 1 and np.array_equal(lam, np.sort(np.diag(T))[::-1]) and np.array_equal(Qe @ np.diag(lam) @ Qe.T, T)
        else:
            assert np.allclose(lam, np.linalg.eigvalsh(T)[::-1], rtol=0, atol=1e-12 * np.abs(T).max())
    assert max(rho) == pytest.approx(R.MEASURED_RHO_EIG, rel=2e-3) and max(rho) <= R.K_EIG / 8


def test_the_block_fit_is_exact_and_the_random_fit_agrees_with_the_svd():
    f = PC.fit_ref("block")
    rho = PC.block_ratios(f["sigma"], f["Q"], f["P"])
    print("RATIO block fit sigma^2 %.3f Q %.3f P %.3f" % rho)
    assert rho == pytest.approx(R.MEASURED_RHO_BLOCK, rel=2e-3) and all(a <= k / 8 for a, k in zip(rho, R.K_BLOCK))
    sv = np.linalg.svd(PC.dense(PC.block_case()), compute_uv=False)
    assert np.allclose(f["sigma"], sv[:3], rtol=1e-13) and np.allclose(sv[:3] ** 2, [108, 56, 25])
    case = PC.random_case()
    assert np.diff(case["indptr"]).sum() == 900 and case["items"].max() < 90
    f, twin = PC.fit_ref("random"), PC.fit_ref("random", R.LD)
    sv = np.linalg.svd(PC.dense(case), compute_uv=False)[:8]
    assert np.abs(f["sigma"] / sv - 1).max() < 1e-6       # eight iterations at oversample 16: converged to single precision
    rho = float(np.abs(f["sigma"] - twin["sigma"]).max() / twin["sigma"][0]) / R.EPS
    print("RATIO random fit sigma %.3f" % rho)
    assert rho == pytest.approx(R.MEASURED_RHO_SIGMA, rel=2e-3) and rho <= R.K_SIGMA / 8
    res = R.residuals(case["indptr"], case["items"], case["nu"], case["ni"], f["Q"], f["sigma"], PC.plan()["chunk"])
    X = PC.dense(case)
    want = np.linalg.norm(X.T @ (X @ f["Q"]) - f["Q"] * f["sigma"] ** 2, axis=0) / f["sigma"][0] ** 2
    assert np.allclose(res, want, rtol=1e-9, atol=1e-15) and res.max() < 1e-4
    assert (R.residual_bound(case["ni"], res, f["sigma"]) < 1e-14).all()


def test_the_wide_fit_reaches_the_paths_it_is_there_for_and_its_ratio_is_the_recorded_one():
    from tests import ials_ref
    case, fit = PC.wide_case(), PC.WIDE_FIT
    p = puresvd.plan(case["nu"], case["ni"], fit["factors"], fit["oversample"])
    r = p["r"]
    assert r == 101 and r % 2 == 1 and fit["factors"] % 2 == 0                 # k_psvd_spmm at an odd and at an even width
    assert p["lds_bytes"] == r * (r + 1) * 8 + 4096                            # one matrix in LDS: the rotations are in global scratch
    rows = np.diff(case["indptr"])
    cols = np.bincount(case["items"], minlength=case["ni"])
    assert rows[0] > p["chunk"] and cols[0] > p["chunk"] and rows[1] == 0 and cols[1] == 0
    assert rows[2:].max() <= p["chunk"] and cols[2:].max() <= p["chunk"]       # the crowd is added by the row's own wave
    assert all(-(-n // ials_ref.gram_slice_rows(n)) >= 3 for n in (case["nu"], case["ni"])) and p["gram_slices"] >= 3
    f, twin = PC.fit_ref("wide"), PC.fit_ref("wide", R.LD)
    assert 1 <= f["sweeps"] < p["sweep_cap"] and f["sweeps"] == twin["sweeps"]
    sv = np.linalg.svd(PC.dense(case), compute_uv=False)[:fit["factors"]]
    assert np.abs(f["sigma"] / sv - 1).max() < 1e-3        # four iterations on close singular values: the leading digits
    rho = float(np.abs(f["sigma"] - twin["sigma"]).max() / twin["sigma"][0]) / R.EPS
    print("RATIO wide fit sigma %.3f" % rho)
    assert rho == pytest.approx(R.MEASURED_RHO_SIGMA_WIDE, rel=2e-3) and rho <= R.K_SIGMA_WIDE / 8
    orthogonal = float(np.abs(f["Q"].T @ f["Q"] - np.eye(fit["factors"])).max()) / (R.EPS * r)
    assert orthogonal <= R.K_ORTH / 8, orthogonal


def test_arguments_are_checked_before_any_device_work():
    lib = L.load()
    h = L._p()
    for args in ((0, 10, 4, 0), (10, 10, 0, 0), (10, 10, 4, -1), (10, 10, 100, 29)):
        assert lib.tfr_psvd_create(C.byref(h), *args, 0) == L.ERR_ARG and not h
    assert b"r = factors + oversample = 129" in lib.tfr_psvd_last_error()
    assert lib.tfr_psvd_create(None, 10, 10, 4, 0, 0) == L.ERR_ARG
    assert lib.tfr_psvd_destroy(None) == L.OK
    for fn, args in ((lib.tfr_psvd_load, (None, None, None)), (lib.tfr_psvd_fit, (None, None, 1, None)), (lib.tfr_psvd_get, (None, 0, None)),
                     (lib.tfr_psvd_sweeps, (None, None)), (lib.tfr_psvd_set_factors, (None, None, None)), (lib.tfr_psvd_residuals, (None, None)),
                     (lib.tfr_psvd_multiply, (None, 0, None, 1, None)), (lib.tfr_psvd_product_ms, (None, 0, 1, 1, None)), (lib.tfr_psvd_orthonormalise, (None, 1, None, 1, None, None)),
                     (lib.tfr_psvd_eig, (None, None, 1, None, None)), (lib.tfr_psvd_fold_in, (None, 0, None, None, None)),
                     (lib.tfr_psvd_export_f32, (None, 0, 0, 0, None))):
        assert fn(*args) == L.ERR_ARG and b"null" in lib.tfr_psvd_last_error()
