"""PureSVD on the device (tfr_psvd_* through tfrecomm_amd.PureSVD), one stage per test from given inputs, on the cases of
tests/puresvd_cases.py against tests/puresvd_ref.py: the product kernel bit for bit in both orientations, the
orthonormalisation, the eigen step, a planted fit with an exact answer, a random fit, fold-in and serving, and the state a
handle keeps between calls.  The constants are tests/puresvd_ref.py's, measured on the CPU by tests/test_puresvd_host.py.

MEASURED on an MI355X (the RATIO lines, run with -s; DESIGN §37 has the table): orth 1.317 of K 11, orthogonality 1.458 of
K_ORTH 12, eigen step 1.536 of K_EIG 11 (T of the random fit; the planted inputs over tests/list_paths.py PSVD_EIG_SIZES give
0.600 at r = 4, 1.313 at 37, 1.023 at 99, 1.071 at 100, 1.056 at 101, 1.161 at 127, 1.125 at 128, in at most 11 sweeps), block
fit 1.788 / 0.965 / 0.966 of K_BLOCK 39 / 9 / 16, random fit sigma 1.070 of K_SIGMA 42, wide fit (r = 101, 9 sweeps) sigma
3.190 of K_SIGMA_WIDE 256 and orthogonality 1.000 of K_ORTH 12."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import ials_ref
from tests import puresvd_cases as PC
from tests import puresvd_ref as R

pytestmark = pytest.mark.gpu

bits = R.bits


def _open(case, fit, load=True):
    m = T.PureSVD(case["nu"], case["ni"], **fit)
    if load:
        m.load((case["indptr"], case["items"]))
    return m


def _fitted(which):
    case, fit = {"block": (PC.block_case(), PC.BLOCK_FIT), "random": (PC.random_case(), PC.RANDOM_FIT),
                 "wide": (PC.wide_case(), PC.WIDE_FIT)}[which]
    m = _open(case, fit)
    m.fit(start=PC.start_block(case, fit))
    return m, case, fit


def _state_error(call, text):
    with pytest.raises(T.TfrError) as e:
        call()
    assert e.value.code == L.ERR_STATE and text in str(e.value), str(e.value)


# ----------------------------------------------------------------------------- 1. the product, bit for bit
@pytest.mark.parametrize("transpose", [False, True], ids=["rows", "lists"])
def test_the_product_is_the_restated_sum_bit_for_bit(transpose):
    """the same lists as the users' rows of one matrix (X in) and as the items' lists of its transpose (X^T in)"""
    indptr, ids, n_rows, n_cols = PC.product_lists()
    ch = PC.plan()["chunk"]
    csr, nu, ni = PC.as_matrix(indptr, ids, n_rows, n_cols, transpose)
    with T.PureSVD(nu, ni, factors=4, oversample=0) as m:
        m.load(csr)
        for r in PC.product_widths():
            B = PC.product_block(n_cols, r)
            want = R.spmm(indptr, ids, B, ch)
            got = m.multiply(B, transpose=transpose)
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (transpose, r)
            assert (got[0] == 0).all() and not np.signbit(got[0]).any()           # the empty row
        again = m.multiply(B, transpose=transpose)
        assert np.array_equal(bits(again), bits(got))                              # a repeat
    # a row alone: every long row as the only row of its own matrix gives the bits it has in the crowd
    for e in np.flatnonzero(np.diff(indptr) >= ch - 1):
        alone = (np.array([0, indptr[e + 1] - indptr[e]], np.int64), ids[indptr[e]:indptr[e + 1]])
        csr1, nu1, ni1 = PC.as_matrix(alone[0], alone[1], 1, n_cols, transpose)
        with T.PureSVD(nu1, ni1, factors=4, oversample=0) as m1:
            m1.load(csr1)
            assert np.array_equal(bits(m1.multiply(B, transpose=transpose)[0]), bits(want[e])), (transpose, int(e))


# ----------------------------------------------------------------------------- 2. orthonormalise
@pytest.mark.parametrize("name", sorted(PC.ORTH_SHAPES))
def test_orthonormalise_against_the_long_double_restatement(name):
    Z = PC.orth_block(name)
    n, r = Z.shape
    with T.PureSVD(4, 4, factors=2, oversample=0) as m:
        V, S, Rd = m.orthonormalise(Z)
    # the first pass's S: the block holds float32 values, so the Gram's fused products are exact and the ALS restatement's
    # rounded ones are the same numbers (the second pass's block is full precision and never leaves the device)
    assert np.array_equal(bits(S[0]), bits(ials_ref.gram_f64(Z))), name
    assert np.array_equal(S[0], S[0].T) and np.array_equal(S[1], S[1].T)
    assert (np.tril(Rd, -1) == 0).all() and (np.diagonal(Rd, axis1=1, axis2=2) > 0).all()
    # each pass's factor against that pass's own S: the backward error of a Cholesky factorisation in any order, with or
    # without fused products, |R^T R - S| <= gamma_{r+1} |R|^T |R| (Higham, Accuracy and Stability, theorem 10.3)
    gamma = (r + 1) * R.EPS / (1 - (r + 1) * R.EPS)
    for p in range(2):
        Rl = Rd[p].astype(R.LD)
        assert (np.abs(Rl.T @ Rl - S[p].astype(R.LD)) <= gamma * (np.abs(Rl).T @ np.abs(Rl))).all(), (name, p)
    rho, orthogonal = R.orth_ratios(Z, V, Rd[0])
    print("RATIO orth %s [%d, %d] device rho %.3f (K %d) orthogonal %.3f (K_ORTH %d)" % (name, n, r, rho, R.K, orthogonal, R.K_ORTH))
    assert rho <= R.K and orthogonal <= R.K_ORTH, (name, rho, orthogonal)


def test_a_block_with_a_repeated_column_is_refused_and_the_fit_is_forgotten():
    with T.PureSVD(4, 4, factors=2, oversample=0) as m:
        with pytest.raises(T.TfrError) as e:
            m.orthonormalise(PC.repeated_column_block())
        assert e.value.code == L.ERR_ARG and "orthonormalisation 0, pass 1: the pivot of column 9 is not positive and finite" in str(e.value)
    m, case, fit = _fitted("random")
    with m:
        V0 = PC.start_block(case, fit).copy()
        V0[:, 5] = V0[:, 2]
        with pytest.raises(T.TfrError) as e:
            m.fit(start=V0)
        assert e.value.code == L.ERR_ARG and "fit: orthonormalisation 0, pass 1: the pivot of column 5" in str(e.value)
        _state_error(lambda: m.singular_values, "no factors")                      # loaded, not fitted
        m.fit(start=PC.start_block(case, fit))                                     # and still usable
        assert np.array_equal(bits(m.singular_values), bits(_fitted_sigma()))


def _fitted_sigma():
    m, _, _ = _fitted("random")
    with m:
        return m.singular_values


# ----------------------------------------------------------------------------- 3. the eigen step
def _eig_inputs():
    out = [("%s-%d" % (kind, r), kind, r) for r in PC.EIG_SIZES for kind in ("diagonal", "planted")]
    return out + [("fit-random", "fit", 24)]


@pytest.mark.parametrize("name,kind,r", _eig_inputs(), ids=[x[0] for x in _eig_inputs()])
def test_the_eigen_step(name, kind, r):
    T_ = PC.fit_ref("random")["T"] if kind == "fit" else PC.eig_input(kind, r)
    cap = PC.plan()["sweep_cap"]
    with T.PureSVD(4, 4, factors=2, oversample=0) as m:
        lam, Qe = m.eig(T_)
        sweeps = m.sweeps()
        lam2, Qe2 = m.eig(T_)
        assert np.array_equal(bits(lam), bits(lam2)) and np.array_equal(bits(Qe), bits(Qe2))
        bad = np.array(T_)
        if r > 1:
            bad[0, 1] += 1.0
            with pytest.raises(T.TfrError) as e:
                m.eig(bad)
            assert e.value.code == L.ERR_ARG and "differ" in str(e.value)
    assert not R.eig_rules(lam, Qe) and 1 <= sweeps < cap, (name, sweeps)
    if kind == "diagonal":                                 # an exact permutation, no rotation
        assert sweeps == 1 and np.array_equal(lam, np.sort(np.diag(T_))[::-1])
        assert ((Qe == 0) | (Qe == 1)).all() and np.array_equal(Qe @ np.diag(lam) @ Qe.T, T_)
    rho = R.eig_ratio(T_, lam, Qe)
    print("RATIO eig %s device sweeps %d rho %.3f (K_EIG %d)" % (name, sweeps, rho, R.K_EIG))
    assert rho <= R.K_EIG, (name, rho)


# ----------------------------------------------------------------------------- 4. a planted fit with an exact answer
def test_the_block_fit_gives_the_exact_factors():
    m, case, fit = _fitted("block")
    with m:
        sigma, Q, P, ritz = m.singular_values, m.item_factors, m.user_factors, m.ritz_values
        assert 1 <= m.sweeps() < PC.plan()["sweep_cap"] and len(m.fit_ms_parts) == 3 and m.fit_ms > 0
    rho = PC.block_ratios(sigma, Q, P)
    print("RATIO block fit device sigma^2 %.3f Q %.3f P %.3f (K_BLOCK %s)" % (rho + (R.K_BLOCK,)))
    assert all(a <= k for a, k in zip(rho, R.K_BLOCK)), rho
    assert np.array_equal(bits(sigma), bits(np.sqrt(np.maximum(ritz[:3], 0)))) and ritz.shape == (5,) and (np.diff(ritz) <= 0).all()
    assert np.array_equal(bits(P), bits(R.spmm(case["indptr"], case["items"], Q, PC.plan()["chunk"])))


# ----------------------------------------------------------------------------- 5. a random fit
def test_the_random_fit():
    m, case, fit = _fitted("random")
    ref = PC.fit_ref("random")
    ch = PC.plan()["chunk"]
    with m:
        sigma, Q, P, res = m.singular_values, m.item_factors, m.user_factors, m.residuals()
    rho = float(np.abs(sigma - ref["sigma"]).max() / ref["sigma"][0]) / R.EPS
    orthogonal = float(np.abs(Q.T @ Q - np.eye(fit["factors"])).max()) / (R.EPS * (fit["factors"] + fit["oversample"]))
    print("RATIO random fit device sigma %.3f (K_SIGMA %d) orthogonal %.3f (K_ORTH %d)" % (rho, R.K_SIGMA, orthogonal, R.K_ORTH))
    assert rho <= R.K_SIGMA and orthogonal <= R.K_ORTH, (rho, orthogonal)
    assert np.array_equal(bits(P), bits(R.spmm(case["indptr"], case["items"], Q, ch)))
    want = R.residuals(case["indptr"], case["items"], case["nu"], case["ni"], Q, sigma, ch)
    assert (np.abs(res - want) <= R.residual_bound(case["ni"], want, sigma)).all(), (res, want)


# ----------------------------------------------------------------------------- 5b. a wide fit, and fold-ins of long lists
def _lists_of(rs, n_items, lengths):
    rows = [np.sort(rs.choice(n_items, n, replace=False)).astype(np.int32) for n in lengths]
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64), np.concatenate(rows).astype(np.int32)


def test_the_wide_fit_and_long_fold_ins():
    """300 x 280, r = 101 (tests/puresvd_cases.py wide_case): inside a fit the product runs at an odd width with both
    orientations' longest list cut into chunks, every Gram takes three slices, the eigen step keeps its rotations in global
    scratch with index r sitting out.  Then fold-ins whose lists need a chunk plan of their own, which must leave the model's
    chunk tables as they were."""
    m, case, fit = _fitted("wide")
    ref = PC.fit_ref("wide")
    indptr, items, nu, ni, f = case["indptr"], case["items"], case["nu"], case["ni"], fit["factors"]
    ch, cap = PC.plan()["chunk"], PC.plan()["sweep_cap"]
    assert np.diff(indptr)[0] > ch
    with m:
        sigma, Q, P, sweeps = m.singular_values, m.item_factors, m.user_factors, m.sweeps()
        assert np.array_equal(bits(P), bits(R.spmm(indptr, items, Q, ch)))
        assert 1 <= sweeps < cap, sweeps
        rho = float(np.abs(sigma - ref["sigma"]).max() / ref["sigma"][0]) / R.EPS
        orthogonal = float(np.abs(Q.T @ Q - np.eye(f)).max()) / (R.EPS * (f + fit["oversample"]))
        print("RATIO wide fit device sweeps %d sigma %.3f (K_SIGMA_WIDE %d) orthogonal %.3f (K_ORTH %d)" % (
            sweeps, rho, R.K_SIGMA_WIDE, orthogonal, R.K_ORTH))
        assert rho <= R.K_SIGMA_WIDE and orthogonal <= R.K_ORTH, (rho, orthogonal)
        m.fit(start=PC.start_block(case, fit))
        again = (m.singular_values, m.item_factors, m.user_factors)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((sigma, Q, P), again))   # two fits: the same bits

        rs = np.random.RandomState(12)
        B = [PC.product_block(ni, 7), PC.product_block(nu, 7)]
        before = [m.multiply(B[0]), m.multiply(B[1], transpose=True)]
        tptr, tids = R.transpose_lists(indptr, items, nu, ni)
        assert np.array_equal(bits(before[0]), bits(R.spmm(indptr, items, B[0], ch)))
        assert np.array_equal(bits(before[1]), bits(R.spmm(tptr, tids, B[1], ch)))
        # a list is strictly increasing, so 280 items hold none of 2 chunk + 1 entries: here the longest is every item (a
        # second chunk of several entries), and the three-chunk list is folded in on a wider catalogue below
        lengths = [ch - 1, ch, ch + 1, ni, 0]
        lists = _lists_of(rs, ni, lengths)
        got = m.fold_in_users(lists)
        assert np.array_equal(bits(got), bits(R.spmm(lists[0], lists[1], Q, ch))), "fold-in of long lists"
        assert (got[4] == 0).all() and not np.signbit(got[4]).any()
        assert np.array_equal(bits(m.fold_in_users((indptr, items))), bits(P)), "fold-in of the resident lists"
        m.fold_in_users(lists)                                                     # the last plan standing is not the model's
        after = [m.multiply(B[0]), m.multiply(B[1], transpose=True)]
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after)), "multiply after the fold-ins"
        assert np.array_equal(bits(m.user_factors), bits(P))
    # 2 chunk + 1 entries need a catalogue that long: factors set on 2 chunk + 40 items, resident rows of their own, one of
    # them long; an even and an odd width
    ni2 = 2 * ch + 40
    lengths = [ch - 1, ch, ch + 1, 2 * ch + 1, 0]
    lists = _lists_of(rs, ni2, lengths)
    own = _lists_of(rs, ni2, [3, ch + 5, 0, 9])
    for f2 in (8, 7):
        Q2 = PC.product_block(ni2, f2)
        with T.PureSVD(4, ni2, factors=f2, oversample=0) as m2:
            m2.load(own)
            m2.set_factors(Q2, np.ones(f2))
            P2 = m2.user_factors
            assert np.array_equal(bits(P2), bits(R.spmm(own[0], own[1], Q2, ch)))
            got = m2.fold_in_users(lists)
            assert np.array_equal(bits(got), bits(R.spmm(lists[0], lists[1], Q2, ch))), "fold-in of a three-chunk list, width %d" % f2
            assert np.array_equal(bits(m2.fold_in_users(own)), bits(P2))
            m2.fold_in_users(lists)
            assert np.array_equal(bits(m2.multiply(Q2)), bits(P2)), "multiply after the fold-ins, width %d" % f2


# ----------------------------------------------------------------------------- 6. fold-in and serving
def test_fold_in_and_serving():
    m, case, fit = _fitted("random")
    indptr, items, nu, ni, f = case["indptr"], case["items"], case["nu"], case["ni"], fit["factors"]
    with m:
        Q, P = m.item_factors, m.user_factors
        rows = m.fold_in_users((indptr, items))                                    # the resident lists
        assert np.array_equal(bits(rows), bits(P))
        lists = (np.array([0, 0, 3, 3, 7], np.int64), np.array([1, 5, 80, 0, 2, 40, 89], np.int32))
        got = m.fold_in_users(lists)
        assert np.array_equal(bits(got), bits(R.spmm(lists[0], lists[1], Q, PC.plan()["chunk"]))) and (got[0] == 0).all() and (got[2] == 0).all()
        with pytest.raises(L.OutOfRangeError) as e:
            m.fold_in_users((np.array([0, 2], np.int64), np.array([1, ni], np.int32)))
        assert "fold_in: list row 0: id %d out of range" % ni in str(e.value)
        with pytest.raises(T.TfrError) as e:
            m.fold_in_users((np.array([0, 2], np.int64), np.array([5, 1], np.int32)))
        assert e.value.code == L.ERR_ARG and "fold_in: list row 0 is not strictly increasing" in str(e.value)

        with m.to_svd_model() as plain:
            tabs = plain.tables()
            assert tabs[L.P].tobytes() == P.astype(np.float32).tobytes() and tabs[L.Q].tobytes() == Q.astype(np.float32).tobytes()
            assert tabs[L.MU] == 0 and not tabs[L.BU].any() and not tabs[L.BI].any()
            with pytest.raises(ValueError):
                m.recommend_lists(plain, lists)
            held = (np.arange(nu, dtype=np.int32), (np.arange(nu) * 7 % ni).astype(np.int32))
            out = T.evaluate_ranking(plain, held[0], held[1], ks=(5,))
            assert out["ranks"].size == nu and (out["ranks"] >= 0).all()
        n = lists[0].size - 1
        with T.SvdModel(n, ni, f) as host:
            host.set_tables(np.float32(0.0), np.zeros(n, np.float32), np.zeros(ni, np.float32), got.astype(np.float32), Q.astype(np.float32))
            want = {ex: host.recommend(np.arange(n, dtype=np.int32), 6, exclude=lists if ex else None) for ex in (True, None)}
        with m.to_svd_model(extra_users=3) as svd:                                 # more lists than guest rows
            for ex, (wi, ws) in want.items():
                gi, gs = m.recommend_lists(svd, lists, k=6, exclude=ex)
                assert gi.tobytes() == wi.tobytes() and gs.tobytes() == ws.tobytes(), ex
                if ex:
                    assert not set(gi[1]) & {1, 5, 80}


def test_product_ms_times_the_kernel_alone():
    case, fit = PC.random_case(), PC.RANDOM_FIT
    with _open(case, fit, load=False) as m:
        _state_error(lambda: m.product_ms(24), "product_ms: no data: call tfr_psvd_load first")
        m.load((case["indptr"], case["items"]))
        for transpose in (False, True):
            for cols in (1, 24, 128):
                ms = m.product_ms(cols, transpose, reps=3)
                assert len(ms) == 3 and all(0 < t < 1000 for t in ms), (transpose, cols, ms)
        for bad in (dict(cols=0), dict(cols=129), dict(cols=8, reps=0)):
            with pytest.raises(T.TfrError) as e:
                m.product_ms(**bad)
            assert e.value.code == L.ERR_ARG


# ----------------------------------------------------------------------------- 7. state
def test_the_state_between_calls():
    case, fit = PC.random_case(), PC.RANDOM_FIT
    V0 = PC.start_block(case, fit)
    with _open(case, fit, load=False) as m:
        _state_error(lambda: m.fit(start=V0), "fit: no data: call tfr_psvd_load first")
        _state_error(lambda: m.multiply(V0), "multiply: no data")
        m.load((case["indptr"], case["items"]))
        _state_error(lambda: m.item_factors, "get: no factors: call tfr_psvd_fit or tfr_psvd_set_factors first")
        _state_error(lambda: m.residuals(), "residuals: no factors")
        _state_error(lambda: m.fold_in_users((np.array([0, 1], np.int64), np.array([1], np.int32))), "fold_in: no factors")
        m.fit(start=V0)
        first = (m.singular_values, m.item_factors, m.user_factors, m.ritz_values)
        m.fit(start=V0)
        again = (m.singular_values, m.item_factors, m.user_factors, m.ritz_values)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again))      # two fits: the same bits
        # rows folded in belong to the factors they came from: a refit and set_factors forget them
        lists = (np.array([0, 2], np.int64), np.array([1, 5], np.int32))
        export_fold = lambda h: h._lib.tfr_psvd_export_f32(h._h, 2, 0, 1, None)
        m.fold_in_users(lists)
        assert export_fold(m) == L.ERR_ARG and b"null destination" in m._lib.tfr_psvd_last_error()      # the rows are there
        m.fit(start=V0)
        assert export_fold(m) == L.ERR_STATE and b"no fold-in rows" in m._lib.tfr_psvd_last_error()
        m.fold_in_users(lists)
        m.set_factors(first[1], first[0])
        assert export_fold(m) == L.ERR_STATE
        # a refused load leaves the factors as they were
        with pytest.raises(L.OutOfRangeError):
            m.load((case["indptr"], np.where(np.arange(case["items"].size) == 3, case["ni"], case["items"]).astype(np.int32)))
        assert np.array_equal(bits(m.item_factors), bits(first[1])) and np.array_equal(bits(m.user_factors), bits(first[2]))
        # set_factors(get...) round-trips
        with _open(case, fit) as other:
            other.set_factors(first[1], first[0])
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first[:3], (other.singular_values, other.item_factors, other.user_factors)))
            _state_error(lambda: other.ritz_values, "no Ritz values")
            assert np.array_equal(bits(other.residuals()), bits(m.residuals()))
        # a second load forgets the fit
        m.load((case["indptr"], case["items"]))
        _state_error(lambda: m.singular_values, "no factors")
        m.fit(start=V0)
        assert np.array_equal(bits(m.item_factors), bits(first[1]))
