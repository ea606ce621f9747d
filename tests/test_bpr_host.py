"""BPR without a device: the negative sampler's NumPy restatement (tests/bpr_ref.py) and its properties, the float64 step
against central finite differences, and the binding of the tfr_bpr_* symbols."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import bpr_ref as R


def _csr(rows):
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    items = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return indptr, items


def test_mix_restates_splitmix64_finaliser():
    def scalar(z):                                             # the header's definition with Python integers
        M = (1 << 64) - 1
        z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M
        z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    zs = [0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, 123456789]
    assert [int(v) for v in R.mix(np.array(zs, np.uint64))] == [scalar(z) for z in zs]
    assert int(R.step_key(0, 5)) == scalar(scalar(0 ^ 0x9E3779B97F4A7C15) ^ 5)


def test_sampler_never_returns_a_positive():
    rs = np.random.RandomState(0)
    U, I = 50, 40
    rows = [np.sort(rs.choice(I, rs.randint(0, 36), replace=False)) for _ in range(U)]
    indptr, items = _csr(rows)
    users = rs.randint(0, U, 5000)
    for step in (0, 1, 77):
        j = R.sample(indptr, items, users, I, seed=3, step=step, attempts=16)
        for b in np.flatnonzero(j >= 0):
            assert j[b] not in rows[users[b]]
            assert 0 <= j[b] < I


def test_full_row_is_skipped_and_empty_row_takes_attempt_zero():
    I = 30
    indptr, items = _csr([np.arange(I), [], [4, 9]])
    users = np.array([0, 1, 0, 1, 2] * 20)
    j = R.sample(indptr, items, users, I, seed=11, step=4, attempts=64)
    assert np.all(j[users == 0] == -1)                         # every item is a positive of user 0
    c = R.candidates(11, 4, users.size, I, 64)
    assert np.array_equal(j[users == 1], c[users == 1, 0].astype(np.int64))   # nothing to reject: the first draw


def test_sampler_is_uniform_over_the_eligible_items():
    """one seeded case: counts of 20000 draws for a user with 10 of 50 items positive, against a fixed chi-square bound
    (39 degrees of freedom: the 0.999 quantile is 72.1)"""
    I = 50
    pos = np.array([0, 3, 7, 12, 18, 21, 30, 33, 41, 49])
    indptr, items = _csr([pos])
    j = R.sample(indptr, items, np.zeros(20000, np.int64), I, seed=5, step=2, attempts=16)
    assert np.all(j >= 0)
    elig = np.setdiff1d(np.arange(I), pos)
    counts = np.bincount(j, minlength=I)
    assert not counts[pos].any()
    e = j.size / elig.size
    chi2 = float(np.sum((counts[elig] - e) ** 2 / e))
    assert chi2 < 72.1, chi2


def test_steps_and_seeds_draw_differently():
    a = R.candidates(0, 0, 64, 1000, 4)
    assert not np.array_equal(a, R.candidates(0, 1, 64, 1000, 4))
    assert not np.array_equal(a, R.candidates(1, 0, 64, 1000, 4))
    assert np.array_equal(a, R.candidates(0, 0, 64, 1000, 4))


def _problem(seed, U=6, I=8, D=3):
    rs = np.random.RandomState(seed)
    t = {R.MU: np.array(0.3), R.BU: rs.normal(0, .5, U), R.BI: rs.normal(0, .5, I),
         R.PF: rs.normal(0, .5, (U, D)), R.QF: rs.normal(0, .5, (I, D))}
    # repeated users; item 2 is the positive of one triple and the negative of another; an explicit j == i; a skipped one
    u = np.array([0, 0, 1, 1, 2, 3, 3, 4, 5, 0])
    i = np.array([1, 2, 3, 5, 2, 6, 6, 7, 0, 4])
    j = np.array([2, 3, 2, 5, 0, 1, 7, 3, 4, -1])
    return t, u, i, j


@pytest.mark.parametrize("item_abs", [False, True])
@pytest.mark.parametrize("reg_bias", [False, True])
def test_gradients_match_finite_differences(item_abs, reg_bias):
    t, u, i, j = _problem(1 + 2 * item_abs + reg_bias)
    lam, h = 0.07, 1e-6
    G = R.gradients(t, u, i, j, lam, item_abs, reg_bias)
    for k in (R.BI, R.PF, R.QF):
        num = np.zeros_like(t[k])
        for idx in np.ndindex(t[k].shape):
            tp = {kk: v.copy() for kk, v in t.items()}
            tm = {kk: v.copy() for kk, v in t.items()}
            tp[k][idx] += h
            tm[k][idx] -= h
            num[idx] = (R.cost(tp, u, i, j, lam, item_abs, reg_bias) - R.cost(tm, u, i, j, lam, item_abs, reg_bias)) / (2 * h)
        np.testing.assert_allclose(G[k][0], num, rtol=1e-6, atol=1e-7, err_msg="table %d" % k)
        assert not G[k][0][~G[k][1]].any()                   # gradients only on touched rows


def test_skipped_triple_counts_as_absent():
    t, u, i, j = _problem(3)
    lam = 0.05
    keep = j >= 0
    a = R.gradients(t, u, i, j, lam)
    b = R.gradients(t, u[keep], i[keep], j[keep], lam)
    for k in a:
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1])
    assert R.cost(t, u, i, j, lam) == R.cost(t, u[keep], i[keep], j[keep], lam)


def test_bpr_symbols_are_exported_and_bound():
    lib = L.load()
    names = ["tfr_bpr_set_positives", "tfr_bpr_set_sampler", "tfr_bpr_negatives", "tfr_bpr_train_step",
             "tfr_bpr_train_step_dev", "tfr_bpr_train_steps_drawn"]
    for n in names:
        assert hasattr(lib, n), "libtfrecomm_hip.so does not export %s" % n
        assert n in L.SIGNATURES, "binding missing for %s" % n
    for meth in ("set_positives", "set_bpr_sampler", "bpr_negatives", "train_bpr_step", "train_bpr_step_dev",
                 "train_bpr_steps_drawn"):
        assert callable(getattr(T.SvdModel, meth))


def test_gpu_widths_reach_every_register_instantiation():
    """tests/test_gpu_bpr.py WIDTHS reaches every (NJ, last register full) a supported D can reach"""
    from tests import test_gpu_bpr as G
    from tests.test_width_coverage import SUPPORTED
    reach = {G.registers(D) for D in SUPPORTED}
    assert {G.registers(D) for D in G.WIDTHS} == reach and 1 in G.WIDTHS
