"""The conjugate-gradient implicit ALS on the device (csrc/ials_cg.hip through ImplicitALS(solver="cg")) against the
restatements of tests/ials_cg_ref.py on the cases of tests/ials_cg_cases.py.  The Gram, which both solvers share, is held per
entry to its derived bound and to bitwise symmetry, and to the same bytes from a handle of either solver; each half to the
longdouble iterate at the same step count, fed the tables the device read and the device's own Gram; the converged run to the exact minimiser and to the Cholesky path; then what must hold bit for
bit, the trajectory, the wide loss, planted blocks end to end at 128 factors, and the refusals."""
import ctypes as C_
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import ials_cases as C0
from tests import ials_cg_cases as C
from tests import ials_cg_ref as G
from tests import ials_ref as R

pytestmark = pytest.mark.gpu

BY_ID = {c["id"]: c for c in C.CASES + C.CONV_CASES}


def _open(case, steps, load=True, **kw):
    m = T.ImplicitALS(case["nu"], case["ni"], factors=case["d"], regularization=case["lam"], alpha=case["alpha"], solver="cg",
                      cg_steps=steps, **kw)
    m.set_factors(case["X"], case["Y"])
    if load:
        m.load(C0.csr(case))
    return m


def _both(m):
    return m.user_factors, m.item_factors


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _gram_ld(tab):
    t = tab.astype(R.LD)
    return t.T @ t


def _check_halves(case, steps_list=C.STEPS, sides=(0, 1)):
    """each half of ``sides`` at each step count, from the case's own tables: held to the longdouble iterate at the same
    steps, fed those tables and the device's own Gram of them.  cond2(A) is computed once per half.  Returns the worst ratio."""
    lst = R.lists(case, 0), R.lists(case, 1)
    tabs = [case["X"], case["Y"]]
    bad, worst, cond, grams = [], 0.0, {}, {}
    for steps in steps_list:
        with _open(case, steps) as m:
            for side in sides:
                own, other = tabs[side], tabs[1 - side]
                m.set_factors(case["X"], case["Y"])
                Gd = m.gram(1 - side)
                if side not in grams:
                    grams[side] = Gd
                    assert Gd.tobytes() == Gd.T.copy().tobytes(), "%s: the Gram is not bitwise symmetric" % case["id"]
                    err = np.abs(Gd.astype(R.LD) - _gram_ld(other)).astype(np.float64)
                    if not (err <= R.gram_bound(other)).all():
                        bad.append("%s: the Gram of side %d is outside (n + 2) eps |T|^T |T| by %.3g"
                                   % (case["id"], 1 - side, (err / R.gram_bound(other)).max()))
                    cond[side] = G.conds(other, lst[side], case["lam"], case["alpha"], Gd)
                assert Gd.tobytes() == grams[side].tobytes()
                m.half_sweep(side)
                got = m.user_factors if side == 0 else m.item_factors
                untouched = m.item_factors if side == 0 else m.user_factors
                what = "%s, %s half, %d steps" % (case["id"], ("user", "item")[side], steps)
                assert untouched.tobytes() == other.tobytes(), "%s wrote the other table" % what
                assert np.isfinite(got).all(), "%s: NaN or Inf" % what
                ref = G.cg_half(own, other, lst[side], case["lam"], case["alpha"], steps, G=Gd, cond=cond[side])
                bad += R.check_half(ref, got, G.K_CG, what)
                worst = max(worst, float(R.ratios(ref, got).max()))
    print("RATIO %s %.3f of K_CG = %d" % (case["id"], worst, G.K_CG))
    assert not bad, "\n".join(bad)
    return worst


# ----------------------------------------------------------------------------- Gram
@pytest.mark.parametrize("d", C.GRAM_WIDTHS)
def test_wide_gram_per_entry_and_bitwise_symmetric(d):
    for n in C.GRAM_NS + ((131073,) if d == 65 else ()):
        rs = np.random.RandomState(1000 * d + n % 1000)
        X, Y = rs.uniform(-1.0, 1.0, (n, d)), rs.uniform(-1.0, 1.0, (3, d))
        with T.ImplicitALS(n, 3, factors=d, solver="cg") as m:
            m.set_factors(X, Y)
            Gu, Gi, again = m.gram(0), m.gram(1), m.gram(0)
        assert Gu.tobytes() == again.tobytes(), (n, d)
        for got, tab in ((Gu, X), (Gi, Y)):
            assert got.tobytes() == got.T.copy().tobytes(), "n = %d, d = %d: not bitwise symmetric" % (n, d)
            err = np.abs(got.astype(R.LD) - _gram_ld(tab)).astype(np.float64)
            assert (err <= R.gram_bound(tab)).all(), (n, d, float((err / R.gram_bound(tab)).max()))


def test_both_solvers_return_the_same_gram_bytes():
    """one Gram for both paths: at d = 1, 5, 33 and 64 a Cholesky handle and a conjugate-gradient handle give the same bytes,
    on either side"""
    for d in (1, 5, 33, 64):
        rs = np.random.RandomState(9 + d)
        X, Y = rs.uniform(-1.0, 1.0, (643, d)), rs.uniform(-1.0, 1.0, (3, d))
        out = []
        for kw in (dict(), dict(solver="cg")):
            with T.ImplicitALS(643, 3, factors=d, **kw) as m:
                m.set_factors(X, Y)
                out.append((m.gram(0), m.gram(1)))
        assert _same(out[0], out[1]), d


# ----------------------------------------------------------------------------- half-sweeps per entity
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_each_half_follows_the_longdouble_iterate_at_the_same_steps(case):
    _check_halves(case)


@functools.lru_cache(maxsize=None)
def _grid():
    return C0.grid_entities()


def _alone(case, u):
    """the case with only user u's row"""
    keep = np.zeros(case["nu"], bool)
    keep[u] = True
    x = C0.csr(case).multiply(keep[:, None]).tocsr()
    x.eliminate_zeros()
    x.sort_indices()
    return dict(case, indptr=x.indptr.astype(np.int64), items=x.indices.astype(np.int32), vals=np.ascontiguousarray(x.data, np.float64))


def _check_alone(case, steps, X, users):
    for u in users:
        with _open(_alone(case, u), steps) as m:
            m.half_sweep(0)
            assert m.user_factors[u].tobytes() == X[u].tobytes(), "%s: user %d alone differs from itself in the crowd" % (case["id"], u)


@pytest.mark.parametrize("swap", [False, True], ids=["as-given", "swapped"])
def test_more_entities_than_the_grid(swap):
    """70 000 entities on one side, every tenth of them empty: k_ials_cg_fit's blocks each take a second one"""
    case = C0.swapped(_grid()) if swap else _grid()
    assert max(case["nu"], case["ni"]) > 65535
    _check_halves(case, steps_list=(3,))
    if not swap:
        with _open(case, 3) as m:
            m.half_sweep(0)
            X = m.user_factors
        _check_alone(case, 3, X, [5, 5 + 65535 + 1])       # user 65 541 is its block's second entity (65 540 is empty)


# ----------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("case", C.CONDITIONING, ids=lambda c: c["id"])
def test_few_pairs_at_256_components(case):
    """1, 5 and 40 pairs against 256 components, lambda down to 1e-6: the bound carries cond2(A); nothing is NaN or Inf"""
    for c in (case, C.normal(case)):
        _check_halves(c, steps_list=(3,))


# ----------------------------------------------------------------------------- convergence
@pytest.mark.parametrize("case", [c for c in C.CONV_CASES if c["d"] in (9, 33)], ids=lambda c: c["id"])
def test_three_d_steps_reach_the_exact_minimiser_and_the_cholesky_path(case):
    lst = R.lists(case, 0), R.lists(case, 1)
    with _open(case, 3 * case["d"]) as m, T.ImplicitALS(case["nu"], case["ni"], factors=case["d"], regularization=case["lam"],
                                                         alpha=case["alpha"]) as ch:
        ch.set_factors(case["X"], case["Y"])
        ch.load(C0.csr(case))
        for side in (0, 1):
            own, other = (case["X"], case["Y"]) if side == 0 else (case["Y"], case["X"])
            m.set_factors(case["X"], case["Y"])
            ch.set_factors(case["X"], case["Y"])
            Gd = m.gram(1 - side)
            m.half_sweep(side)
            ch.half_sweep(side)
            got, chol = (m.user_factors, ch.user_factors) if side == 0 else (m.item_factors, ch.item_factors)
            exact = R.half(other, lst[side], case["lam"], case["alpha"], G=Gd)
            ref = G.against_exact(own, exact)
            what = "%s, side %d" % (case["id"], side)
            print("CONV %s: %.3f of K_CONV = %d" % (what, float(R.ratios(ref, got).max()), G.K_CONV))
            assert not R.check_half(ref, got, G.K_CONV, what)
            # the Cholesky path read its own Gram: its statement is K eps cond |x*|; the margin is the sum of the two bounds
            tol = R.EPS * exact["cond"] * (G.K_CONV * ref["xmax"] + R.K * exact["xmax"])
            err = np.abs(got - chol).max(1)
            assert (err <= tol).all(), (what, float((err / np.maximum(tol, 1e-300)).max()))
            assert (got[exact["N"] == 0] == 0).all() and (chol[exact["N"] == 0] == 0).all()


# ----------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("cid", ["cg-widths-d65", "cg-widths-d129-swapped-normal", "cg-long-d256"])
def test_three_sweeps_in_one_call_equal_three_calls_and_six_halves(cid):
    case = BY_ID[cid]
    with _open(case, 3) as m:
        m.sweep(3)
        once = _both(m)
        m.set_factors(case["X"], case["Y"])
        m.sweep(3)
        assert _same(once, _both(m)), "a repeat differs"
        m.set_factors(case["X"], case["Y"])
        for _ in range(3):
            m.sweep(1)
        assert _same(once, _both(m))
        m.set_factors(case["X"], case["Y"])
        for _ in range(3):
            m.half_sweep(0)
            m.half_sweep(1)
        assert _same(once, _both(m))
        assert not _same(once, (case["X"], case["Y"]))


@pytest.mark.parametrize("cid,users", [("cg-widths-d65", (1, 4, 8, 14)), ("cg-long-d256", (0, 2, 5)), ("cg-widths-d192-normal", (3, 9))])
def test_an_entity_alone_equals_itself_in_the_crowd(cid, users):
    case = BY_ID[cid]
    with _open(case, 3) as m:
        m.half_sweep(0)
        X = m.user_factors
    _check_alone(case, 3, X, users)


def test_a_second_load_replaces_the_first():
    first = BY_ID["cg-widths-d65"]
    rs = np.random.RandomState(77)
    nu, ni, d = first["nu"], first["ni"], 65
    X, Y = rs.rand(nu, d), rs.rand(ni, d)
    a = sp.random(nu, ni, 0.05, random_state=rs, data_rvs=lambda n: rs.randint(1, 5, n).astype(np.float64)).tocsr()
    with T.ImplicitALS(nu, ni, factors=d, regularization=0.1, alpha=40.0, solver="cg", cg_steps=3) as m:
        m.set_factors(X, Y)
        m.load(a)
        m.sweep(1)
        fresh = _both(m)
        m.set_factors(X, Y)
        m.load(C0.csr(first))
        m.sweep(1)
        moved = _both(m)
        m.set_factors(X, Y)
        m.load(a)                                          # fewer pairs: as if the first load had never been
        m.sweep(1)
        assert not _same(moved, fresh) and _same(_both(m), fresh)


def test_the_chunk_size_is_validated_and_ignored():
    case = BY_ID["cg-long-d65"]
    got = []
    for chunk in (32, 512):
        with _open(case, 3, chunk=chunk) as m:
            m.sweep(1)
            got.append(_both(m))
    assert _same(*got)
    with pytest.raises(T.TfrError):
        _open(case, 3, chunk=48)


# ----------------------------------------------------------------------------- trajectory
def test_ten_iterations_follow_the_float64_restatement_and_the_loss_never_rises():
    case = C0.trajectory()
    with T.ImplicitALS(case["nu"], case["ni"], factors=8, regularization=0.1, alpha=40.0, iterations=10, solver="cg", cg_steps=3) as m:
        m.fit(C0.csr(case), seed=0)
        X, Y = _both(m)
        assert m.sweep_ms > 0
        m.set_factors(case["X"], case["Y"])
        last = m.loss()
        for half in range(20):
            m.half_sweep(half % 2)
            now = m.loss()
            assert now <= last + G.K_LOSS_WIDE * R.EPS * R.loss_terms(*_both(m), case), (half, last, now)
            last = now
        assert _same((X, Y), _both(m))
    wx, wy = G.sweep_f64(case, case["X"], case["Y"], 3, 10)
    for name, got, want in (("X", X, wx), ("Y", Y, wy)):
        err = np.abs(got - want).max() / np.abs(want).max()
        print("TRAJECTORY %s: %.3e of the table scale %.3g" % (name, err, np.abs(want).max()))
        assert err <= 1e-9, "%s: %.3e" % (name, err)


# ----------------------------------------------------------------------------- loss
@pytest.mark.parametrize("cid", [i for i in C.LOSS_IDS if BY_ID[i]["d"] > 64])
def test_wide_loss_against_the_longdouble_formula(cid):
    case = BY_ID[cid]
    assert case["d"] in (65, 128, 256)
    with _open(case, 3) as m:
        X, Y = case["X"], case["Y"]
        for step in range(3):
            got = m.loss()
            want, terms = R.loss(X, Y, case), R.loss_terms(X, Y, case)
            err = float(abs(R.LD(got) - want))
            print("LOSS %s step %d: %.17g, error %.3g of the bound" % (cid, step, got, err / (G.K_LOSS_WIDE * R.EPS * terms)))
            assert err <= G.K_LOSS_WIDE * R.EPS * terms, (cid, step, got, float(want))
            m.half_sweep(step % 2)
            X, Y = _both(m)


# ----------------------------------------------------------------------------- end to end
def test_planted_blocks_are_recovered_at_128_factors():
    """the data of test_gpu_ials.test_planted_blocks_are_recovered: 200 users in 4 groups, 120 items in 4 blocks, one in-block
    item held out per user.  lambda = 10: at 0.01 the wide model overfits 200 users."""
    rs = np.random.RandomState(3)
    U, I = 200, 120
    tu, ti, hu, hi = [], [], [], []
    for u in range(U):
        g = u % 4
        own = g * 30 + rs.choice(30, 12, replace=False)
        rest = np.setdiff1d(np.arange(I), own)
        held, kept = own[0], own[1:]
        items = np.concatenate((kept, rs.choice(np.setdiff1d(rest, [held]), 2, replace=False)))
        tu += [u] * items.size; ti += list(items); hu.append(u); hi.append(held)
    tu, ti, hu, hi = (np.asarray(a, np.int32) for a in (tu, ti, hu, hi))
    train = T.rated_matrix(tu, ti, U, I)
    with T.ImplicitALS(U, I, factors=128, solver="cg", cg_steps=3, regularization=10.0, alpha=40.0, iterations=10) as m:
        m.fit(train, seed=0)
        with m.to_svd_model() as svd:
            res = T.evaluate_ranking(svd, hu, hi, exclude=train, ks=(10,))
    pop = np.bincount(ti, minlength=I).astype(np.float64)
    hits = 0
    for u, t in zip(hu, hi):
        s = pop.copy()
        s[train.indices[train.indptr[u]:train.indptr[u + 1]]] = -np.inf
        order = np.lexsort((np.arange(I), -s))[:10]
        hits += int(t in order)
    recall, recall_pop = res["mean"]["recall@10"], hits / float(U)
    print("planted blocks at 128 factors: recall@10 CG iALS %.3f, popularity %.3f" % (recall, recall_pop))
    assert recall >= 2 * recall_pop and recall_pop > 0


def test_to_svd_model_at_a_width_the_svd_model_refuses():
    with T.ImplicitALS(5, 7, factors=65, solver="cg") as m:
        with pytest.raises(T.TfrError):
            m.to_svd_model()
    with T.ImplicitALS(5, 7, factors=68, solver="cg") as m:
        m.init_factors(0)
        with m.to_svd_model() as svd:
            assert svd.tables()[L.P].tobytes() == m.user_factors.astype(np.float32).tobytes()


# ----------------------------------------------------------------------------- errors
def test_refusals():
    lib = L.load()
    for d, steps, lam, alpha in ((0, 3, 0.1, 1.0), (257, 3, 0.1, 1.0), (8, 0, 0.1, 1.0), (8, 1025, 0.1, 1.0), (8, 3, 0.0, 1.0),
                                 (8, 3, -1.0, 1.0), (8, 3, 0.1, -1.0)):
        h = L._p()
        assert lib.tfr_ials_create_cg(C_.byref(h), 4, 4, d, lam, alpha, steps, 0) == L.ERR_ARG and not h.value
    case = BY_ID["cg-widths-d65"]
    with _open(case, 3, load=False) as m:
        ms, out = C_.c_float(), C_.c_double()
        assert lib.tfr_ials_half(m._h, 0, C_.byref(ms)) == L.ERR_STATE
        assert lib.tfr_ials_sweep(m._h, 1, C_.byref(ms)) == L.ERR_STATE
        assert lib.tfr_ials_loss(m._h, C_.byref(out)) == L.ERR_STATE
        assert _same(_both(m), (case["X"], case["Y"]))
    with pytest.raises(T.TfrError):
        T.ImplicitALS(4, 4, factors=128)                    # the default solver keeps its limit
    with T.ImplicitALS(4, 4, factors=256, solver="cg", cg_steps=1024) as m:
        assert m.gram(0).shape == (256, 256)
