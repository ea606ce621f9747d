"""Implicit-feedback ALS on the device (csrc/ials.hip through ImplicitALS) against the longdouble restatements of
tests/ials_ref.py on the cases of tests/ials_cases.py.  The Gram, the user half and the item half are told apart: the user
half is checked from the case's tables, the item half with the reference fed the device's own X, and each half's reference
takes the device's own Gram, which has its own, derived, bound.  Then what must hold bit for bit, the loss, a ten-iteration
trajectory, planted blocks end to end, the export into an SvdModel, and the refusals."""
import ctypes as C_
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import ials_cases as C
from tests import ials_ref as R
from tests import topk_ref

pytestmark = pytest.mark.gpu

BY_ID = {c["id"]: c for c in C.CASES}


def _open(case, chunk=None, load=True):
    m = T.ImplicitALS(case["nu"], case["ni"], factors=case["d"], regularization=case["lam"], alpha=case["alpha"],
                      chunk=case["chunk"] if chunk is None else chunk)
    m.set_factors(case["X"], case["Y"])
    if load:
        m.load(C.csr(case))
    return m


def _both(m):
    return m.user_factors, m.item_factors


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _check_case(case, dense=False, sides=(0, 1)):
    """the half-sweeps of ``sides`` in turn, each held to the reference fed the tables the device read and the device's own
    Gram of them; returns (X, Y) after them"""
    with _open(case) as m:
        lst = R.lists(case, 0), R.lists(case, 1)
        tabs = [case["X"], case["Y"]]
        bad, rho = [], {}
        for side in sides:
            other = tabs[1 - side]
            G = m.gram(1 - side)
            m.half_sweep(side)
            got = m.user_factors if side == 0 else m.item_factors
            what = "%s, %s half" % (case["id"], ("user", "item")[side])
            ref = R.half(other, lst[side], case["lam"], case["alpha"], G=G)
            bad += R.check_half(ref, got, R.K, what)
            rho[side] = float(R.ratios(ref, got).max())
            untouched = m.item_factors if side == 0 else m.user_factors
            assert untouched.tobytes() == other.tobytes(), "%s wrote the other table" % what
            err = np.abs(G.astype(R.LD) - R.gram(other)).astype(np.float64)
            if not (err <= R.gram_bound(other)).all():
                bad.append("%s: its Gram is outside (n + 2) eps |T|^T |T| by %.3g" % (what, (err / R.gram_bound(other)).max()))
            if dense:
                bad += R.check_half(R.dense_half(other, lst[side], case["lam"], case["alpha"]), got, R.K, what + ", definition")
            tabs[side] = got
        print("RATIO %s %s" % (case["id"], rho))
        assert not bad, "\n".join(bad)
        if tuple(sides) == (0, 1):
            m.set_factors(case["X"], case["Y"])            # the same sweep again, in one call: the same bits
            m.sweep(1)
            assert _same(tabs, _both(m)), "%s: half(0); half(1) and sweep(1) from the same tables differ" % case["id"]
        return tabs


# ----------------------------------------------------------------------------- Gram
@pytest.mark.parametrize("n,d", list(zip(C.GRAM_NS, (64, 33, 64, 17, 64, 3))))
def test_gram_against_longdouble_per_entry(n, d):
    rs = np.random.RandomState(n)
    X, Y = rs.uniform(-1.0, 1.0, (n, d)), rs.uniform(-1.0, 1.0, (3, d))
    with T.ImplicitALS(n, 3, factors=d) as m:
        m.set_factors(X, Y)
        G, Gi, again = m.gram(0), m.gram(1), m.gram(0)
    assert G.tobytes() == again.tobytes()
    for got, tab in ((G, X), (Gi, Y)):
        err = np.abs(got.astype(R.LD) - R.gram(tab)).astype(np.float64)
        assert (err <= R.gram_bound(tab)).all(), float((err / R.gram_bound(tab)).max())


# ----------------------------------------------------------------------------- half-sweeps per entity
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_one_sweep_per_entity_half_by_half(case):
    _check_case(case, dense=case["id"] in C.DENSE_IDS)


@functools.lru_cache(maxsize=None)
def _grid(which):
    return getattr(C, which)()


def _alone(case, u):
    """the case with only user u's row"""
    keep = np.zeros(case["nu"], bool)
    keep[u] = True
    x = C.csr(case).multiply(keep[:, None]).tocsr()
    x.eliminate_zeros()
    x.sort_indices()
    return dict(case, indptr=x.indptr.astype(np.int64), items=x.indices.astype(np.int32), vals=np.ascontiguousarray(x.data, np.float64))


def _check_alone(case, X, users):
    for u in users:
        with _open(_alone(case, u)) as m:
            m.half_sweep(0)
            assert m.user_factors[u].tobytes() == X[u].tobytes(), "%s: user %d alone differs from itself in the crowd" % (case["id"], u)


@pytest.mark.parametrize("swap", [False, True], ids=["as-given", "swapped"])
def test_more_entities_than_the_grid(swap):
    """70 000 entities on one side, every tenth of them empty: k_ials_fit's blocks each take a second one.  Both halves are
    checked, every entity."""
    case = C.swapped(_grid("grid_entities")) if swap else _grid("grid_entities")
    assert max(case["nu"], case["ni"]) > 65535 and min(case["nu"], case["ni"]) == 300
    X, _ = _check_case(case)
    if not swap:
        _check_alone(case, X, [5, 5 + 65535 + 1])          # user 65 541 is its block's second entity (65 540 is empty)


@pytest.mark.parametrize("swap", [False, True], ids=["as-given", "swapped"])
def test_more_chunks_than_the_grid(swap):
    """66 000 chunks at chunk = 32 and d = 9: k_ials_partial's blocks each take a second one.  The chunked half is checked,
    every entity (the reference of the other half would double the test's time and adds no path)."""
    case = C.swapped(_grid("grid_chunks")) if swap else _grid("grid_chunks")
    side = 1 if swap else 0
    assert R.n_chunks(R.lists(case, side)[0], 32).sum() > 65535
    X, _ = _check_case(case, sides=(side,))
    if not swap:
        _check_alone(case, X, [5, case["nu"] - 1])         # the last user's chunks lie beyond the grid: each is some block's second


# ----------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("cid", ["chunk32-d9", "widths-d28-swapped", "long-d64"])
def test_three_sweeps_in_one_call_equal_three_calls_and_six_halves(cid):
    case = BY_ID[cid]
    with _open(case) as m:
        m.sweep(3)
        once = _both(m)
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


@pytest.mark.parametrize("cid,users", [("chunk32-d9", (0, 2, 8, 10)), ("chunk64-d33", (1, 5, 9)), ("long-d33", (0, 2, 4, 5)),
                                        ("widths-d63", (1, 4, 8))])
def test_an_entity_alone_equals_itself_in_the_crowd(cid, users):
    case = BY_ID[cid]
    with _open(case) as m:
        m.half_sweep(0)
        X = m.user_factors
    _check_alone(case, X, users)


def test_a_second_load_replaces_the_first():
    first = BY_ID["chunk32-d9"]
    rs = np.random.RandomState(77)
    nu, ni, d = first["nu"], first["ni"], 9
    X, Y = rs.rand(nu, d), rs.rand(ni, d)
    a = sp.random(nu, ni, 0.05, random_state=rs, data_rvs=lambda n: rs.randint(1, 5, n).astype(np.float64)).tocsr()
    with T.ImplicitALS(nu, ni, factors=d, regularization=0.1, alpha=40.0, chunk=32) as m:
        m.set_factors(X, Y)
        m.load(a)
        m.sweep(1)
        fresh = _both(m)
        m.set_factors(X, Y)
        m.load(C.csr(first))                               # chunked lists on both sides
        m.sweep(1)
        moved = _both(m)
        m.set_factors(X, Y)
        m.load(a)                                          # fewer pairs, no chunks: as if the first load had never been
        m.sweep(1)
        assert not _same(moved, fresh) and _same(_both(m), fresh)


@pytest.mark.parametrize("swap", [False, True], ids=["as-given", "swapped"])
@pytest.mark.parametrize("d", [9, 33])
def test_chunk_sizes_agree_within_the_bound(d, swap):
    """the same data at chunk 32, 64 and 512 (nothing chunked): the user half, which reads the same tables in all three,
    agrees within the per-entity bound, and the chunked entities do differ somewhere"""
    case = BY_ID["chunk32-d%d" % d + ("-swapped" if swap else "")]
    got = {}
    for ch in (32, 64, 512):
        with _open(case, chunk=ch) as m:
            m.half_sweep(0)
            got[ch] = m.user_factors
    ref = R.half(case["Y"], R.lists(case, 0), case["lam"], case["alpha"])
    for ch in (32, 64, 512):
        assert not R.check_half(ref, got[ch], R.K, "chunk %d" % ch)
    assert R.n_chunks(case["indptr"], 32).max() >= 2 and R.n_chunks(case["indptr"], 512).sum() == 0
    for ch in (32, 64):                                    # swapped, the one long list (41 users) is cut at 32 only
        cut = R.n_chunks(case["indptr"], ch) > 0
        assert (got[ch][~cut] == got[512][~cut]).all()
        assert not cut.any() or (got[ch][cut] != got[512][cut]).any(), "chunk %d: no chunked entity differs at all" % ch


# ----------------------------------------------------------------------------- loss
DENSE = [BY_ID[i] for i in C.DENSE_IDS]


@pytest.mark.parametrize("case", DENSE, ids=lambda c: c["id"])
def test_loss_against_the_definition_and_never_increasing(case):
    with _open(case) as m:
        X, Y = case["X"], case["Y"]
        last = None
        for step in range(11):
            got = m.loss()
            if step in (0, 1, 2, 10):
                want, terms = R.loss_dense(X, Y, case), R.loss_terms(X, Y, case)
                err = float(abs(R.LD(got) - want))
                print("LOSS %s step %d: %.17g, error %.3g of the bound" % (case["id"], step, got, err / (R.K_LOSS * R.EPS * terms)))
                assert err <= R.K_LOSS * R.EPS * terms, (case["id"], step, got, float(want))
            if last is not None and case["lam"] >= 1e-3:
                assert got <= last + R.K_LOSS * R.EPS * R.loss_terms(*_both(m), case), (case["id"], step, last, got)
            last = got
            if step < 10:
                m.half_sweep(step % 2)
                X, Y = _both(m)
        assert m.loss() == last


# ----------------------------------------------------------------------------- trajectory
def test_ten_iterations_follow_the_float64_restatement():
    case = C.trajectory()
    with T.ImplicitALS(case["nu"], case["ni"], factors=8, regularization=0.1, alpha=40.0, iterations=10) as m:
        m.fit(C.csr(case), seed=0)
        X, Y = _both(m)
        assert m.sweep_ms > 0
    wx, wy = R.sweep_f64(case, case["X"], case["Y"], 10)
    for name, got, want in (("X", X, wx), ("Y", Y, wy)):
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= 1e-9, "%s: %.3e" % (name, err)


# ----------------------------------------------------------------------------- end to end
def test_planted_blocks_are_recovered():
    """200 users in 4 groups, 120 items in 4 blocks; each user holds 12 items of its block and 2 random ones, one in-block
    item is held out.  recall@10 of the held-out item is at least twice that of the popularity ranking."""
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
    with T.ImplicitALS(U, I, factors=8, regularization=0.01, alpha=40.0, iterations=10) as m:
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
    print("planted blocks: recall@10 iALS %.3f, popularity %.3f" % (recall, recall_pop))
    assert recall >= 2 * recall_pop and recall_pop > 0


# ----------------------------------------------------------------------------- export
def test_to_svd_model_holds_the_float32_casts_and_recommends_by_dot_product():
    rs = np.random.RandomState(5)
    U, I, d = 70, 150, 24
    X, Y = rs.randint(-8, 9, (U, d)) / 8.0, rs.randint(-8, 9, (I, d)) / 8.0      # dyadic: float32 dots are exact, ties are real
    with T.ImplicitALS(U, I, factors=d) as m:
        m.set_factors(X, Y)
        with m.to_svd_model() as svd:
            t = svd.tables()
            users = np.arange(U, dtype=np.int32)
            items, scores = svd.recommend(users, 10)
        assert m.user_factors.tobytes() == X.tobytes()
    assert t[L.P].tobytes() == X.astype(np.float32).tobytes() and t[L.Q].tobytes() == Y.astype(np.float32).tobytes()
    assert t[L.MU] == 0 and not t[L.BU].any() and not t[L.BI].any()
    S = topk_ref.svd_scores(t[L.P], t[L.Q], t[L.BU], t[L.BI], 0.0, users)
    wi, ws = topk_ref.topk_ref(S, 10)
    assert np.array_equal(items, wi) and np.array_equal(scores, ws)
    case = C.trajectory()                                   # fitted, non-dyadic factors: still the casts
    with _open(case) as m:
        m.sweep(2)
        with m.to_svd_model() as svd:
            t = svd.tables()
        assert t[L.P].tobytes() == m.user_factors.astype(np.float32).tobytes()
        assert t[L.Q].tobytes() == m.item_factors.astype(np.float32).tobytes()


# ----------------------------------------------------------------------------- errors
def test_refusals_leave_the_model_as_it_was():
    lib = L.load()
    for d, lam, alpha in ((0, 0.1, 1.0), (65, 0.1, 1.0), (8, 0.0, 1.0), (8, -1.0, 1.0), (8, 0.1, -1.0)):
        h = L._p()
        assert lib.tfr_ials_create(C_.byref(h), 4, 4, d, lam, alpha, 0) == L.ERR_ARG and not h.value
    case = BY_ID["chunk32-d9"]
    with _open(case) as m:
        m.sweep(1)
        want = _both(m)
    with _open(case, load=False) as m:
        ms, out = C_.c_float(), C_.c_double()
        assert lib.tfr_ials_sweep(m._h, 1, C_.byref(ms)) == L.ERR_STATE     # nothing loaded yet
        assert lib.tfr_ials_half(m._h, 0, C_.byref(ms)) == L.ERR_STATE
        assert lib.tfr_ials_loss(m._h, C_.byref(out)) == L.ERR_STATE
        assert lib.tfr_ials_half(m._h, 2, None) == L.ERR_ARG
        m.load(C.csr(case))

        def load(indptr=case["indptr"], items=case["items"], vals=case["vals"], chunk=32):
            indptr, items, vals = np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(items, np.int32), np.ascontiguousarray(vals, np.float64)
            return lib.tfr_ials_load(m._h, L.ptr_i64(indptr), L.ptr_i32(items), vals.ctypes.data_as(L._f64p), chunk)

        def changed(a, k, v):
            a = a.copy()
            a[k] = v
            return a

        mid = int(case["indptr"][3]) + 1                      # inside user 3's row
        for bad in (0.0, -1.0, np.nan, np.inf):
            assert load(vals=changed(case["vals"], mid, bad)) == L.ERR_ARG
        assert load(items=changed(case["items"], mid, case["items"][mid - 1])) == L.ERR_ARG    # a repeated pair
        assert load(items=changed(case["items"], mid, 0)) == L.ERR_ARG                          # a row out of order
        assert load(items=changed(case["items"], mid, case["ni"])) == L.ERR_OOB
        assert load(items=changed(case["items"], mid, -1)) == L.ERR_OOB
        for chunk in (-32, 16, 48, 33):
            assert load(chunk=chunk) == L.ERR_ARG
        assert b"chunk" in lib.tfr_ials_last_error()
        with pytest.raises(IndexError):
            m._check(L.ERR_OOB)
        m.sweep(1)                                            # still the lists (and the chunk size) of the good load
        assert _same(_both(m), want)
        assert load(chunk=0) == L.OK                          # 0 = 512
