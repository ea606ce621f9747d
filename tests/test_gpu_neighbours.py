"""Nearest neighbours in factor space on the device (tfr_neighbours* / similar_items, similar_users, similar_features) against
the NumPy statement of the contract in tests/neighbours_ref.py."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests.neighbours_ref import (neighbours_ref, neighbours_from_scores, neighbour_scores, scores_f64, dyadic_table,
                                  pow4_table)
from tests import svdpp_ref
from tests import widths as W

pytestmark = pytest.mark.gpu

KS = (1, 10, 129, 256)                                     # both queue capacities (k + 128 <= 256, and above)
LDS_PER_CU = 160 * 1024                                    # the limit tests/test_lds_budget.py uses
SEED = 20                                                  # the toleranced tests' seed (see test_random_tables_within_tolerance)


def svd_model(P, Q, **kw):
    U, I, D = P.shape[0], Q.shape[0], P.shape[1]
    m = T.SvdModel(U, I, D, **kw)
    m.set_tables(np.float32(0.25), np.zeros(U, np.float32), np.zeros(I, np.float32), P, Q)
    return m


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def with_ties(rs, t):
    """duplicate rows (exact ties, ordered by id only), a mirrored row and a zero row, where the table is large enough"""
    R = t.shape[0]
    if R >= 31:
        src = rs.randint(0, R, 6)
        for s in src:
            t[rs.randint(0, R, 3)] = t[s]
        t[R // 2] = -t[src[0]]
        t[R // 3] = 0
    return t


def queries(rs, R):
    return [np.arange(R, dtype=np.int32), np.array([rs.randint(R)], np.int32),
            np.array([R - 1, 0, R // 2, 0, R - 1, R - 1], np.int32)]


@pytest.mark.parametrize("R", [1, 31, 33, 129, 300])       # across the 32-row tile, the 128-row round and a slice boundary
@pytest.mark.parametrize("D", W.TOPK)
def test_exact_ids_and_scores(R, D):
    rs = np.random.RandomState(1000 * R + D)
    Q = with_ties(rs, dyadic_table(rs, R, D))              # dot exact
    P = with_ties(rs, pow4_table(rs, R, D))                # dot and cosine exact
    m = svd_model(P, Q)
    cases = [("items", Q, "dot", m.similar_items), ("users", P, "dot", m.similar_users), ("users", P, "cosine", m.similar_users)]
    qs = queries(rs, R)
    for name, tab, metric, fn in cases:
        allrows = np.arange(R)
        wi, ws = neighbours_from_scores(neighbour_scores(tab, allrows, metric), allrows, max(KS))
        for k in KS:
            for q in qs:
                ids, sc = fn(q, k, metric)
                assert np.array_equal(ids, wi[q][:, :k]), (name, metric, k, q.size)
                assert np.array_equal(bits(sc), bits(ws[q][:, :k])), (name, metric, k, q.size)
                assert not np.any(ids == q[:, None])                            # self never returned
                assert np.all(ids[:, R - 1:] == -1) and np.all(sc[:, R - 1:] == -np.inf)
    m.close()


def boundary_mismatches(ids, ref_ids, S_ref, tol):
    """ids that are in one of the two top-k sets only: each must score (by S_ref) within tol of the reference's k-th score;
    returns how many there are"""
    n = 0
    for r in range(ids.shape[0]):
        kth = S_ref[r, ref_ids[r, -1]]
        odd = np.array(sorted(set(ids[r].tolist()) ^ set(ref_ids[r].tolist())), np.int64)
        assert np.all(np.abs(S_ref[r, odd] - kth) <= tol), (r, odd, S_ref[r, odd], kth, tol)
        n += odd.size
    return n


@pytest.mark.parametrize("D", [64, 27])
def test_random_tables_within_tolerance(D):
    """Seed 20: on the CPU the f32 statement against float64 leaves no more than 2 % of k n ids to the boundary rule at both
    widths (checked below before the device is asked)."""
    rs = np.random.RandomState(SEED)
    R, k = 1200, 10
    Tab = rs.normal(0, .3, (R, D)).astype(np.float32)
    rows = np.arange(R, dtype=np.int32)
    cap = 0.02 * k * R
    m = svd_model(Tab[:8].copy(), Tab)
    for metric in ("cosine", "dot"):
        S64 = scores_f64(Tab, rows, metric)
        S32 = neighbour_scores(Tab, rows, metric)
        tol = 4 * float(np.abs(S32 - S64).max())           # what the f32 statement itself deviates, x 4 for 1 / sqrtf
        ref_ids, ref_sc = neighbours_from_scores(S32, rows, k)
        ids64, _ = neighbours_from_scores(S64.astype(np.float32), rows, k)
        n_cpu = boundary_mismatches(ids64, ref_ids, S32.astype(np.float64), tol)
        ids, sc = m.similar_items(rows, k, metric)
        got64 = np.take_along_axis(S64, ids.astype(np.int64), 1)
        print("D %d %s: tol %.3e, max |score - float64| %.3e, boundary ids cpu %d gpu" % (
            D, metric, tol, float(np.abs(sc - got64).max()), n_cpu), end=" ")
        assert n_cpu <= cap, (metric, n_cpu, cap)
        assert np.all(ids >= 0) and not np.any(ids == rows[:, None])
        assert np.all(np.abs(sc - got64) <= tol), (metric, float(np.abs(sc - got64).max()), tol)
        n_gpu = boundary_mismatches(ids, ref_ids, S32.astype(np.float64), tol)
        print(n_gpu)
        assert n_gpu <= cap, (metric, n_gpu, cap)
    m.close()


def random_excl(rs, n, R, frac=0.2):
    rows = [np.unique(rs.randint(0, R, rs.randint(0, max(1, int(R * frac))))) for _ in range(n)]
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return (indptr, np.concatenate(rows).astype(np.int32)), rows


@pytest.mark.parametrize("item_abs", [False, True])
def test_exclusions_range_zero_rows_item_abs_and_padding(item_abs):
    rs = np.random.RandomState(31 + item_abs)
    R, D = 300, 33
    Q = with_ties(rs, pow4_table(rs, R, D))
    Q[[4, 5, 250]] = 0
    m = svd_model(Q[:5].copy(), Q, item_abs=item_abs)
    q = np.concatenate([rs.randint(0, R, 60), [4, 5, 250, 4]]).astype(np.int32)
    ex, rows = random_excl(rs, q.size, R)
    for metric in ("cosine", "dot"):
        for k in (10, 256):
            for kw, rkw in ((dict(exclude=ex), dict(excl=rows)), (dict(lo=100, hi=229), dict(lo=100, hi=229)),
                            (dict(exclude=ex, lo=3, hi=7), dict(excl=rows, lo=3, hi=7))):
                ids, sc = m.similar_items(q, k, metric, **kw)
                wi, ws = neighbours_ref(Q, q, k, metric, item_abs=item_abs, **rkw)
                assert np.array_equal(ids, wi), (metric, k, kw.keys())
                assert np.array_equal(bits(sc), bits(ws)), (metric, k, kw.keys())
                if "exclude" in kw:
                    assert all(not set(ids[r].tolist()) & set(rows[r].tolist()) for r in range(q.size))
                if "lo" in kw:
                    assert np.all((ids == -1) | ((ids >= kw["lo"]) & (ids < kw["hi"])))
    # a zero row: every cosine is +0, so its neighbours are the lowest ids; nothing is NaN
    ids, sc = m.similar_items([250], 5)
    assert ids[0].tolist() == [0, 1, 2, 3, 4] and np.all(bits(sc) == 0)
    # everything excluded: -1 / -inf; ids only: no scores array
    allx = (np.array([0, R], np.int64), np.arange(R, dtype=np.int32))
    ids, sc = m.similar_items([9], 7, exclude=allx)
    assert np.all(ids == -1) and np.all(sc == -np.inf)
    only = m.similar_items([9, 10], 7, return_scores=False)
    assert only.shape == (2, 7) and np.array_equal(only, m.similar_items([9, 10], 7)[0])
    assert m.similar_items(np.zeros(0, np.int32), 3)[0].shape == (0, 3)
    # NaN rows are never returned, and a NaN query row has no neighbours
    Qn = Q.copy()
    Qn[17] = np.nan
    m.set_table(L.Q, Qn)
    ids, sc = m.similar_items([1, 17], 256, lo=0, hi=200)
    assert 17 not in ids[0] and np.all(ids[0, :198] >= 0) and np.all(ids[0, 198:] == -1) and np.all(ids[1] == -1)
    m.close()


def test_errors_and_model_still_works():
    import torch
    rs = np.random.RandomState(41)
    Q = dyadic_table(rs, 30, 16)
    m = svd_model(dyadic_table(rs, 20, 16), Q)
    lib = L.load()
    out = np.full((2, 4), 77, np.int32)
    good, ip = np.array([0, 1], np.int32), np.array([0, 1, 2], np.int64)

    def call(rows=good, which=L.NB_ITEMS, metric=1, k=4, indptr=None, excl=None, lo=0, hi=30):
        return lib.tfr_neighbours(m._h, which, metric, L.ptr_i32(rows), 2, k, None if indptr is None else L.ptr_i64(indptr),
                                  None if excl is None else L.ptr_i32(excl), lo, hi, L.ptr_i32(out), None)
    assert call(rows=np.array([0, 30], np.int32)) == L.ERR_OOB
    assert call(rows=np.array([0, 20], np.int32), which=L.NB_USERS, hi=20) == L.ERR_OOB
    assert call(indptr=ip, excl=np.array([3, 30], np.int32)) == L.ERR_OOB
    assert call(indptr=np.array([0, 0, 2], np.int64), excl=np.array([5, 3], np.int32)) == L.ERR_ARG
    for bad in (dict(k=0), dict(k=257), dict(metric=2), dict(metric=-1), dict(which=2), dict(lo=-1), dict(lo=5, hi=5),
                dict(hi=31), dict(which=L.NB_USERS, hi=21)):
        assert call(**bad) == L.ERR_ARG, bad
    assert np.all(out == 77)                                # outputs untouched by every refused call
    with pytest.raises(ValueError):
        m.similar_items([0], 3, metric="euclid")
    dev = torch.device("cuda", 0)
    dq = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    with pytest.raises(L.TfrError) as e:                    # the top-K error bits: 16 for an unsorted row, 1 for an id out of range
        m.similar_items_dev(dq, 4, exclude=(torch.tensor([0, 0, 2], device=dev), torch.tensor([5, 3], dtype=torch.int32, device=dev)))
        m.sync()
    assert e.value.code == L.ERR_ARG
    with pytest.raises(L.OutOfRangeError):
        m.similar_items_dev(dq, 4, exclude=(torch.tensor([0, 1, 2], device=dev), torch.tensor([3, 30], dtype=torch.int32, device=dev)))
        m.sync()
    with pytest.raises(L.OutOfRangeError):
        m.similar_items_dev(torch.tensor([0, 30], dtype=torch.int32, device=dev), 4)
        m.sync()
    ids, sc = m.similar_items(good, 4, "dot")
    wi, ws = neighbours_ref(Q, good, 4, "dot")
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws))
    logits, _, _ = m.train_step([0, 1], [2, 3], [1.0, 2.0])
    assert np.all(np.isfinite(logits))
    m.close()


def fresh_answer(m, which, q, k):
    """the same query on a new model loaded with m's tables as they are now"""
    t = m.tables()
    with T.SvdModel(m.user_num, m.item_num, m.dim) as f:
        f.set_tables(t[L.MU], t[L.BU], t[L.BI], t[L.P], t[L.Q])
        return getattr(f, which)(q, k, "cosine")


def test_inverse_norms_follow_the_tables():
    """query, train (or load a table), query again: the cached inverse norms must not outlive the tables they were made from"""
    rs = np.random.RandomState(51)
    U, I, D, k = 150, 260, 20, 10
    m = T.SvdModel(U, I, D, optimizer="sgd", lr=0.05)
    m.init_tables(seed=5, feature_stddev=0.3, bias_stddev=0.5)
    qi, qu = np.arange(0, I, 3, dtype=np.int32), np.arange(0, U, 2, dtype=np.int32)
    u, i, r = rs.randint(0, U, 4000), rs.randint(0, I, 4000), rs.randint(1, 6, 4000).astype(np.float32)

    def both():
        return m.similar_items(qi, k), m.similar_users(qu, k)

    def check(before):
        now = both()
        for (ids, sc), which, q, (_, sc0) in zip(now, ("similar_items", "similar_users"), (qi, qu), before):
            wi, ws = fresh_answer(m, which, q, k)
            assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), which
            assert not np.array_equal(bits(sc), bits(sc0)), which      # the tables did move
        return now
    first = both()
    again = both()                                          # served from the cache: the same bits
    assert all(np.array_equal(bits(a[1]), bits(b[1])) for a, b in zip(first, again))
    m.train_step(u, i, r)
    second = check(first)
    import torch
    dev = torch.device("cuda", 0)
    du, di, dr = (torch.from_numpy(x).to(dev) for x in (u.astype(np.int32), i.astype(np.int32), r))
    torch.cuda.synchronize(dev)                             # the step runs on the model's stream
    m.train_step_dev(du.data_ptr(), di.data_ptr(), dr.data_ptr(), u.size)      # asynchronous: the query is ordered after it
    third = check(second)
    m.set_table(L.Q, (m.get_table(L.Q) * np.linspace(0.5, 2, D, dtype=np.float32)).astype(np.float32))
    m.set_table(L.P, (m.get_table(L.P) * np.linspace(2, 0.5, D, dtype=np.float32)).astype(np.float32))
    fourth = check(third)
    m.init_tables(seed=6, feature_stddev=0.3, bias_stddev=0.5)
    check(fourth)
    m.close()


def test_device_entries_equal_host_entries():
    import torch
    rs = np.random.RandomState(61)
    R, D = 700, 64
    P, Q = rs.normal(0, .3, (R, D)).astype(np.float32), rs.normal(0, .3, (R, D)).astype(np.float32)
    m = svd_model(P, Q)
    q = rs.randint(0, R, 300).astype(np.int32)
    ex, _ = random_excl(rs, q.size, R)
    dev = torch.device("cuda", 0)
    dq, dex = torch.from_numpy(q).to(dev), (torch.from_numpy(ex[0]).to(dev), torch.from_numpy(ex[1]).to(dev))
    for host, devf in ((m.similar_items, m.similar_items_dev), (m.similar_users, m.similar_users_dev)):
        for metric in ("cosine", "dot"):
            for k in (25, 200):
                hi_, hs = host(q, k, metric, exclude=ex, lo=10, hi=650)
                di, ds = devf(dq, k, metric, exclude=dex, lo=10, hi=650)
                m.sync()
                assert np.array_equal(di.cpu().numpy(), hi_)
                assert np.array_equal(bits(ds.cpu().numpy()), bits(hs))
    m.close()


def test_query_chunks_rebase_the_exclusions():
    """65536 + 33 queries: two chunks of the shared driver (csrc/topk.h TOPK_CHUNK_MAX), the second with its exclusion indptr
    rebased on the host path and offset on the device path.  Every row is checked, the chunk's edge rows by name."""
    import torch
    rs = np.random.RandomState(111)
    R, D, k, n = 300, 8, 10, 65536 + 33
    assert T.neighbours.plan(D, k, n, R)["row_chunk"] == 65536
    Q = with_ties(rs, dyadic_table(rs, R, D))              # dot exact
    m = svd_model(Q[:4].copy(), Q)
    q = rs.randint(0, R, n).astype(np.int32)
    rows = [np.unique(rs.randint(0, R, rs.randint(1, 60))) if r % 10 == 0 else np.zeros(0, np.int64) for r in range(n)]
    ex = (np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32))
    hi_, hs = m.similar_items(q, k, "dot", exclude=ex)
    dev = torch.device("cuda", 0)
    di, ds = m.similar_items_dev(torch.from_numpy(q).to(dev), k, "dot",
                                 exclude=(torch.from_numpy(ex[0]).to(dev), torch.from_numpy(ex[1]).to(dev)))
    m.sync()
    assert np.array_equal(di.cpu().numpy(), hi_) and np.array_equal(bits(ds.cpu().numpy()), bits(hs))
    S = neighbour_scores(Q, np.arange(R), "dot")           # per table row, shared by the repeats
    free_i, free_s = neighbours_from_scores(S, np.arange(R), k)
    wi, ws = free_i[q], free_s[q]
    with_x = np.arange(0, n, 10)
    wi[with_x], ws[with_x] = neighbours_from_scores(S[q[with_x]], q[with_x], k, [rows[r] for r in with_x])
    for r in (0, 65535, 65536, n - 1):
        ri, rsc = neighbours_ref(Q, q[r:r + 1], k, "dot", excl=[rows[r]])
        assert np.array_equal(hi_[r], ri[0]) and np.array_equal(bits(hs[r]), bits(rsc[0])), r
    assert np.array_equal(hi_, wi) and np.array_equal(bits(hs), bits(ws))
    assert any(not np.array_equal(wi[r], free_i[q[r]]) for r in with_x if r >= 65536)   # the second chunk's exclusions bite
    m.close()


def pow4_implicit(U, I, rs):
    """|N(u)| in {0, 1, 4, 16}: s_u a power of two, so that on dyadic tables e_u = P[u] + z_u is exact"""
    rows = [np.sort(rs.choice(I, (0, 1, 4, 16)[rs.randint(4)], replace=False)) for _ in range(U)]
    indptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


@pytest.mark.parametrize("D", [33, 64])
def test_svdpp(D):
    import torch
    rs = np.random.RandomState(71 + D)
    U, I, k = 140, 90, 12
    P, Q, Y = dyadic_table(rs, U, D), with_ties(rs, pow4_table(rs, I, D)), dyadic_table(rs, I, D)
    N = pow4_implicit(U, I, rs)
    zero = np.zeros
    qi, qu = rs.randint(0, I, 50).astype(np.int32), rs.randint(0, U, 70).astype(np.int32)
    s = svd_model(P, Q)
    with T.SvdppModel(U, I, D) as pp:
        pp.set_implicit(N)
        # Y = 0: the SVD model on the same tables, bit for bit, users and items
        pp.set_tables(np.float32(0.25), zero(U, np.float32), zero(I, np.float32), P, Q, zero((I, D), np.float32))
        for metric in ("cosine", "dot"):
            for a, b, q in ((pp.similar_items, s.similar_items, qi), (pp.similar_users, s.similar_users, qu)):
                gi, gs = a(q, k, metric)
                wi, ws = b(q, k, metric)
                assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws)), metric
        # users on the effective rows e_u = P[u] + z_u: exact on these tables, so the dot form is equal bit for bit
        pp.set_table(L.Y, Y)
        z, _, _ = svdpp_ref.implicit_parts(Y.astype(np.float64), N[0], N[1], np.arange(U))
        E = (P.astype(np.float64) + z).astype(np.float32)
        assert np.array_equal(E.astype(np.float64), P.astype(np.float64) + z)
        gi, gs = pp.similar_users(qu, k, "dot")
        wi, ws = neighbours_ref(E, qu, k, "dot")
        assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws))
        assert not np.array_equal(gi, s.similar_users(qu, k, "dot")[0])        # z does enter
        # the cosine of the same rows within the f32 statement's own deviation from float64, x 4
        S64, S32 = scores_f64(E, qu, "cosine"), neighbour_scores(E, qu, "cosine")
        tol = 4 * float(np.abs(S32 - S64).max())
        gi, gs = pp.similar_users(qu, k, "cosine")
        assert np.all(np.abs(gs - np.take_along_axis(S64, gi.astype(np.int64), 1)) <= tol)
        boundary_mismatches(gi, neighbours_from_scores(S32, qu, k)[0], S32.astype(np.float64), tol)
        # items are unchanged by Y, and a user query does not disturb the item side's cached norms
        gi, gs = pp.similar_items(qi, k)
        wi, ws = s.similar_items(qi, k)
        assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws))
        # device twins
        dev = torch.device("cuda", 0)
        for fn, dfn, q in ((pp.similar_users, pp.similar_users_dev, qu), (pp.similar_items, pp.similar_items_dev, qi)):
            hi_, hs = fn(q, k)
            di, ds = dfn(torch.from_numpy(q).to(dev), k)
            pp.sync()
            assert np.array_equal(di.cpu().numpy(), hi_) and np.array_equal(bits(ds.cpu().numpy()), bits(hs))
    s.close()


@pytest.mark.parametrize("D", W.FM_TOPK)
def test_fm_similar_features_over_a_block(D):
    rs = np.random.RandomState(81 + D)
    Un, In, k = 40, 260, 10
    F = Un + In
    V = with_ties(rs, pow4_table(rs, F, D))
    with T.FmModel(F, D) as fm:
        fm.set(0.5, dyadic_table(rs, F, 1).reshape(-1), V)
        feats = (Un + rs.randint(0, In, 30)).astype(np.int32)
        for metric in ("cosine", "dot"):
            ids, sc = fm.similar_features(feats, Un, F, k, metric)                # "items like this one"
            wi, ws = neighbours_ref(V, feats, k, metric, lo=Un, hi=F)
            assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws)), metric
            # the same as the contract on the block V[lo:hi] alone, ids shifted by lo
            bi, bs = neighbours_ref(V[Un:F], feats - Un, k, metric)
            assert np.array_equal(ids, np.where(bi >= 0, bi + Un, -1)) and np.array_equal(bits(sc), bits(bs))
        ids, _ = fm.similar_features([3], 0, Un, 5, "dot")                        # the user block
        assert np.array_equal(ids, neighbours_ref(V, [3], 5, "dot", lo=0, hi=Un)[0])
        ids, _ = fm.similar_features([3], k=5)                                    # every feature
        assert np.array_equal(ids, neighbours_ref(V, [3], 5)[0])
        with pytest.raises(T.TfrError) as e:
            fm.similar_features([3], 0, F + 1)
        assert e.value.code == L.ERR_ARG
        with pytest.raises(L.OutOfRangeError):
            fm.similar_features([F], 0, F)


def test_queries_leave_the_model_untouched():
    rs = np.random.RandomState(91)
    U, I, D = 120, 200, 32
    batches = [(rs.randint(0, U, 500), rs.randint(0, I, 500), rs.randint(1, 6, 500).astype(np.float32)) for _ in range(3)]
    res = []
    for interleave in (False, True):
        m = T.SvdModel(U, I, D, adam_mode="lazy")
        m.init_tables(seed=9, feature_stddev=0.3, bias_stddev=0.5)
        for u, i, r in batches:
            m.train_step(u, i, r)
            if interleave:
                step = m.get_step()
                m.similar_items(np.arange(0, I, 3), 20)
                m.similar_users(np.arange(0, U, 3), 20, "dot")
                assert m.get_step() == step
        res.append(m.tables())
        m.close()
    for w in (L.MU, L.BU, L.BI, L.P, L.Q):
        assert np.array_equal(bits(res[0][w]), bits(res[1][w])), w


@pytest.mark.parametrize("D", W.TOPK)
def test_plan_lds_fits_a_cu(D):
    for k in (1, 10, 128, 129, 256):
        for n, cand in ((1, 1), (300, 300), (3706, 3706), (10677, 10677), (1 << 20, 1 << 20)):
            p = T.neighbours.plan(D, k, n, cand)
            assert 0 < p["lds_bytes"] <= LDS_PER_CU, (D, k, n, cand, p)
