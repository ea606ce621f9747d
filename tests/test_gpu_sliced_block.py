"""The shared scoring block (csrc/score_tile.h sliced_topk_block) and the slice merge (csrc/topk.hip k_topk_merge) on the
device, bit for bit against the contract, at the shapes where the block runs many rounds, compacts its queues mid-stream,
filters by a raised threshold, meets empty and short slices and merges up to 256 lists.

The cases are tests/sliced_cases.py: every score is exact in f32, so ids are compared with array_equal and scores as uint32.
tests/test_sliced_block_ref_host.py shows on the CPU which paths each case takes and that the case list reaches all of them;
here the plan the library reports is held to the one those claims were derived from."""
import ctypes as C

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import sliced_block_ref as M
from tests import sliced_cases as SC
from tests import svdpp_ref
from tests.neighbours_ref import neighbours_ref, pow4_table

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same(got, want, what):
    (gi, gs), (wi, ws) = got, want
    if not np.array_equal(gi, wi):
        r = int(np.flatnonzero((gi != wi).any(1))[0])
        q = int(np.flatnonzero(gi[r] != wi[r])[0])
        raise AssertionError("%s: ids differ in %d rows, first at row %d place %d: got %d (%r), want %d (%r)" % (
            what, int((gi != wi).any(1).sum()), r, q, gi[r, q], gs[r, q], wi[r, q], ws[r, q]))
    assert np.array_equal(bits(gs), bits(ws)), what + ": score bits differ"


def library_plan(fn, D, k, n, cand):
    lds, upb, sl, ch = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
    L.check(fn(D, k, n, cand, C.byref(lds), C.byref(upb), C.byref(sl), C.byref(ch)))
    return dict(upb=upb.value, slices=sl.value, chunk=ch.value, lds=lds.value)


def check_plan(c, fn=None, n_rows=None):
    """the library's plan is the restated one, and gives the slices and rounds the case claims"""
    n = c.n_rows if n_rows is None else n_rows
    got = library_plan(fn or L.load().tfr_topk_plan, c.D, c.k, n, c.I)
    p = c.plan(n)
    assert got == dict(upb=p["upb"], slices=p["slices"], chunk=p["chunk"], lds=max(p["lds_score"], p["lds_merge"])), (got, p)
    assert p["slices"] == c.slices and M.rounds_per_slice(p, 0, c.I) == c.claimed_rounds(), (c, p)
    assert n % p["upb"] != 0
    return p


def svd_model(c, Q=None):
    t = c.tables()
    m = T.SvdModel(SC.NU, c.I, c.D)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"] if Q is None else Q)
    return m


@pytest.mark.parametrize("c", SC.CASES, ids=repr)
def test_recommend(c):
    check_plan(c)
    m = svd_model(c)
    got = m.recommend(c.rows(), c.k, exclude=c.excl_csr())
    m.close()
    assert_same(got, c.expected(), c.name)


@pytest.mark.parametrize("c", SC.TALL + SC.WIDE, ids=repr)
def test_similar_items_dot(c):
    """the same block under the neighbour scorer: the candidate table is the pattern table with the users' one-feature rows
    put in as its queries, where the self mask meets them in a late round, after a compaction"""
    check_plan(c, L.load().tfr_neighbours_plan)
    m = svd_model(c, c.nb_table())
    got = m.similar_items(c.nb_queries(), c.k, "dot", exclude=c.excl_csr())
    m.close()
    wi, ws = c.nb_reference()
    assert_same(got, (wi[c.rows()], ws[c.rows()]), c.name)
    assert not np.any(got[0] == c.nb_queries()[:, None])


def test_similar_items_cosine_on_power_of_four_rows():
    """rows whose sum of squares is a power of four: the inverse norms are powers of two and the cosine is exact"""
    rs = np.random.RandomState(7)
    R, D, k, n = 1500, 16, 100, 8192 + 5
    p = M.topk_plan(k, n, R)
    assert library_plan(L.load().tfr_neighbours_plan, D, k, n, R)["slices"] == p["slices"] == 4
    assert M.rounds_per_slice(p, 0, R) == [3, 3, 3, 3]
    tab = pow4_table(rs, R, D)
    tab[rs.randint(0, R, 40)] = tab[rs.randint(0, R, 40)]  # exact ties, ordered by id alone
    distinct = rs.choice(R, 32, replace=False).astype(np.int32)
    rows = SC.BY_NAME["tall_k100_ragged"].rows()
    assert rows.size == n
    m = T.SvdModel(4, R, D)
    m.set_tables(np.float32(0), np.zeros(4, np.float32), np.zeros(R, np.float32), np.zeros((4, D), np.float32), tab)
    got = m.similar_items(distinct[rows], k, "cosine")
    m.close()
    wi, ws = neighbours_ref(tab, distinct, k, "cosine")
    assert_same(got, (wi[rows], ws[rows]), "cosine")


def test_fm_topk_over_an_offset_item_block():
    """FmModel.topk hands the block item tables that start inside V and W (37 rows in: no multiple of the 128-item round) and
    exclusions relative to that start"""
    c = SC.BY_NAME["wide_k128"]
    check_plan(c)
    t, lo = c.tables(), 37
    V = np.concatenate([t["P"], np.full((lo - SC.NU, c.D), 7.0, np.float32), t["Q"]])
    W = np.concatenate([t["bu"], np.full(lo - SC.NU, 9.0, np.float32), t["bi"]])
    with T.FmModel(lo + c.I, c.D) as fm:
        fm.set(float(t["mu"]), W, V)
        got = fm.topk(c.rows(), lo, lo + c.I, c.k, exclude=c.excl_csr())
    assert_same(got, c.expected(), c.name)


def test_svdpp_recommend():
    """the block on the effective user rows P[u] + z_u: even users get their whole row from four implicit items (z exact:
    1 / sqrt(4) times four rows of half the row), odd users have no implicit items"""
    c = SC.BY_NAME["wide_k256"]
    check_plan(c)
    t = c.tables()
    P, Y = t["P"].copy(), np.zeros((c.I, c.D), np.float32)
    sets = []
    for u in range(SC.NU):
        if u % 2 == 0:
            ids = np.arange(4 * u, 4 * u + 4)
            Y[ids] = 0.5 * P[u]
            P[u] = 0
            sets.append(ids)
        else:
            sets.append(np.zeros(0, np.int64))
    N = (np.concatenate([[0], np.cumsum([s.size for s in sets])]).astype(np.int64), np.concatenate(sets).astype(np.int32))
    z, _, _ = svdpp_ref.implicit_parts(Y.astype(np.float64), N[0], N[1], np.arange(SC.NU))
    assert np.array_equal(P.astype(np.float64) + z, t["P"].astype(np.float64))
    with T.SvdppModel(SC.NU, c.I, c.D) as pp:
        pp.set_implicit(N)
        pp.set_tables(t["mu"], t["bu"], t["bi"], P, t["Q"], Y)
        got = pp.recommend(c.rows(), c.k, exclude=c.excl_csr())
    assert_same(got, c.expected(), c.name)


def test_recommend_dev_chunks_its_exclusions():
    """65536 + 48 rows: two chunks.  The device entry hands the second chunk `indptr + 65536` with absolute offsets; the
    host entry rebases a copy.  Both equal the contract, and rows of the second chunk have exclusions that bite."""
    import torch
    c = SC.Case("two_chunks", "tall", 1500, 8, 10, 65536 + 48, 1, 12)
    p = check_plan(c)
    assert p["chunk"] == 65536 < c.n_rows
    rows, ex = c.rows(), c.excl_csr()
    want = c.expected()
    free = topk_free(c)
    second = np.arange(65536, c.n_rows)
    assert np.any(np.diff(ex[0])[second] > 0)
    assert any(not np.array_equal(want[0][r], free[rows[r]]) for r in second), "no exclusion bites in the second chunk"
    m = svd_model(c)
    host = m.recommend(rows, c.k, exclude=ex)
    dev = torch.device("cuda", 0)
    di, ds = m.recommend_dev(torch.from_numpy(np.array(rows)).to(dev), c.k,
                             exclude=(torch.from_numpy(ex[0]).to(dev), torch.from_numpy(ex[1]).to(dev)))
    m.sync()
    got_dev = (di.cpu().numpy(), ds.cpu().numpy())
    m.close()
    assert_same(host, want, "host entry")
    assert_same(got_dev, want, "device entry")


def topk_free(c):
    from tests.topk_ref import topk_ref
    return topk_ref(c.scores(), c.k)[0]


@pytest.mark.parametrize("name", ["wide_k128", "wide_k256_specials"])
def test_rank_of_every_recommended_item_is_its_place(name):
    """k_rank_count walks the same rounds and slices: the items recommend returned rank 0, 1, ..., in that order"""
    c = SC.BY_NAME[name]
    m = svd_model(c)
    rows, ex = c.rows(), c.excl_csr()
    items, _ = m.recommend(rows, c.k, exclude=ex)
    assert np.array_equal(items, c.expected()[0])
    n = (items >= 0).sum(1)
    assert np.all((items >= 0) == (np.arange(c.k)[None, :] < n[:, None]))
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ranks = m.rank_items(rows, (indptr, items[items >= 0].astype(np.int32)), exclude=ex)
    m.close()
    assert n.max() == c.k and n.min() == 0
    assert np.array_equal(ranks, np.concatenate([np.arange(x) for x in n]).astype(np.int32))
