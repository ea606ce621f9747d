"""Folding new users and items into an implicit ALS on the device (tfr_ials_fold_in, tfr_ials_export_f32 through
ImplicitALS.fold_in_* / partial_fit_* / recommend_lists) on the cases of tests/ials_fold_cases.py: the half-sweep's own bits for
lists the model holds, the longdouble references for lists it has never seen, what a fold-in writes and what it must leave
alone, the Gram tag after every call that touches the Gram or a table, the float32 export bit for bit, top-K for guests, and
the refusals."""
import ctypes as C_

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import ials_cases as C0
from tests import ials_cg_ref as G
from tests import ials_fold_cases as F
from tests import ials_ref as R

pytestmark = pytest.mark.gpu

TAG_CASES = ("fold-chol-d17-chunk32", "fold-cg3-d33-chunk32")


def _open(case, load=True, X=None, Y=None):
    kw = dict(solver="cg", cg_steps=case["steps"]) if case["steps"] else {}
    m = T.ImplicitALS(case["nu"], case["ni"], factors=case["d"], regularization=case["lam"], alpha=case["alpha"],
                      chunk=case["chunk"], **kw)
    m.set_factors(case["X"] if X is None else X, case["Y"] if Y is None else Y)
    if load:
        m.load(C0.csr(case))
    return m


def _both(m):
    return m.user_factors, m.item_factors


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _fold(m, side, lst, start=None):
    return (m.fold_in_users, m.fold_in_items)[side](F.csr(lst), start=start)


def _partial_fit(m, side, ids, lst):
    (m.partial_fit_users, m.partial_fit_items)[side](ids, F.csr(lst))


def _subset(case, side):
    """a permuted subset of side's entities with an empty list, every chunked one and ten others"""
    N = np.diff(R.lists(case, side)[0])
    rs = np.random.RandomState(11 + side)
    rest = rs.choice(np.flatnonzero((N > 0) & (N <= case["chunk"])), 10, replace=False)
    return rs.permutation(np.concatenate((np.flatnonzero(N == 0)[:1], np.flatnonzero(N > case["chunk"]), rest)))


# ----------------------------------------------------------------------------- 1. the half-sweep's own bits
@pytest.mark.parametrize("case", F.CHOL_CASES + F.CG_CASES, ids=lambda c: c["id"])
def test_the_stored_lists_fold_in_to_the_rows_the_half_sweep_writes(case):
    for side in (0, 1):
        sub = _subset(case, side)
        lst = F.take(R.lists(case, side), sub)
        N = np.diff(lst[0])
        assert (N == 0).any() and (N > case["chunk"]).any()
        with _open(case) as m:
            before = _both(m)
            got = _fold(m, side, lst, start=before[side][sub] if case["steps"] else None)
            assert _same(_both(m), before), "%s: a fold-in without rows wrote a table" % case["id"]
            m.half_sweep(side)
            after = _both(m)
            assert not _same((after[side][sub],), (before[side][sub],))
            assert got.tobytes() == after[side][sub].tobytes(), "%s, side %d: not the half-sweep's bits" % (case["id"], side)
            assert (got[N == 0] == 0).all()


# ----------------------------------------------------------------------------- 2. lists the model has never seen
@pytest.mark.parametrize("case", F.CHOL_CASES, ids=lambda c: c["id"])
def test_unseen_lists_against_the_longdouble_half(case):
    """before any load: a model that was only set can serve"""
    bad = []
    for side in (0, 1):
        other = (case["Y"], case["X"])[side]
        lst = case["new"][side]
        with _open(case, load=False) as m:
            got = _fold(m, side, lst)
            again = _fold(m, side, lst)
            Gd = m.gram(1 - side)
            assert _same(_both(m), (case["X"], case["Y"]))
        assert got.tobytes() == again.tobytes()
        ref = R.half(other, lst, case["lam"], case["alpha"], G=Gd)
        print("RATIO %s side %d: %.3f of K = %d" % (case["id"], side, float(R.ratios(ref, got).max()), R.K))
        bad += R.check_half(ref, got, R.K, "%s side %d" % (case["id"], side))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", F.CG_CASES + [F.CONV_CASE], ids=lambda c: c["id"])
def test_unseen_lists_against_the_longdouble_iterate_from_the_given_start(case):
    """K_CG against the iterate at the same steps; the 3 d-step case K_CONV against the exact minimiser"""
    bad = []
    conv = case["id"].startswith("fold-conv")
    k = G.K_CONV if conv else G.K_CG
    for side in (0, 1):
        other = (case["Y"], case["X"])[side]
        lst = case["new"][side]
        with _open(case, load=False) as m:
            got = {"zero": _fold(m, side, lst), "given": _fold(m, side, lst, start=case["start"][side])}
            Gd = m.gram(1 - side)
            assert _same(_both(m), (case["X"], case["Y"]))
        cond = G.conds(other, lst, case["lam"], case["alpha"], Gd)
        exact = R.half(other, lst, case["lam"], case["alpha"], G=Gd) if conv else None
        for name, start in (("zero", np.zeros_like(case["start"][side])), ("given", case["start"][side])):
            ref = G.against_exact(start, exact) if conv else G.cg_half(start, other, lst, case["lam"], case["alpha"], case["steps"],
                                                                       G=Gd, cond=cond)
            what = "%s side %d start %s" % (case["id"], side, name)
            print("RATIO %s: %.3f of %d" % (what, float(R.ratios(ref, got[name]).max()), k))
            assert np.isfinite(got[name]).all(), what
            bad += R.check_half(ref, got[name], k, what)
        assert got["zero"].tobytes() != got["given"].tobytes() or conv
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------- 3. partial_fit_*
@pytest.mark.parametrize("cid", ["fold-chol-d33-chunk32", "fold-chol-d64-chunk64", "fold-cg3-d128-chunk32"])
def test_partial_fit_writes_the_named_rows_and_nothing_else(cid):
    case = F.BY_ID[cid]
    for side in (0, 1):
        lst = case["new"][side]
        n = lst[0].size - 1
        ids = np.random.RandomState(5 + side).permutation((case["nu"], case["ni"])[side])[:n]
        with _open(case) as m:
            before = _both(m)
            # a conjugate-gradient handle starts partial_fit from the rows as they stand: the same start, spelled out
            want = _fold(m, side, lst, start=before[side][ids] if case["steps"] else None)
            _partial_fit(m, side, ids, lst)
            now = _both(m)
            assert now[side][ids].tobytes() == want.tobytes(), "%s side %d: the named rows are not fold_in's" % (cid, side)
            keep = np.setdiff1d(np.arange(before[side].shape[0]), ids)
            assert now[side][keep].tobytes() == before[side][keep].tobytes(), "%s side %d: another row moved" % (cid, side)
            assert now[1 - side].tobytes() == before[1 - side].tobytes(), "%s side %d: the partner table moved" % (cid, side)
            assert not _same(now, before)
            m.sweep(1)
            with _open(case, X=now[0], Y=now[1]) as twin:
                twin.sweep(1)
                assert _same(_both(m), _both(twin)), "%s side %d: the sweep after a partial_fit is not the twin's" % (cid, side)
            with pytest.raises(ValueError):
                _partial_fit(m, side, np.concatenate((ids[:-1], ids[:1])), lst)


# ----------------------------------------------------------------------------- 4. a fold-in changes nothing else
@pytest.mark.parametrize("cid", ["fold-chol-d33-chunk32", "fold-chol-d17-chunk64", "fold-cg3-d33-chunk32"])
def test_a_fold_in_between_two_sweeps_changes_neither(cid):
    case = F.BY_ID[cid]
    with _open(case) as a, _open(case) as b:
        a.sweep(1)
        b.sweep(1)
        for side in (0, 1):                                # chunked lists included: their plan and partial sums are fold-in's own
            _fold(a, side, case["new"][side])
            _fold(a, side, F.take(R.lists(case, side), _subset(case, side)))
        assert _same(_both(a), _both(b))
        a.sweep(1)
        b.sweep(1)
        assert _same(_both(a), _both(b)), "%s: the sweep after a fold-in differs from the twin's" % cid


# ----------------------------------------------------------------------------- 5. the Gram tag
def _disturbances(case):
    rs = np.random.RandomState(77)
    X2, Y2 = rs.uniform(0.0, 1.0, case["X"].shape), rs.uniform(0.0, 1.0, case["Y"].shape)
    ids = [rs.permutation(n)[:case["new"][s][0].size - 1] for s, n in ((0, case["nu"]), (1, case["ni"]))]
    return [("set Y", lambda m: m.set_factors(Y=Y2)), ("set X", lambda m: m.set_factors(X=X2)),
            ("half 0", lambda m: m.half_sweep(0)), ("half 1", lambda m: m.half_sweep(1)),
            ("gram 0", lambda m: m.gram(0)), ("gram 1", lambda m: m.gram(1)), ("loss", lambda m: m.loss()),
            ("partial_fit_items", lambda m: _partial_fit(m, 1, ids[1], case["new"][1])),
            ("partial_fit_users", lambda m: _partial_fit(m, 0, ids[0], case["new"][0]))]


@pytest.mark.parametrize("cid", TAG_CASES)
@pytest.mark.parametrize("op", range(9), ids=lambda i: ["set-Y", "set-X", "half-0", "half-1", "gram-0", "gram-1", "loss",
                                                         "partial-fit-items", "partial-fit-users"][i])
def test_a_fold_in_after_anything_that_touches_the_gram_or_a_table_equals_a_fresh_model_s(cid, op):
    """the handle is left with the Gram of either table (a fold-in of either side first), then disturbed, then asked for a
    fold-in of either side: a Gram kept from before the disturbance would give other rows than a fresh model holding the
    same tables"""
    case = F.BY_ID[cid]
    name, disturb = _disturbances(case)[op]
    for first in (0, 1):
        for side in (0, 1):
            with _open(case) as m:
                earlier = _fold(m, first, case["new"][first])
                assert _fold(m, first, case["new"][first]).tobytes() == earlier.tobytes(), "the same fold-in twice differs"
                disturb(m)
                got = _fold(m, side, case["new"][side])
                X, Y = _both(m)
            with _open(case, load=False, X=X, Y=Y) as fresh:
                want = _fold(fresh, side, case["new"][side])
            assert got.tobytes() == want.tobytes(), "%s: after a fold-in of side %d and %s, side %d is not a fresh model's" % (
                cid, first, name, side)
            if name == ("set Y", "set X")[side] and first == side:
                # the reused Gram would have shown: the rows from the new partner table are other rows
                assert got.tobytes() != earlier.tobytes()


# ----------------------------------------------------------------------------- 6. export_f32
def _special_table(rs, n, d):
    """uniform values with, planted: exact halfway cases on both sides of an even and an odd float32, values that underflow
    to 0 (one of them the halfway case below the smallest subnormal), float32 subnormals (one a halfway case between two of
    them), values that overflow to infinity (one the halfway case above the largest float32), and a negative zero"""
    t = rs.uniform(-2.0, 2.0, (n, d))
    special = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 2.0 ** -24 - 2.0 ** -52,
               1e-50, -1e-50, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -40), 1e-40, -3e-42, 1.5 * 2.0 ** -149, 2.0 ** -149, 2.0 ** -126,
               1e39, -1e39, float(np.finfo(np.float32).max) + 2.0 ** 103, float(np.finfo(np.float32).max) + 2.0 ** 102,
               float(np.finfo(np.float32).max), -0.0]
    flat = t.reshape(-1)
    flat[rs.choice(flat.size, len(special), replace=False)] = special
    return t


def _export(m, which, lo, rows, d):
    import torch
    buf = torch.full(((rows + 2) * d,), -7.0, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    m._check(m._lib.tfr_ials_export_f32(m._h, which, lo, rows, buf.data_ptr() + 4 * d))
    out = buf.cpu().numpy().reshape(rows + 2, d)
    assert (out[0] == -7.0).all() and (out[-1] == -7.0).all(), "export wrote outside its window"
    return out[1:-1]


def test_export_f32_has_the_bits_of_numpy_s_cast():
    d, nu, ni = 5, 37, 23                                  # d is no multiple of 4; 185 and 115 elements: partly filled blocks
    rs = np.random.RandomState(3)
    X, Y = _special_table(rs, nu, d), _special_table(rs, ni, d)
    lib = L.load()
    with np.errstate(over="ignore"):
        want = [X.astype(np.float32), Y.astype(np.float32)]
    assert np.isinf(want[0]).sum() >= 3 and (want[0] == 0).sum() >= 4
    with T.ImplicitALS(nu, ni, factors=d) as m:
        m.set_factors(X, Y)
        for which, n in ((0, nu), (1, ni)):
            for lo, rows in ((0, n), (0, 3), (4, 9), (n - 6, 6), (n - 1, 1), (n, 0)):
                got = _export(m, which, lo, rows, d)
                assert got.tobytes() == want[which][lo:lo + rows].tobytes(), (which, lo, rows)
            for lo, rows in ((0, n + 1), (n, 1), (-1, 2), (3, -1)):
                assert lib.tfr_ials_export_f32(m._h, which, lo, rows, None) == L.ERR_ARG, (which, lo, rows)
        assert lib.tfr_ials_export_f32(m._h, 3, 0, 1, None) == L.ERR_ARG
        assert lib.tfr_ials_export_f32(m._h, 2, 0, 0, None) == L.ERR_STATE
        assert lib.tfr_ials_export_f32(m._h, 0, 0, 1, None) == L.ERR_ARG          # rows to write and nowhere to write them
    case = F.BY_ID["fold-chol-d17-chunk32"]
    with _open(case, load=False) as m:
        assert lib.tfr_ials_fold_in(m._h, 0, 0, L.ptr_i64(np.zeros(1, np.int64)), None, None, 0, None, None, None, None) == L.OK
        assert lib.tfr_ials_export_f32(m._h, 2, 0, 0, None) == L.ERR_STATE        # n = 0 was a no-op
        rows = _fold(m, 1, case["new"][1])
        n = rows.shape[0]
        for lo, cnt in ((0, n), (0, 2), (3, 5), (n - 4, 4)):
            assert _export(m, 2, lo, cnt, case["d"]).tobytes() == rows[lo:lo + cnt].astype(np.float32).tobytes(), (lo, cnt)
        assert lib.tfr_ials_export_f32(m._h, 2, 0, n + 1, None) == L.ERR_ARG
        short = F.take(case["new"][0], [3, 4])
        _fold(m, 0, short)
        assert lib.tfr_ials_export_f32(m._h, 2, 0, n, None) == L.ERR_ARG          # the window is the LAST fold-in's
        assert _export(m, 2, 0, 2, case["d"]).tobytes() == _fold(m, 0, short).astype(np.float32).tobytes()


# ----------------------------------------------------------------------------- 7. recommend_lists
@pytest.mark.parametrize("cid", ["fold-chol-d33-chunk32", "fold-chol-d64-chunk64", "fold-cg3-d128-chunk32"])
def test_recommend_lists_equals_a_model_set_on_the_host_to_the_folded_rows(cid):
    case = F.BY_ID[cid]
    lst = case["new"][0]
    lists = F.csr(lst)
    n = lists.shape[0]
    resident = np.arange(0, case["nu"], 7, dtype=np.int32)
    with _open(case) as m:
        rows = _fold(m, 0, lst)
        with T.SvdModel(n, case["ni"], case["d"]) as host:
            host.set_tables(np.float32(0.0), np.zeros(n, np.float32), np.zeros(case["ni"], np.float32), rows.astype(np.float32),
                            case["Y"].astype(np.float32))
            want = {(k, ex): host.recommend(np.arange(n, dtype=np.int32), k, exclude=lists if ex else None)
                    for k in (10, 200) for ex in (False, True)}
        with m.to_svd_model() as plain, pytest.raises(ValueError):
            m.recommend_lists(plain, lists)
        for guests in (5, n + 3):                          # more lists than guest rows: slices of 5, 5 and 3; and all at once
            with m.to_svd_model(extra_users=guests) as svd:
                assert svd.user_num == case["nu"] + guests
                P = svd.tables()[L.P]
                assert P[:case["nu"]].tobytes() == case["X"].astype(np.float32).tobytes() and (P[case["nu"]:] == 0).all()
                before = svd.recommend(resident, 10, exclude=C0.csr(case))
                for (k, ex), (wi, ws) in want.items():
                    gi, gs = m.recommend_lists(svd, lists, k=k, exclude=ex)
                    assert gi.tobytes() == wi.tobytes() and gs.tobytes() == ws.tobytes(), (cid, guests, k, ex)
                    assert m.recommend_lists(svd, lists, k=k, exclude=ex, return_scores=False).tobytes() == wi.tobytes()
                    if ex:
                        assert not any(set(gi[e]) & set(lst[1][lst[0][e]:lst[0][e + 1]]) for e in range(n))
                after = svd.recommend(resident, 10, exclude=C0.csr(case))
                assert _same(before, after), "%s: guests changed what resident users are recommended" % cid
        assert _same(_both(m), (case["X"], case["Y"]))


# ----------------------------------------------------------------------------- 8. refusals
def _call(m, side, ptr, ids, vals, chunk=0, rows=None, start=None, n=None):
    f64 = lambda a: None if a is None else a.ctypes.data_as(L._f64p)
    out = np.full(((ptr.size - 1 if n is None else max(n, 0)) * m.factors,), 7.0)
    keep = [np.ascontiguousarray(ptr, np.int64), np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64),
            None if rows is None else np.ascontiguousarray(rows, np.int32), None if start is None else np.ascontiguousarray(start, np.float64)]
    rc = m._lib.tfr_ials_fold_in(m._h, side, ptr.size - 1 if n is None else n, L.ptr_i64(keep[0]), L.ptr_i32(keep[1]), f64(keep[2]),
                                 chunk, None if keep[3] is None else L.ptr_i32(keep[3]), f64(keep[4]), f64(out), None)
    assert rc == L.OK or (out == 7.0).all(), "a refused fold-in wrote its output"
    return rc


@pytest.mark.parametrize("cid", ["fold-chol-d17-chunk32", "fold-cg3-d33-chunk32"])
def test_every_refusal_gives_its_code_and_leaves_the_model_as_it_was(cid):
    case = F.BY_ID[cid]
    ptr, ids, vals, _ = case["new"][0]
    n, d, nu, ni = ptr.size - 1, case["d"], case["nu"], case["ni"]
    k1 = int(ptr[1])                                       # the one entry of list 1
    k5 = int(ptr[5]) + 3                                   # inside list 5 (33 entries)
    rows = np.arange(n, dtype=np.int32)

    def changed(a, k, v):
        b = a.copy()
        b[k] = v
        return b

    swapped = ids.copy()
    swapped[k5], swapped[k5 + 1] = ids[k5 + 1], ids[k5]
    refusals = [
        ("side 2", L.ERR_ARG, dict(side=2)), ("side -1", L.ERR_ARG, dict(side=-1)),
        ("indptr[0] = 1", L.ERR_ARG, dict(ptr=changed(ptr, 0, 1))),
        ("indptr decreases", L.ERR_ARG, dict(ptr=changed(ptr, 6, ptr[5] - 1))),
        ("negative n", L.ERR_ARG, dict(n=-1)),
        ("unsorted list", L.ERR_ARG, dict(ids=swapped)),
        ("repeated id", L.ERR_ARG, dict(ids=changed(ids, k5 + 1, ids[k5]))),
        ("zero value", L.ERR_ARG, dict(vals=changed(vals, k5, 0.0))), ("negative value", L.ERR_ARG, dict(vals=changed(vals, k5, -1.0))),
        ("nan value", L.ERR_ARG, dict(vals=changed(vals, k1, np.nan))), ("inf value", L.ERR_ARG, dict(vals=changed(vals, k1, np.inf))),
        ("chunk 48", L.ERR_ARG, dict(chunk=48)), ("chunk -32", L.ERR_ARG, dict(chunk=-32)), ("chunk 16", L.ERR_ARG, dict(chunk=16)),
        ("duplicate rows", L.ERR_ARG, dict(rows=changed(rows, 4, rows[9]))), ("negative row", L.ERR_ARG, dict(rows=changed(rows, 2, -1))),
        ("row out of range", L.ERR_OOB, dict(rows=changed(rows, 2, nu))),
        ("id out of range", L.ERR_OOB, dict(ids=changed(ids, k1, ni))), ("negative id", L.ERR_OOB, dict(ids=changed(ids, k1, -1))),
    ]
    if not case["steps"]:
        refusals.append(("start on a Cholesky handle", L.ERR_ARG, dict(start=case["start"][0])))
    lib = L.load()
    with _open(case) as m, _open(case) as twin:
        assert lib.tfr_ials_fold_in(m._h, 0, n, None, L.ptr_i32(ids), m._p64(vals), 0, None, None, None, None) == L.ERR_ARG
        for name, code, kw in refusals:
            a = dict(side=0, ptr=ptr, ids=ids, vals=vals)
            a.update(kw)
            assert _call(m, **a) == code, "%s: expected %d" % (name, code)
            assert m._lib.tfr_ials_last_error()
            assert _same(_both(m), _both(twin)), "%s: a refused fold-in changed a table" % name
            m.sweep(1)
            twin.sweep(1)
            assert _same(_both(m), _both(twin)), "%s: the sweep after a refused fold-in is not the twin's" % name
        assert lib.tfr_ials_export_f32(m._h, 2, 0, 0, None) == L.ERR_STATE        # none of them counted as a fold-in
        assert _call(m, 0, ptr, ids, vals, n=0) == L.OK                            # n = 0: a no-op
        assert _call(m, 0, ptr, ids, vals, chunk=64, rows=rows) == L.OK            # and the call they all spoiled goes through
        assert not _same(_both(m), _both(twin))
