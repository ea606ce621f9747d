"""The ALS half-sweeps on the device, per entity (csrc/als_kernels.hip: k_als_partial, k_als_fit, k_als_predict), against
the longdouble reference of tests/als_step_ref.py on the cases of tests/als_cases.py: every count of live A-entry slots, both
staging forms, every tile and chunk edge, both grid-stride loops, the sweep sets and ill-conditioned normal equations.  The
two halves of a sweep are told apart: the user half is checked from the case's tables, the work half with the reference fed
the device's own U and W_user.  Then what must hold bit for bit: a repeat, three sweeps in one call or three calls, an
entity alone or in the crowd, a second load after a first."""
import ctypes as C_
import functools

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import als_cases as C
from tests import als_step_ref as S
from tests import widths as W

pytestmark = pytest.mark.gpu

assert {c["d"] for c in C.CASES if c["id"].startswith("tile_edges")} >= set(W.ALS_STEP)
ENV = "TFR_ALS_CHUNK"
BY_ID = {c["id"]: c for c in C.CASES}


def _tables(case):
    return dict(U=case["U"], V=case["V"], W_user=case["Wu"], W_work=case["Ww"], bias=case["bias"])


def _open(case):
    """a model holding the case's tables and bias; no ratings yet"""
    als = T.MangakiALS3(nb_components=case["d"], nb_iterations=1, lambda_=case["lam"], verbose=False)
    als.nb_users, als.nb_works = case["nu"], case["nw"]
    als.init_vars()
    als.load_state(_tables(case))
    return als


def _load(als, case, monkeypatch, rows=None):
    """tfr_als_load on the case's columns (or on ``rows`` of them) with TFR_ALS_CHUNK as the case wants it; the load sets
    bias = mean(y), so the case's bias is set again after it.  Returns the status of the load."""
    if case["ch"] is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, str(case["ch"]))
    u, w, y = (np.ascontiguousarray(case[k] if rows is None else case[k][rows]) for k in ("u", "w", "y"))
    rc = als._lib.tfr_als_load(als._h, L.ptr_i64(u), L.ptr_i64(w), als._p64(y), y.size)
    monkeypatch.delenv(ENV, raising=False)
    if rc == L.OK:
        als._check(als._lib.tfr_als_set_bias(als._h, case["bias"]))
    return rc


def _sweep(als, n=1):
    als._check(als._lib.tfr_als_sweep(als._h, n, None))
    return als.state()


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("U", "V", "W_user", "W_work"))


def _one_sweep(case, monkeypatch, rows=None):
    als = _open(case)
    try:
        assert _load(als, case, monkeypatch, rows) == L.OK
        return _sweep(als)
    finally:
        als.close()


def _check_case(case, monkeypatch):
    als = _open(case)
    try:
        assert _load(als, case, monkeypatch) == L.OK
        after = _sweep(als)
        report = {}
        bad = S.check_sweep(case, after, S.K, report)
        print("RATIO %s %s" % (case["id"], {k: "rho_x %.3f rho_w %.3f" % v for k, v in report.items()}))
        assert not bad, "\n".join(bad)
        als.load_state(_tables(case))                      # the same sweep again: the same bits
        assert _same(after, _sweep(als)), "%s: a second run from the same tables differs" % case["id"]
        return after
    finally:
        als.close()


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_one_sweep_per_entity_half_by_half(case, monkeypatch):
    _check_case(case, monkeypatch)


@pytest.mark.parametrize("swap", [False, True], ids=["as-given", "swapped"])
@pytest.mark.parametrize("ch,d", C.CHUNK_CASES)
def test_chunked_and_unchunked_loads_agree(ch, d, swap, monkeypatch):
    """the same ratings with TFR_ALS_CHUNK (lists cut into chunks) and without (nothing chunked at these lengths): the user
    half, which reads the same tables in both, agrees within the bound; the swapped orientation puts the work side's lists
    there"""
    cid = "chunk_edges-ch%d-d%d" % (ch, d)
    a, b = BY_ID[cid + ("-swapped" if swap else "")], BY_ID[cid + "-unchunked" + ("-swapped" if swap else "")]
    ra, rb = _one_sweep(a, monkeypatch), _one_sweep(b, monkeypatch)
    lists, users = S.sides(a)[0]
    assert S.n_chunks(lists, S.chunk_size(a["ch"])).sum() > 0 and S.n_chunks(lists, S.chunk_size(b["ch"])).sum() == 0
    ref = S.half_sweep(a["U"], a["Wu"], a["V"], a["Ww"], lists, users, a["bias"], a["lam"])
    dx, dw = S.bounds(ref, a["lam"], S.K)
    ex = np.abs(ra["U"][users] - rb["U"][users]).max(1)
    ew = np.abs(ra["W_user"][users] - rb["W_user"][users])
    print("chunked against unchunked: worst x %.3g, worst w %.3g of the bound" % ((ex / dx).max(), (ew / dw).max()))
    assert (ex <= dx).all() and (ew <= dw).all()
    chunked = users[S.n_chunks(lists, S.chunk_size(a["ch"]))[users] > 0]
    assert (ex[np.isin(users, chunked)] > 0).any(), "no chunked entity differs at all: was the variable read?"


# ----------------------------------------------------------------------------- the grid-stride loops
@functools.lru_cache(maxsize=None)
def _grid():
    return C.grid_stride()


def _rows_of_user(case, e):
    return np.flatnonzero(case["u"] == e)


def _check_alone(case, crowd, users, monkeypatch):
    """each of ``users`` fitted alone (only its ratings loaded; the same tables and bias) has the bits it has in the crowd"""
    for e in users:
        alone = _one_sweep(case, monkeypatch, _rows_of_user(case, e))
        assert alone["U"][e].tobytes() == crowd["U"][e].tobytes() and alone["W_user"][e] == crowd["W_user"][e], \
            "%s: user %d alone differs from itself in the crowd" % (case["id"], e)


@pytest.mark.parametrize("swap", [False, True], ids=["as-given", "swapped"])
def test_both_grid_stride_loops_run_a_second_entity(swap, monkeypatch):
    """more than 65 535 fitted entities on one side (k_als_fit's blocks each fit a second one) and more than 65 535 chunks
    on the other (k_als_partial's blocks each sum a second chunk); every entity is checked"""
    case = C.swapped(_grid()) if swap else _grid()
    (lu, users), (lw, works) = S.sides(case)
    cu, cw = S.n_chunks(lu, 32).sum(), S.n_chunks(lw, 32).sum()
    big, small = (works, users) if swap else (users, works)
    assert big.size > 65535 and (cu if swap else cw) > 65535 and small.size == 300
    crowd = _check_case(case, monkeypatch)
    if not swap:
        # user e and user e + 65 535 share a block of k_als_fit; user 5 + 65 535 comes second in it
        assert users[5] == 5 and users[5 + 65535] == 5 + 65535
        chunked = int(users[np.argmax(S.n_chunks(lu, 32)[users] >= 2)])
        _check_alone(case, crowd, [5, 5 + 65535, chunked], monkeypatch)
    else:
        # the chunks of the last user lie beyond the grid of k_als_partial: each is some block's second chunk
        first = np.cumsum(S.n_chunks(lu, 32)) - S.n_chunks(lu, 32)
        assert first[299] >= 65535
        _check_alone(case, crowd, [0, 299], monkeypatch)


# ----------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("cid", ["chunk_edges-ch32-d9", "tile_edges-d28-swapped", "sweep_sets"])
def test_three_sweeps_in_one_call_equal_three_calls(cid, monkeypatch):
    case = BY_ID[cid]
    als = _open(case)
    try:
        assert _load(als, case, monkeypatch) == L.OK
        once = _sweep(als, 3)
        als.load_state(_tables(case))
        for _ in range(3):
            thrice = _sweep(als, 1)
        assert _same(once, thrice)
        assert not _same(once, dict(_tables(case)))
    finally:
        als.close()


@pytest.mark.parametrize("cid,users", [("chunk_edges-ch64-d32", (0, 1, 4, 6)), ("chunk_edges-ch32-d9", (3, 4, 7)),
                                        ("tile_edges-d23", (4, 10, 12, 13)), ("tile_edges-d16-swapped", (3, 7, 500, 1099))])
def test_an_entity_alone_equals_itself_in_the_crowd(cid, users, monkeypatch):
    """short, tile-edge and chunked entities (at TFR_ALS_CHUNK and at the built-in chunk size)"""
    case = BY_ID[cid]
    lists, fitted = S.sides(case)[0]
    users = [e for e in users if e in fitted]
    assert len(users) >= 3
    if not cid.endswith("swapped"):
        assert any(S.n_chunks(lists, S.chunk_size(case["ch"]))[e] > 1 for e in users)
    _check_alone(case, _one_sweep(case, monkeypatch), users, monkeypatch)


def test_a_second_load_replaces_the_first(monkeypatch):
    """chunk_edges(32) loaded and swept, the tables restored, then tile_edges(9) loaded without the variable (no chunks on
    its work side, fewer on its user side, other list and sweep-set sizes): as if the first load had never been.  One model
    takes both loads, so both cases get tables of the larger of their sizes."""
    first, second = BY_ID["chunk_edges-ch32-d9"], BY_ID["tile_edges-d9"]
    assert first["d"] == second["d"]
    big = dict(first, nu=max(first["nu"], second["nu"]), nw=max(first["nw"], second["nw"]))
    rs = np.random.RandomState(77)
    tabs = dict(U=rs.rand(big["nu"], 9), V=rs.rand(big["nw"], 9), Wu=rs.rand(big["nu"]) / 2, Ww=rs.rand(big["nw"]) / 2)
    first, second = dict(big, **tabs), dict(second, nu=big["nu"], nw=big["nw"], **tabs)
    assert S.n_chunks(S.sides(first)[1][0], 32).sum() > 0 and S.n_chunks(S.sides(second)[1][0], S.CHUNK).sum() == 0
    fresh = _one_sweep(second, monkeypatch)
    als = _open(first)
    try:
        assert _load(als, first, monkeypatch) == L.OK
        moved = _sweep(als)
        als.load_state(_tables(second))
        assert _load(als, second, monkeypatch) == L.OK
        again = _sweep(als)
    finally:
        als.close()
    assert not _same(moved, fresh) and _same(again, fresh)
    assert not S.check_sweep(second, again, S.K)


# ----------------------------------------------------------------------------- predict
def test_predict_strides_over_more_pairs_than_its_grid(monkeypatch):
    """n = 4096 * 256 + 77: the first 77 threads of k_als_predict take a second pair"""
    rs = np.random.RandomState(9)
    nu, nw, d, n = 300, 200, 7, 4096 * 256 + 77
    case = dict(d=d, lam=0.1, bias=-0.75, nu=nu, nw=nw, U=rs.uniform(-1, 1, (nu, d)), V=rs.uniform(-1, 1, (nw, d)),
                Wu=rs.uniform(-1, 1, nu), Ww=rs.uniform(-1, 1, nw))
    u, w = rs.randint(0, nu, n), rs.randint(0, nw, n)
    als = _open(case)
    try:
        got = als.predict(np.stack([u, w], 1))
        none = als.predict(np.zeros((0, 2), np.int64))
    finally:
        als.close()
    assert none.shape == (0,) and got.shape == (n,)
    want, mag = S.predict(case["U"], case["V"], case["Wu"], case["Ww"], case["bias"], u, w)
    err = np.abs(got.astype(S.LD) - want).astype(np.float64)
    bound = (d + 3) * S.EPS * mag
    k = int(np.argmax(err / bound))
    assert (err <= bound).all(), "pair %d of %d: error %.3g, bound %.3g" % (k, n, err[k], bound[k])


# ----------------------------------------------------------------------------- errors
def test_errors_leave_the_model_as_it_was(monkeypatch):
    lib = L.load()
    for d in (0, 33):
        h = L._p()
        assert lib.tfr_als_create(C_.byref(h), 4, 4, d, 0.1, 0) == L.ERR_ARG and not h.value
    case = BY_ID["chunk_edges-ch32-d9"]
    want = _one_sweep(case, monkeypatch)
    als = _open(case)
    try:
        assert als._lib.tfr_als_sweep(als._h, 1, None) == L.ERR_STATE          # no ratings loaded yet
        assert _load(als, case, monkeypatch) == L.OK
        for col, size in (("u", case["nu"]), ("w", case["nw"])):
            wrong = dict(case, **{col: case[col].copy()})
            wrong[col][len(wrong[col]) // 2] = size                            # an id equal to the table size
            assert _load(als, wrong, monkeypatch) == L.ERR_OOB
        assert _same(_sweep(als), want)                                        # still the lists (and the bias) of the good load
    finally:
        als.close()
