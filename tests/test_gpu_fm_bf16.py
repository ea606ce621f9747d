"""The FM served from its bf16 snapshot, on the device: the conversion bit for bit, the forward (host CSR, device CSR and the
resident stores) per row against float64 on the round-tripped V, exact cases bit for bit against the float32 forward, the
quantisation statement against the float32 forward, the binary metrics, top-K on exact tables, and what moves the snapshot.

Inputs, the kernel's lane geometry and the bounds are those of tests/fm_bf16_cases.py, shown on the CPU in
tests/test_fm_bf16_host.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import bf16
from tests import fm_bf16_cases as C
from tests import fm_cases
from tests import fm_ref as FR
from tests.topk_ref import svd_scores, topk_ref

pytestmark = pytest.mark.gpu


def fm_from(D, mu, Wt, V, **kw):
    m = T.FmModel(V.shape[0], D, **kw)
    m.set(mu, Wt, V)
    return m


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def forward_dev(m, indptr, indices, data, entry="forward_bf16_dev"):
    import torch
    n = indptr.size - 1
    dp, di, dx = (torch.from_numpy(np.array(a)).cuda() for a in (indptr, indices, data))      # (the cases are read-only)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    getattr(m, entry)(dp.data_ptr(), di.data_ptr(), dx.data_ptr(), n, out.data_ptr())
    m.sync()
    return out.cpu().numpy()


def sub_csr(indptr, indices, data, rows):
    lens = (indptr[1:] - indptr[:-1])[rows]
    sel = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64), indices[sel.astype(np.int64)], data[sel.astype(np.int64)]


# ---------------------------------------------------------------- 1. conversion
@pytest.mark.parametrize("D", C.WIDTHS)
def test_conversion_is_pack_rows_bit_for_bit(D):
    mu, Wt, V = C.tables(D)
    V = V.copy()
    V[0, 0], V[1, D - 1] = -0.0, np.inf
    V[2, 0], V[3, 0] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8        # ties: to the even neighbour below, and above
    V[4, D - 1] = 1e-40                                        # a subnormal
    with fm_from(D, mu, Wt, V) as m:
        m.snapshot_bf16()
        got = m.bf16_rows()
    want = bf16.pack_rows(V)
    assert got.dtype == np.uint16 and got.shape == want.shape == (C.F, bf16.row_stride(D))
    assert np.array_equal(got, want)
    assert want[2, 0] == 0x3F80 and want[3, 0] == 0x3F82 and not want[:, D:].any()


# ---------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("D", C.WIDTHS)
def test_forward_holds_per_row_on_round_tripped_rows_in_every_entry_and_load_form(D, monkeypatch):
    mu, Wt, V = C.tables(D)
    indptr, indices, data = C.design()
    x = fm_cases.as_csr((indptr, indices, data), C.F)
    with fm_from(D, mu, Wt, V) as m:
        m.snapshot_bf16()
        y = {}
        for ntv in ("0", "1"):
            monkeypatch.setenv("TFR_FM_BF16_NTV", ntv)
            y[ntv] = m.forward_csr_bf16(indptr, indices, data)
        monkeypatch.delenv("TFR_FM_BF16_NTV")
        again = m.forward_csr_bf16(indptr, indices, data)
        via_scipy = m.fma_bf16(x)
        dev = forward_dev(m, indptr, indices, data)
        m.upload_rows(x, np.zeros(C.N, np.float32), "eval")
        resident = m.predict_resident_bf16("eval")
        alone = {r: m.forward_csr_bf16(*sub_csr(indptr, indices, data, [r])) for r in (0, 1, 7, 8, 500, C.N - 1)}
    assert y["0"].dtype == np.float32 and y["0"].shape == (C.N,)
    assert same_bits(y["0"], y["1"]) and same_bits(y["0"], again) and same_bits(y["0"], via_scipy)
    assert same_bits(y["0"], dev) and same_bits(y["0"], resident)
    for r, got in alone.items():
        assert same_bits(got, y["0"][r:r + 1]), r
    rep = {}
    bad = FR.forward_excess(y["0"], mu, Wt, bf16.round_trip(V), indptr, indices, data, report=rep)
    print("RATIO bf16 forward D%d dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
        D, rep["forward"]["dev"]["short"], rep["forward"]["dev"]["long"], rep["forward"]["c_ref"]["short"], rep["forward"]["c_ref"]["long"]))
    assert not bad, bad
    assert y["0"][0] == mu                                   # the empty row


@pytest.mark.parametrize("D", [5, 256])
def test_rows_past_one_grid_pass(D):
    """more rows than the launch's blocks own: the rows of the second pass, and the last block's spare groups"""
    G = C.lanes(D)
    indptr, indices, data = C.stride_design(G)
    n = indptr.size - 1
    rs = np.random.RandomState(D)
    Wt, V = rs.normal(0, 0.1, 40).astype(np.float32), rs.normal(0, 0.1, (40, D)).astype(np.float32)
    mu = np.float32(-0.3)
    first_pass = C.GRID_CAP * (256 // G)
    assert n > first_pass
    rows = np.concatenate([np.arange(50), np.sort(rs.choice(np.arange(50, first_pass), 1500, replace=False)), np.arange(first_pass - 20, n)])
    sub = sub_csr(indptr, indices, data, rows)
    with fm_from(D, mu, Wt, V) as m:
        m.snapshot_bf16()
        y = m.forward_csr_bf16(indptr, indices, data)
        ys = m.forward_csr_bf16(*sub)
    assert y.shape == (n,) and same_bits(y[rows], ys)
    bad = FR.forward_excess(ys, mu, Wt, bf16.round_trip(V), *sub)
    assert not bad, bad


# ---------------------------------------------------------------- 3. exactness
@pytest.mark.parametrize("D", C.WIDTHS)
def test_snapshot_and_float32_forwards_agree_bit_for_bit_where_everything_is_exact(D):
    mu, Wt, V = C.dyadic_model(D)
    indptr, indices, data = C.dyadic_design()
    assert C.dyadic_faults(mu, Wt, V, indptr, indices, data) == []
    with fm_from(D, mu, Wt, V) as m:
        m.snapshot_bf16()
        y32 = m.forward_csr(indptr, indices, data)
        y16 = m.forward_csr_bf16(indptr, indices, data)
    assert same_bits(y16, y32)
    assert np.array_equal(y16.astype(np.float64), FR.forward_terms(mu, Wt, V, indptr, indices, data)["y"])


# ---------------------------------------------------------------- 4. quantisation
@pytest.mark.parametrize("D", C.WIDTHS)
def test_snapshot_predictions_stay_within_the_quantisation_bound_of_the_float32_ones(D):
    mu, Wt, V = C.tables(D)
    indptr, indices, data = C.design()
    with fm_from(D, mu, Wt, V) as m:
        m.snapshot_bf16()
        y32 = m.forward_csr(indptr, indices, data)
        y16 = m.forward_csr_bf16(indptr, indices, data)
    first, second = C.quantisation_bound(mu, Wt, V, indptr, indices, data)
    f32 = (C.float32_allowance(mu, Wt, V, indptr, indices, data)
           + C.float32_allowance(mu, Wt, bf16.round_trip(V), indptr, indices, data))
    diff = np.abs(y16.astype(np.float64) - y32.astype(np.float64))
    moved = first > 0
    print("QUANT D%d device: max |bf16 - f32| / first term %.3f; float32 allowance / first term, median %.3f" % (
        D, (diff[moved] / first[moved]).max(), np.median(f32[moved] / first[moved])))
    assert np.all(diff <= first + second + f32), np.flatnonzero(diff > first + second + f32)[:10]
    assert diff.max() > 0


# ---------------------------------------------------------------- 5. metrics
class _FromSnapshot(object):
    """the two calls tests/test_gpu_fm_fit.py's statement makes, answered from the snapshot"""

    def __init__(self, m):
        self.eval_binary_resident, self.predict_resident = m.eval_binary_resident_bf16, m.predict_resident_bf16


def test_binary_metrics_of_the_eval_store_from_the_snapshot():
    from tests import fm_fit_ref
    from tests.test_gpu_fm_fit import _metrics_against_the_models_own_predictions as held
    x, y = fm_fit_ref.make_store(41, n=5000, positives=0.4)
    rs = np.random.RandomState(8)
    Wt, V = rs.normal(0, 0.5, fm_fit_ref.F).astype(np.float32), rs.normal(0, 0.3, (fm_fit_ref.F, 20)).astype(np.float32)
    with fm_from(20, -0.2, Wt, V, loss="nll") as m:
        m.snapshot_bf16()
        s = _FromSnapshot(m)
        m.upload_rows(x, y, "eval")
        got, lg = held(s, y)
        assert 0.0 < got["auc"] < 1.0
        assert same_bits(lg, m.fma_bf16(x))                                          # the resident forward is the forward
        assert not same_bits(lg, m.predict_resident("eval"))                         # and not the float32 one
        # heavy ties: every row the same, two labels
        lab = (np.arange(301) % 3 == 0).astype(np.float32)
        m.upload_rows(x[np.full(301, 12)], lab, "eval")
        got, lg = held(s, lab)
        assert np.all(lg == lg[0]) and got["auc"] == 0.5
        # two tied levels and an empty row, labels against the levels
        lab = (np.arange(150) % 2).astype(np.float32)
        m.upload_rows(x[np.array([12, 40, 0] * 50)], lab, "eval")
        held(s, lab)
        # one class only
        m.upload_rows(x[:200], np.ones(200, np.float32), "eval")
        held(s, np.ones(200, np.float32))
    with fm_from(20, -0.2, Wt, V, loss="mse") as m2:                                 # the regression model has no such metrics
        m2.snapshot_bf16()
        m2.upload_rows(x, y, "eval")
        with pytest.raises(T.TfrError) as e:
            m2.eval_binary_resident_bf16()
        assert e.value.code == L.ERR_STATE
        assert m2.predict_resident_bf16("eval").shape == (5000,)


# ---------------------------------------------------------------- 6. top-K
@pytest.mark.parametrize("D", C.TOPK_WIDTHS)
def test_topk_and_get_ranking_on_exact_tables(D):
    t = C.topk_tables(D)
    Un, In, mu, Wt, V = t["users"], t["items"], t["mu"], t["W"], t["V"]
    users = np.array([0, 7, 39, 7, 21], np.int32)
    excl_rows = [np.array([], np.int64), np.array([1, 5, 9]), np.arange(0, In, 2), np.array([499]), np.array([0])]
    ex = (np.concatenate(([0], np.cumsum([len(e) for e in excl_rows]))).astype(np.int64), np.concatenate(excl_rows).astype(np.int32))
    S = svd_scores(V[:Un], V[Un:], Wt[:Un], Wt[Un:], mu, users)
    with fm_from(D, mu, Wt, V) as m:
        m.snapshot_bf16()
        for k in (10, 256):
            items, scores = m.topk_bf16(users, Un, Un + In, k, exclude=ex)
            wi, ws = topk_ref(S, k, excl_rows)
            assert np.array_equal(items, wi) and same_bits(scores, ws), k
            assert same_bits(m.topk(users, Un, Un + In, k, exclude=ex)[1], ws)       # the float32 entry's, on exact tables
            only = m.topk_bf16(users, Un, Un + In, k, exclude=ex, return_scores=False)
            assert np.array_equal(only, wi)
        assert (wi[2] == -1).sum() == 256 - In // 2 and np.all(np.isneginf(ws[2][wi[2] == -1]))      # padding past the eligible
        gi, gs = m.get_ranking_bf16(7, Un, In, k=10)
        wi, ws = topk_ref(S[1:2], 10)
        assert np.array_equal(gi, wi[0]) and same_bits(gs, ws[0])
        # a narrower item block that starts inside the table: ids are relative to item_lo
        lo, hi = Un + 123, Un + 123 + 77
        items, scores = m.topk_bf16(users, lo, hi, 10)
        wi, ws = topk_ref(S[:, 123:200], 10)
        assert np.array_equal(items, wi) and same_bits(scores, ws)
        with pytest.raises(T.TfrError):
            m.topk_bf16(users, Un, Un + In + 1, 10)


# ---------------------------------------------------------------- 7. state
def _every_entry(m, indptr, indices, data, x):
    return {
        "forward_csr_bf16": lambda: m.forward_csr_bf16(indptr, indices, data),
        "forward_csr_bf16, no rows": lambda: m.forward_csr_bf16([0], [], []),
        "fma_bf16": lambda: m.fma_bf16(x),
        "forward_bf16_dev, no rows": lambda: m.forward_bf16_dev(None, None, None, 0, None),
        "predict_resident_bf16": lambda: m.predict_resident_bf16("eval"),
        "eval_binary_resident_bf16": lambda: m.eval_binary_resident_bf16(),
        "topk_bf16": lambda: m.topk_bf16([1, 2], 100, 300, 10),
        "topk_bf16, no users": lambda: m.topk_bf16(np.zeros(0, np.int32), 100, 300, 10),
        "get_ranking_bf16": lambda: m.get_ranking_bf16(3, 100, 200, 10),
        "bf16_rows": lambda: m.bf16_rows(),
    }


def _refused(m, indptr, indices, data, x):
    for name, call in _every_entry(m, indptr, indices, data, x).items():
        with pytest.raises(T.TfrError) as e:
            call()
        assert e.value.code == L.ERR_STATE and "tfr_fm_bf16_snapshot" in str(e.value), name


def test_snapshot_is_a_copy_that_only_a_snapshot_moves():
    D = 28
    mu, Wt, V = C.tables(D)
    indptr, indices, data = C.design()
    x = fm_cases.as_csr((indptr, indices, data), C.F)
    y = (np.arange(C.N) % 2).astype(np.float32)
    rs = np.random.RandomState(2)
    with fm_from(D, mu, Wt, V, loss="nll", optimizer="adam", lr=0.01) as m:
        m.upload_rows(x, y, "eval")
        m.upload_rows(x, y, "train")
        _refused(m, indptr, indices, data, x)
        m.drop_bf16()                                        # nothing to drop: fine
        m.snapshot_bf16()
        assert m.sync() == 0.0                               # waits for the snapshot, which is no timed launch; the next call is sound

        def answers():
            return (m.forward_csr_bf16(indptr, indices, data), m.predict_resident_bf16("eval"), m.bf16_rows(),
                    m.eval_binary_resident_bf16(), m.topk_bf16([1, 2, 50], 100, 300, 10))

        def same(a, b):
            return (same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
                    and np.array_equal(a[4][0], b[4][0]) and same_bits(a[4][1], b[4][1]))
        a0 = answers()
        f32_before = m.forward_csr(indptr, indices, data)
        m.train_step(x, y)
        m.train_steps_resident(rs.randint(0, C.N, 128), 64)
        assert not same_bits(m.forward_csr(indptr, indices, data), f32_before)       # the tables moved
        assert same(answers(), a0)
        m.set(0.5, Wt[::-1].copy(), V[::-1].copy())
        assert same(answers(), a0)
        m.init(seed=3)
        assert same(answers(), a0)
        m.set(0.5, Wt[::-1].copy(), V[::-1].copy())
        m.snapshot_bf16()                                    # a second snapshot follows the tables
        a1 = answers()
        assert not same_bits(a1[0], a0[0]) and np.array_equal(a1[2], bf16.pack_rows(V[::-1]))
        assert not FR.forward_excess(a1[0], 0.5, Wt[::-1], bf16.round_trip(V[::-1]), indptr, indices, data)
        m.drop_bf16()
        _refused(m, indptr, indices, data, x)
        assert m.forward_csr(indptr, indices, data).shape == (C.N,)                  # the float32 entries do not need it


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_a_snapshot_leaves_the_float32_forward_and_training_bit_identical(optimizer):
    D = 36
    mu, Wt, V = C.tables(D)
    indptr, indices, data = C.design()
    x = fm_cases.as_csr((indptr, indices, data), C.F)
    y = (np.arange(C.N) % 2).astype(np.float32)
    ids = np.random.RandomState(4).randint(0, C.N, 3 * 64)
    out = []
    for snap in (False, True):
        with fm_from(D, mu, Wt, V, loss="nll", optimizer=optimizer, lr=0.01, reg=0.01) as m:
            m.upload_rows(x, y, "train")
            if snap:
                m.snapshot_bf16()
            got = [m.forward_csr(indptr, indices, data)]
            pred, loss = m.train_step(x, y)
            if snap:
                m.forward_csr_bf16(indptr, indices, data)    # a snapshot call between the steps
            losses = m.train_steps_resident(ids, 64)
            got += [pred, np.float32(loss), losses, m.forward_csr(indptr, indices, data), np.array(m.get_step(), np.float64)]
            slots = (0,) if optimizer == "sgd" else (0, L.SLOT_M, L.SLOT_V)
            got += [m.get_table(which | slot) for which in (L.MU, L.BU, L.P) for slot in slots]
            out.append(got)
    assert len(out[0]) == len(out[1])
    for k, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8)), k


def test_out_of_range_feature_raises_and_the_model_still_answers():
    D = 13
    mu, Wt, V = C.tables(D)
    indptr, indices, data = C.design()
    with fm_from(D, mu, Wt, V) as m:
        m.snapshot_bf16()
        want = m.forward_csr_bf16(indptr, indices, data)
        for bad_id in (C.F, -1, 2 ** 31 - 1):
            bad = indices.copy()
            bad[indptr[7] + 5] = bad_id                       # inside the long row
            with pytest.raises(T.OutOfRangeError):
                m.forward_csr_bf16(indptr, bad, data)
            assert same_bits(m.forward_csr_bf16(indptr, indices, data), want)
        x = sp.csr_matrix((data, indices, indptr), shape=(C.N, C.F))
        assert same_bits(m.fma_bf16(x), want)
