"""The FM trainer on the device: the minibatch gather against scipy's X[ids], resident steps against the host-fed step bit for
bit, the refusals, the binary metrics of resident predictions, and the five-fold driver.  Inputs: tests/fm_fit_ref.py.

tests/test_gpu_fm_step.py pins the step itself per row; the tests here pin that a resident step is that step."""
import json
import os

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import fm
from tests import fm_fit_ref as FR
from tests import widths as W

pytestmark = pytest.mark.gpu

SGD_LR, ADAM_LR, LAM = 2.0 ** -10, 0.002, 0.01            # the step tests' (tests/fm_cases.py)
PAIRS = (("nll", "sgd"), ("nll", "adam"), ("mse", "adam"))
WIDTHS = (13, 64, 252)                                     # a scalar-load width, a vector width, one above 128
assert set(WIDTHS) <= set(W.FM_STEP)
TABLES = (L.MU, L.BU, L.P)


def _tables(D, seed=0):
    rs = np.random.RandomState(seed)
    return (np.float32(0.1), rs.normal(0, 0.1, FR.F).astype(np.float32),
            rs.normal(0, 0.1 / np.sqrt(max(D, 16) / 16), (FR.F, D)).astype(np.float32))


def _model(D, loss="nll", opt="sgd"):
    m = T.FmModel(FR.F, D, loss=loss, optimizer=opt, lr=ADAM_LR if opt == "adam" else SGD_LR, reg=LAM)
    m.set(*_tables(D))
    return m


def _state(m, adam):
    out = {}
    for t in TABLES:
        out[t] = m.get_table(t)
        if adam:
            out[t | L.SLOT_M], out[t | L.SLOT_V] = m.get_table(t | L.SLOT_M), m.get_table(t | L.SLOT_V)
    return out


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "table %d differs" % k


def _train_targets(loss):
    x, y = FR.store("train")
    return x, (y if loss == "nll" else np.random.RandomState(2).normal(0, 1, FR.N).astype(np.float32))


# ----------------------------------------------------------------------------- the gather
@pytest.fixture(scope="module")
def stored():
    with T.FmModel(FR.F, 8) as m:
        for which in ("train", "eval"):
            m.upload_rows(*FR.store(which), which=which)
        yield m


@pytest.mark.parametrize("which", ["train", "eval"])
@pytest.mark.parametrize("name", sorted(FR.batches()))
def test_gather_equals_scipy_row_indexing(stored, name, which):
    ids = FR.batches()[name]
    x, y = FR.store(which)
    wx, wy = FR.gather_rows_ref(x, y, ids)
    gx, gy = stored.gather_rows(ids, which)
    assert gx.shape == wx.shape
    assert np.array_equal(gx.indptr, wx.indptr)
    assert np.array_equal(gx.indices, wx.indices)
    assert np.array_equal(gx.data.view(np.uint32), wx.data.view(np.uint32))
    assert np.array_equal(gy.view(np.uint32), wy.view(np.uint32))


# ----------------------------------------------------------------------------- resident steps are the host-fed step
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("loss,opt", PAIRS)
def test_resident_steps_equal_host_fed_steps_bit_for_bit(loss, opt, D):
    adam = opt == "adam"
    x, y = _train_targets(loss)
    ids, B = FR.train_ids(64), 64
    with _model(D, loss, opt) as res, _model(D, loss, opt) as host:
        res.upload_rows(x, y)
        got = res.train_steps_resident(ids, B)
        want = np.array([host.train_step(x[ids[s * B:(s + 1) * B]], y[ids[s * B:(s + 1) * B]])[1] for s in range(6)], np.float32)
        assert np.all(np.isfinite(want))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
        assert res.get_step() == host.get_step() and res.get_step()[0] == 6
        _assert_same_state(_state(res, adam), _state(host, adam))


@pytest.mark.parametrize("loss,opt", PAIRS)
def test_two_calls_of_three_steps_equal_one_call_of_six(loss, opt):
    adam = opt == "adam"
    x, y = _train_targets(loss)
    ids, B = FR.train_ids(64), 64
    with _model(64, loss, opt) as one, _model(64, loss, opt) as two:
        for m in (one, two):
            m.upload_rows(x, y)
        l6 = one.train_steps_resident(ids, B)
        assert two.train_steps_resident(ids[:3 * B], B, want_loss=False) is None      # queued, not waited for
        l3 = two.train_steps_resident(ids[3 * B:], B)
        assert np.array_equal(l6[3:].view(np.uint32), l3.view(np.uint32))
        assert one.get_step() == two.get_step()
        _assert_same_state(_state(one, adam), _state(two, adam))


# ----------------------------------------------------------------------------- refusals
def test_an_id_outside_the_store_is_refused_and_leaves_the_model_untouched():
    x, y = FR.store("train")
    ids = FR.train_ids(64).copy()
    with _model(64, "nll", "adam") as m:
        m.upload_rows(x, y)
        m.train_steps_resident(ids[:64], 64)
        before, step = _state(m, True), m.get_step()
        for bad in (FR.N, -1):
            ids[5 * 64 + 7] = bad                                                    # in the call's last step
            with pytest.raises(T.OutOfRangeError):
                m.train_steps_resident(ids, 64)
            with pytest.raises(T.OutOfRangeError):
                m.gather_rows(np.array([0, bad]))
        assert m.get_step() == step
        _assert_same_state(before, _state(m, True))


def test_a_second_upload_replaces_the_first():
    x, y = FR.store("train")
    x2, y2 = FR.make_store(99, n=300)
    ids = np.array([299, 0, 150, 299])
    with _model(16) as m:
        m.upload_rows(x, y)
        m.upload_rows(x2, y2)
        gx, gy = m.gather_rows(ids)
        wx, wy = FR.gather_rows_ref(x2, y2, ids)
        assert np.array_equal(gx.indptr, wx.indptr) and np.array_equal(gx.indices, wx.indices)
        assert np.array_equal(gx.data, wx.data) and np.array_equal(gy, wy)
        with pytest.raises(T.OutOfRangeError):
            m.train_steps_resident(np.array([300]), 1)                               # a row of the first store only
        with pytest.raises(T.TfrError):
            m.gather_rows(ids, "eval")                                               # the eval store was never uploaded


def test_calls_without_a_store_and_bad_stores_are_refused():
    x, y = FR.store("train")
    with _model(16) as m:
        step = m.get_step()
        for call in (lambda: m.train_steps_resident(np.arange(4), 4), lambda: m.gather_rows(np.arange(4)),
                     lambda: m.predict_resident("train"), lambda: m.eval_binary_resident()):
            with pytest.raises(T.TfrError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        indptr, indices = x.indptr.astype(np.int64), x.indices.astype(np.int32)

        def upload(ip, ix):
            return m._lib.tfr_fm_upload_rows(m._h, 0, L.ptr_i64(ip), L.ptr_i32(ix), L.ptr_f32(x.data), L.ptr_f32(y), FR.N)
        assert upload(indptr, np.where(indices == FR.F - 1, FR.F, indices).astype(np.int32)) == L.ERR_OOB   # one past the model's
        assert upload(indptr, np.where(indices == 0, -1, indices).astype(np.int32)) == L.ERR_OOB
        down = indptr.copy()
        down[10] = down[9] - 1                                                       # decreasing
        assert upload(down, indices) == L.ERR_ARG
        assert upload(indptr + 1, indices) == L.ERR_ARG                              # does not start at 0
        with pytest.raises(ValueError):
            m.upload_rows(x[:, :FR.F - 1], y)                                        # not the model's feature count
        with pytest.raises(T.TfrError):
            m.gather_rows(np.arange(4))                                              # the refused uploads left no store
        assert m.get_step() == step


# ----------------------------------------------------------------------------- metrics
def _metrics_against_the_models_own_predictions(m, y):
    from sklearn.metrics import roc_auc_score
    got = m.eval_binary_resident()
    lg = m.predict_resident("eval")
    n = y.size
    assert got["n"] == n and lg.shape == (n,)
    l64 = lg.astype(np.float64)
    acc = np.mean(np.round(1.0 / (1.0 + np.exp(-l64))) == y)
    nll = np.mean(np.maximum(l64, 0) - l64 * y + np.log1p(np.exp(-np.abs(l64))))
    print("METRICS n %d acc %.6f (numpy %.6f) nll %.9f (float64 %.9f) auc %.15f" % (n, got["acc"], acc, got["mean_nll"], nll, got["auc"]))
    assert abs(got["acc"] - acc) <= 2.0 / n                                          # a logit within rounding of 0 may flip
    assert abs(got["mean_nll"] - nll) <= 1e-5 * nll
    if 0 < y.sum() < n:
        assert abs(got["auc"] - roc_auc_score(y, l64)) <= 1e-12                      # same logits: exact rank arithmetic
    else:
        assert np.isnan(got["auc"])
    return got, lg


def test_binary_metrics_of_the_eval_store():
    x, y = FR.make_store(41, n=5000, positives=0.4)
    assert 0.37 < y.mean() < 0.43
    with T.FmModel(FR.F, 20, loss="nll") as m:
        rs = np.random.RandomState(8)
        m.set(-0.2, rs.normal(0, 0.5, FR.F).astype(np.float32), rs.normal(0, 0.3, (FR.F, 20)).astype(np.float32))
        m.upload_rows(x, y, "eval")
        got, lg = _metrics_against_the_models_own_predictions(m, y)
        assert 0.0 < got["auc"] < 1.0
        assert np.array_equal(lg.view(np.uint32), m.fma(x).view(np.uint32))          # the resident forward is the forward
        # heavy ties: every row the same, two labels
        row = x[np.full(301, 12)]
        lab = (np.arange(301) % 3 == 0).astype(np.float32)
        m.upload_rows(row, lab, "eval")
        got, lg = _metrics_against_the_models_own_predictions(m, lab)
        assert np.all(lg == lg[0]) and got["auc"] == 0.5
        # two tied levels and an empty row, labels against the levels
        m.upload_rows(x[np.array([12, 40, 0] * 50)], (np.arange(150) % 2).astype(np.float32), "eval")
        _metrics_against_the_models_own_predictions(m, (np.arange(150) % 2).astype(np.float32))
        # one class only
        m.upload_rows(x[:200], np.ones(200, np.float32), "eval")
        _metrics_against_the_models_own_predictions(m, np.ones(200, np.float32))
    with T.FmModel(FR.F, 20, loss="mse") as m2:                                      # the regression model has no such metrics
        m2.upload_rows(x, y, "eval")
        with pytest.raises(T.TfrError) as e:
            m2.eval_binary_resident()
        assert e.value.code == L.ERR_STATE
        assert m2.predict_resident("eval").shape == (5000,)


# ----------------------------------------------------------------------------- the driver
def test_five_fold_driver_writes_the_references_results_and_learns(tmp_path):
    from sklearn.metrics import roc_auc_score
    U, I, n = 150, 60, 6000
    rs = np.random.RandomState(12)
    pu, qi = rs.normal(0, 1, (U, 2)), rs.normal(0, 1, (I, 2))                        # a planted rank-2 logistic model
    bu, bi = rs.normal(0, 0.5, U), rs.normal(0, 1.5, I)
    user, item = rs.randint(0, U, n), rs.randint(0, I, n)
    logit = bu[user] + bi[item] + np.sum(pu[user] * qi[item], axis=1)
    df = {"user": user.astype(np.int32), "item": item.astype(np.int32),
          "outcome": (rs.rand(n) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)}
    kw = dict(d=4, batch=256, lr=0.05, reg=0.0, optimizer="adam", seed=3)
    folds = fm.run(df, U, I, ["users", "items"], num_iter=3, out_dir=str(tmp_path), **kw)
    untrained = fm.run(df, U, I, ["users", "items"], num_iter=0, **kw)               # initialised, not trained
    assert len(folds) == len(untrained) == 5
    seen = np.concatenate([f["test_rows"] for f in folds])
    assert np.array_equal(np.sort(seen), np.arange(n))                               # every event is tested once
    for k, f in enumerate(folds):
        res = json.load(open(os.path.join(str(tmp_path), str(k), "results.json")))
        assert sorted(res) == ["args", "legends", "metrics"]
        assert sorted(res["legends"]) == ["full", "latex", "short"] and res["legends"]["short"] == "ui4"
        assert sorted(res["metrics"]) == ["ACC", "AUC", "NLL"] and res["args"]["d"] == 4
        assert res["metrics"] == f["metrics"]
        assert np.array_equal(f["y"], df["outcome"][f["test_rows"]])
        assert not set(user[f["test_rows"]]) & set(np.delete(user, f["test_rows"]))  # split by user
        assert abs(f["metrics"]["AUC"] - roc_auc_score(f["y"], f["pred"].astype(np.float64))) <= 1e-12
        assert f["loss"].shape == (3 * ((n - f["test_rows"].size) // 256),) and np.all(np.isfinite(f["loss"]))
        assert untrained[k]["loss"].size == 0
    auc, auc0 = np.mean([f["metrics"]["AUC"] for f in folds]), np.mean([f["metrics"]["AUC"] for f in untrained])
    print("DRIVER mean AUC trained %.4f, initialised only %.4f" % (auc, auc0))
    assert auc > auc0
