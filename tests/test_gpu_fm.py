"""FM second-order forward (BASELINE config 5) through the C-ABI against the float64 oracle
(forward.py:21-22 generalised to count-valued features) and the committed golden rows."""
import numpy as np
import pytest
import scipy.sparse as sp

import tfrecomm_amd as T
from oracle import svd_oracle as so
from tests.util import assert_close
from tests import widths as W

pytestmark = pytest.mark.gpu


def test_fm_golden(golden):
    g = golden("fm_forward.npz")
    keys = sorted({k.split("/")[0] for k in g.files})
    assert len(keys) == 3
    for key in keys:
        V, W, mu = g[key + "/V"], g[key + "/W"], float(g[key + "/mu"])
        with T.FmModel(V.shape[0], V.shape[1]) as m:
            m.set(mu, W, V)
            y = m.forward_csr(g[key + "/indptr"], g[key + "/indices"], g[key + "/data"])
        assert y.dtype == np.float32
        assert_close(y, g[key + "/y"], what=key)
        assert abs(y[0] - mu) < 1e-6                      # the empty row predicts mu


@pytest.mark.parametrize("F,D,n,nnz", [(5000, 64, 3000, 8), (777, 15, 500, 3), (100000, 128, 4096, 12), (64, 4, 10, 64)])
def test_fm_random_csr_matches_oracle_and_scipy_path(F, D, n, nnz):
    _check_random_csr(F, D, n, nnz)


@pytest.mark.parametrize("D", W.FM)
def test_fm_random_csr_at_every_row_geometry(D):
    """k_fm_forward at every (G, VEC)"""
    _check_random_csr(300, D, 200, 6)


def _check_random_csr(F, D, n, nnz):
    rs = np.random.RandomState(F + D)
    V = rs.normal(0, 0.1, (F, D)).astype(np.float32)
    W = rs.normal(0, 0.1, F).astype(np.float32)
    mu = np.float32(0.37)
    X = sp.random(n, F, density=min(1.0, nnz / F), format="csr", random_state=rs,
                  data_rvs=lambda k: rs.randint(1, 4, k).astype(np.float64)).astype(np.float32)
    with T.FmModel(F, D) as m:
        m.set(mu, W, V)
        y = m.fma(X)                                       # forward.py's fma(x)
        y2 = m.fma(X.tocoo())
    want = so.fm_forward(np.float64(mu), W.astype(np.float64), V.astype(np.float64), X.indptr, X.indices,
                         X.data.astype(np.float64))
    assert_close(y, want, rtol=2e-5, what="fm")
    assert np.array_equal(y, y2)
    # on 0/1 features the reference's literal x.dot(V**2) form gives the same numbers
    Xb = X.copy()
    Xb.data[:] = 1.0
    with T.FmModel(F, D) as m:
        m.set(mu, W, V)
        yb = m.fma(Xb)
    ref = so.fm_forward_reference_form(np.float64(mu), W.astype(np.float64), V.astype(np.float64), Xb.indptr, Xb.indices,
                                       Xb.data.astype(np.float64))
    assert_close(yb, ref, rtol=2e-5, what="fm binary")


def test_fm_config5_full_size_properties():
    """BASELINE config 5 at its full table size (1M features x 64: V = 256 MB, read by the non-temporal variant of the
    kernel) on 2^18 rows x 8 non-zeros: a row's prediction depends on its own non-zeros only, so (i) 4096 rows drawn from
    the batch equal the oracle on those rows alone, (ii) the batch in another row order gives the same numbers, bit for
    bit, in that order, (iii) the empty row predicts mu."""
    F, D, n, nnz = 1_000_000, 64, 1 << 18, 8
    rs = np.random.RandomState(5)
    V = rs.normal(0, 0.1, (F, D)).astype(np.float32)
    W = rs.normal(0, 0.1, F).astype(np.float32)
    mu = np.float32(-0.21)
    indptr = np.arange(0, (n + 1) * nnz, nnz, dtype=np.int64)
    indptr[1:] -= nnz                                     # row 0 is empty
    indptr[0] = 0
    indices = rs.randint(0, F, (n - 1) * nnz).astype(np.int32)
    data = rs.randint(1, 4, (n - 1) * nnz).astype(np.float32)
    with T.FmModel(F, D) as m:
        m.set(mu, W, V)
        y = m.forward_csr(indptr, indices, data)
        pick = np.concatenate([[0], rs.choice(np.arange(1, n), 4095, replace=False)])
        sub_ptr = np.zeros(pick.size + 1, np.int64)
        sub_ptr[1:] = np.cumsum(indptr[pick + 1] - indptr[pick])
        sub_idx = np.concatenate([indices[indptr[r]:indptr[r + 1]] for r in pick])
        sub_val = np.concatenate([data[indptr[r]:indptr[r + 1]] for r in pick])
        want = so.fm_forward(np.float64(mu), W.astype(np.float64), V.astype(np.float64), sub_ptr, sub_idx, sub_val.astype(np.float64))
        assert_close(y[pick], want, rtol=2e-5, what="fm rows against the oracle")
        assert abs(y[0] - mu) < 1e-6
        perm = rs.permutation(n)
        X = sp.csr_matrix((data, indices, indptr), shape=(n, F))[perm]
        y2 = m.forward_csr(X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.float32))
        assert np.array_equal(y2, y[perm])


def test_fm_errors():
    with T.FmModel(100, 8) as m:
        m.init(seed=1)
        with pytest.raises(IndexError):
            m.forward_csr([0, 1], [100], [1.0])
        with pytest.raises(T.TfrError):
            m.forward_csr([0, 2, 1], [1, 2], [1.0, 1.0])
        assert m.forward_csr([0], [], []).shape == (0,)
        with pytest.raises(ValueError):
            m.fma(sp.identity(7, format="csr"))
    with pytest.raises(T.TfrError):
        T.FmModel(10, 300)


# ------------------------------------------------------------------ FM training
def _random_design(rs, n, F, nnz, hot=20):
    """CSR rows with a few very hot features (long runs in the backward) and an empty row."""
    rows, cols, vals = [], [], []
    for r in range(n):
        k = 0 if r == 3 else rs.randint(1, nnz + 1)
        picks = set(rs.randint(0, hot, k // 2 + 1).tolist()[:k]) | set(rs.randint(0, F, k).tolist())
        picks = sorted(picks)[:k]
        rows += [r] * len(picks)
        cols += picks
        vals += rs.randint(1, 4, len(picks)).tolist()
    return sp.csr_matrix((np.array(vals, np.float32), (rows, cols)), shape=(n, F))


@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("F,D,n,nnz", [(400, 16, 700, 6), (5000, 64, 3000, 8), (90, 5, 257, 4)])
def test_fm_training_matches_oracle(loss, optimizer, F, D, n, nnz):
    _check_training(loss, optimizer, F, D, n, nnz)


@pytest.mark.parametrize("D", W.FM)
def test_fm_training_at_every_row_geometry(D):
    """k_fm_forward (training form), the FM backward and its apply at every (G, VEC); loss and optimiser rotate"""
    x = W.FM.index(D)
    _check_training(("mse", "nll")[x % 2], ("sgd", "adam")[(x >> 1) % 2], 400, D, 700, 6)


def _check_training(loss, optimizer, F, D, n, nnz):
    rs = np.random.RandomState(F + n)
    V0 = rs.normal(0, 0.1, (F, D)).astype(np.float32)
    W0 = rs.normal(0, 0.1, F).astype(np.float32)
    mu0 = np.float32(0.1)
    # SGD: a rate at which the float64 reference stays at its initial scale (asserted below) - at 0.02 the mse trajectories
    # left it by orders of magnitude (and at 2^-10 the 3000-row one still does) and the scale-relative tolerances meant nothing.  Adam error scales with lr (sign-like
    # first steps)
    lr, lam = (2.0 ** -12, 0.01) if optimizer == "sgd" else (0.002, 0.01)
    V, W, mu = V0.astype(np.float64), W0.astype(np.float64), np.float64(mu0)
    state = so.fm_adam_state(F, D) if optimizer == "adam" else None
    with T.FmModel(F, D, loss=loss, optimizer=optimizer, lr=lr, reg=lam) as m:
        m.set(mu0, W0, V0)
        for s in range(3):
            X = _random_design(rs, n, F, nnz)
            y = (rs.rand(n) < 0.5).astype(np.float32) if loss == "nll" else rs.normal(0, 1, n).astype(np.float32)
            pred, lossv = m.train_step(X, y)
            want_pred, want_loss, mu = so.fm_train_step(mu, W, V, X.indptr, X.indices, X.data.astype(np.float64),
                                                        y.astype(np.float64), lr, lam, loss, optimizer, state)
            # hot features sum ~400 fp32 terms per step; Adam's normalisation amplifies their rounding
            tol = (1e-4 if optimizer == "adam" else 3e-5) * (s + 1)
            assert_close(pred, want_pred, rtol=tol, what="pred step %d" % s)
            assert_close(lossv, want_loss, rtol=tol, what="loss step %d" % s)
        gmu, gW, gV = m.get()
    # the condition under which the tolerances below see a wrong row: the reference did not diverge
    assert np.abs(V).max() <= 2 * np.abs(V0).max() and np.abs(W).max() <= 2 * np.abs(W0).max()
    assert_close(gV, V, rtol=4e-4, what="V")
    assert_close(gW, W, rtol=4e-4, what="W")
    assert abs(gmu - mu) <= 2e-4 * max(1.0, abs(mu))
    assert not np.array_equal(gV, V0)


def test_fm_training_is_deterministic_and_learns():
    rs = np.random.RandomState(1)
    F, D, n = 2000, 16, 4000
    Vt = rs.normal(0, 0.3, (F, 4))
    X = _random_design(rs, n, F, 6)
    logit = np.array([0.5 * ((X[r].toarray() @ Vt) ** 2).sum() - 1.0 for r in range(n)])
    y = (rs.rand(n) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    outs = []
    for rep in range(2):
        with T.FmModel(F, D, loss="nll", optimizer="adam", lr=0.05, reg=0.001) as m:
            m.init(seed=4, stddev=0.05)
            losses = [m.train_step(X, y)[1] for _ in range(30)]
            outs.append((losses, m.get()))
    assert outs[0][0] == outs[1][0]                                  # bit-identical run to run
    assert np.array_equal(outs[0][1][2], outs[1][1][2])
    assert outs[0][0][-1] < 0.8 * outs[0][0][0]                      # the data loss falls


_FM_LOAD_ROUNDS_SCRIPT = r"""
import hashlib, os, sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, %r)
import tfrecomm_amd as T
opt = os.environ["TFR_TEST_OPT"]
from tfrecomm_amd import _lib as L
F, n, nnz = 3000, 4000, 8
for D in (16, 32, 64, 128, 256):                           # every full-width geometry: G = 4, 8, 16, 32, 64
    rs = np.random.RandomState(7 + D)
    with T.FmModel(F, D, loss="nll", optimizer=opt, lr=0.02 if opt == "sgd" else 0.002, reg=0.01) as m:
        m.init(seed=3, stddev=0.05)
        h = hashlib.sha256()
        for s in range(3):
            cols = np.where(rs.rand(n, nnz) < 0.3, rs.randint(0, 12, (n, nnz)), rs.randint(0, F, (n, nnz)))      # hot features
            cols = np.sort(cols, axis=1)
            X = sp.csr_matrix((rs.rand(n * nnz).astype(np.float32) + 0.5, cols.reshape(-1), np.arange(n + 1) * nnz), shape=(n, F))
            y = (rs.rand(n) < 0.5).astype(np.float32)
            pred, loss = m.train_step(X, y)
            h.update(np.asarray(pred).tobytes()); h.update(np.float64(loss).tobytes())
        slots = (0,) if opt == "sgd" else (0, L.SLOT_M, L.SLOT_V)
        for which in (L.MU, L.BU, L.P):
            for slot in slots:
                h.update(np.ascontiguousarray(m.get_table(which | slot)).tobytes())
        print("HASH", D, h.hexdigest())
"""


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_fm_backward_three_round_load_form_is_bit_identical_to_the_general_form(optimizer):
    """TFR_FAST=0: the FM backward through the general form of k_seg_reduce; default: the three-round form (entry records),
    at every full-width geometry (D = 16, 32, 64, 128, 256).  Predictions, losses, mu, W, V and their Adam moments after three
    steps on rows with hot features hash identically."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = []
    for flag in ("1", "0"):
        env = dict(os.environ, TFR_FAST=flag, TFR_TEST_OPT=optimizer)
        p = subprocess.run([sys.executable, "-c", _FM_LOAD_ROUNDS_SCRIPT % root], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        out.append([l for l in p.stdout.decode().splitlines() if l.startswith("HASH")])
    assert len(out[0]) == 5 and out[0] == out[1]


# ------------------------------------------------------------------ the forward in every load form
_FM_VARIANT_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
import tfrecomm_amd as T
from tests import fm_cases as C
from tests import widths as W
out = {}
for D in W.FM_STEP:
    case = [c for c in C.CASES if c["kind"] == "edges" and c["D"] == D][0]
    t = C.tables_of(case)
    (indptr, indices, data), _ = C.batch_of(case, 0)
    with T.FmModel(case["F"], D) as m:
        m.set(t["mu"], t["W"], t["V"])
        out["D%%d" %% D] = m.forward_csr(indptr, indices, data)
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def forward_by_variant(tmp_path_factory):
    """the forward of every W.FM_STEP width on the row edges of tests/fm_cases.py, once per load form: the switch is read once
    per process, so each form runs in a fresh interpreter"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for variant in ("0", "2"):
        path = str(tmp_path_factory.mktemp("fmv") / ("variant%s.npz" % variant))
        p = subprocess.run([sys.executable, "-c", _FM_VARIANT_SCRIPT % root, path], env=dict(os.environ, TFR_FM_VARIANT=variant),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        out[variant] = dict(np.load(path))
    return out


@pytest.mark.parametrize("D", W.FM_STEP)
def test_fm_forward_load_forms_agree_and_hold_per_row(D, forward_by_variant):
    """k_fm_forward<G, VEC, false, false> and <..., true> (non-temporal V rows: unguarded 16-byte loads at full width, four
    scalar loads behind the guard for VEC = 4, one for VEC = 1) give identical bits, and every row - empty, one entry, 70
    entries, a column twice, an explicit zero - lies within limit x eps32 x X_r of float64"""
    from tests import fm_cases as C
    from tests import fm_ref as FR
    case = [c for c in C.CASES if c["kind"] == "edges" and c["D"] == D][0]
    t = C.tables_of(case)
    (indptr, indices, data), _ = C.batch_of(case, 0)
    y0, y2 = forward_by_variant["0"]["D%d" % D], forward_by_variant["2"]["D%d" % D]
    assert y0.dtype == np.float32 and y0.shape == (case["n"],)
    assert np.array_equal(y0.view(np.uint32), y2.view(np.uint32))
    rep = {}
    bad = FR.forward_excess(y0, t["mu"], t["W"], t["V"], indptr, indices, data, report=rep)
    print("RATIO forward D%d dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
        D, rep["forward"]["dev"]["short"], rep["forward"]["dev"]["long"], rep["forward"]["c_ref"]["short"], rep["forward"]["c_ref"]["long"]))
    assert not bad, bad


def test_fm_forward_streams_a_large_table_at_a_partial_width():
    """D = 100 (G = 32, VEC = 4, the last lanes past the row) with F just above 128 MiB / 400 B: the dispatch itself picks the
    non-temporal form, whose loads behind the guard are four scalar ones.  3000 rows drawn from the batch are held per row
    against float64 on those rows alone."""
    import os
    from tests import fm_ref as FR
    assert "TFR_FM_VARIANT" not in os.environ
    D, n = 100, 20000
    F = (128 << 20) // (4 * D) + 1
    assert F * D * 4 >= 128 << 20 > (F - 1) * D * 4
    rs = np.random.RandomState(11)
    rg = np.random.default_rng(11)                         # float32 draws: 34 M of them
    V = rg.standard_normal((F, D), dtype=np.float32) * np.float32(0.04)
    Wt = rg.standard_normal(F, dtype=np.float32) * np.float32(0.1)
    mu = np.float32(-0.21)
    lens = rs.randint(0, 10, n)
    lens[:3] = (0, 70, 1)
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    indices = rs.randint(0, F, indptr[-1]).astype(np.int32)
    indices[:2] = (F - 1, 0)
    data = np.where(rs.rand(indptr[-1]) < 0.33, rs.normal(0, 1, indptr[-1]), rs.randint(1, 4, indptr[-1])).astype(np.float32)
    with T.FmModel(F, D) as m:
        m.set(mu, Wt, V)
        y = m.forward_csr(indptr, indices, data)
    pick = np.concatenate([[0, 1, 2], 3 + rs.choice(n - 3, 2997, replace=False)])
    sub_ptr = np.concatenate(([0], np.cumsum(lens[pick]))).astype(np.int64)
    sel = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in pick])
    feats, inv = np.unique(indices[sel], return_inverse=True)          # the oracle on the rows' own features alone
    rep = {}
    bad = FR.forward_excess(y[pick], mu, Wt[feats], V[feats], sub_ptr, inv.astype(np.int32), data[sel], report=rep)
    print("RATIO forward nt-D100 dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
        rep["forward"]["dev"]["short"], rep["forward"]["dev"]["long"], rep["forward"]["c_ref"]["short"], rep["forward"]["c_ref"]["long"]))
    assert not bad, bad
    assert y[0] == mu
