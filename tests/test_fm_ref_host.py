"""The per-row FM step checks of tests/fm_ref.py, themselves tested on the CPU: the float64 sums agree with the FM oracle,
the float32 restatement stays inside the bound on every case of tests/fm_cases.py, a float32 NumPy stand-in for the device
(entries sorted by feature, summed in the reduce's pieces, lazy Adam or SGD applied) passes every check on every case, and
the same stand-in with one planted fault is rejected by a statement that names the table."""
import numpy as np
import pytest

from oracle import svd_oracle as so
from tests import fm_cases as C
from tests import fm_ref as FR
from tests import step_ref as R

F4 = np.float32


# ----------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", [c for c in C.CASES if c["n"] < 2000], ids=lambda c: c["id"])
def test_the_float64_sums_are_the_fm_oracles(case):
    """``fm_step_grads`` against ``so.fm_train_step`` (tests/test_fm_host.py ties that one to torch autograd): an SGD step
    of lr = 1 moves every table by its gradient"""
    t = C.tables_of(case)
    (indptr, indices, data), y = C.batch_of(case, 0)
    ref, terms = FR.fm_step_grads(t["mu"], t["W"], t["V"], indptr, indices, data, y, case["loss"], C.LAM)
    mu, W, V = np.float64(t["mu"]), t["W"].astype(np.float64), t["V"].astype(np.float64)
    W2, V2 = W.copy(), V.copy()
    yhat, lossv, mu2 = so.fm_train_step(mu, W2, V2, indptr, indices.astype(np.int64), data.astype(np.float64), y.astype(np.float64),
                                        1.0, C.LAM, case["loss"], so.SGD)
    assert np.abs(terms["y"] - yhat).max() <= 1e-12 and abs(terms["loss"][0] - lossv) <= 1e-12 * max(1.0, abs(lossv))
    for name, got in (("V", V - V2), ("W", W - W2), ("mu", mu - mu2)):
        scale = max(1.0, float(np.abs(ref[name][0]).max()))
        assert np.abs(ref[name][0] - got).max() <= 1e-12 * scale, name
    single = np.flatnonzero(np.diff(indptr) == 1)
    if single.size:                                       # a row of one entry: s_r - x V_j vanishes, E does not
        assert np.all(terms["S"][single] == data[indptr[single]].astype(np.float64)[:, None] * V[indices[indptr[single]]])


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_float32_restatement_stays_inside_the_bound(case):
    """as tests/test_step_ref_host.py holds the SVD one: a sequential float32 sum of n terms is off by at most n eps32
    sum |terms| beyond E, so c_ref is finite and at most 64 for the short class, the longest run for the long one"""
    t = C.tables_of(case)
    for s in range(2):
        (indptr, indices, data), y = C.batch_of(case, s)
        ref, terms = FR.fm_step_grads(t["mu"], t["W"], t["V"], indptr, indices, data, y, case["loss"], C.LAM)
        f32 = FR.f32_fm(t["mu"], t["W"], t["V"], indptr, indices, data, y, case["loss"], C.LAM)
        ref = dict(ref, forward=(terms["y"], terms["X"], terms["nnz"]), loss=terms["loss"])
        f32["forward"] = f32["y"]
        for name in FR.NAMES + ("forward", "loss"):
            G, E, n = (np.atleast_1d(a) for a in ref[name])
            c = R.ratio(np.atleast_1d(f32[name]), G, E, n)
            print("%s step%d %s: c_ref short %.2f long %.2f (longest run %d)" % (case["id"], s, name, c["short"], c["long"], int(np.max(n))))
            assert np.isfinite(list(c.values())).all() and c["short"] <= R.LONG_RUN and c["long"] <= max(1, np.max(n)), (name, c)


# ----------------------------------------------------------------------------- a float32 stand-in for the device
def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * float(b) + np.asarray(c, np.float64)).astype(F4)


def _runs(f, G):
    """the stable sort by feature, the piece each sorted entry belongs to, each piece's feature, and the cut runs' features"""
    order = np.argsort(f, kind="stable")
    ks = f[order]
    j = np.arange(ks.size)
    head = np.concatenate(([True], ks[1:] != ks[:-1]))
    pstart = head | (j % C.piece_len(G) == 0)
    piece = np.cumsum(pstart) - 1
    pfeat = ks[pstart]
    cut = np.unique(pfeat[np.flatnonzero(~head[pstart])])
    return order, piece, pfeat, cut


def _device_step(st, csr, y, case, powers, fault=None):
    """one step in float32 in the kernels' order of operations (csrc/fm_kernels.hip, k_seg_reduce's FM branch, adam_sparse,
    finalize.inc.h), with the planted faults"""
    indptr, indices, data = csr
    D, F, n = case["D"], case["F"], indptr.size - 1
    G, _ = C.geometry(D)
    lr, lam = C.hyper_of(case)
    mu, W, V = F4(st["mu"]["w"]), st["W"]["w"], st["V"]["w"]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    f, x = indices.astype(np.int64), data.astype(F4)
    xv = x[:, None] * V[f]
    S = so.segment_sum(xv, rows, n)
    acc = np.sum(S * S - so.segment_sum(xv * xv, rows, n), axis=1, dtype=F4)
    yhat = (mu + so.segment_sum(x * W[f], rows, n)) + F4(0.5) * acc
    g = so.dlogits(yhat, y.astype(F4), case["loss"]).astype(F4)
    a = g[rows] * x
    b = F4(lam) - a * x if fault != "no_x2" else np.full(a.shape, F4(lam))
    srow = S[np.minimum(rows + 1, n - 1)] if fault == "neighbour_s" else S[rows]
    tV = a[:, None] * srow + b[:, None] * V[f]
    tW = a + F4(lam) * W[f] if fault != "no_lamW" else a
    order, piece, pfeat, cut = _runs(f, G)
    cnt = np.bincount(f, minlength=F)
    if fault == "drop":                                   # an entry of a feature with three entries is lost
        k = np.flatnonzero(cnt[f[order]] == 3)[1]
        order, piece = np.delete(order, k), np.delete(piece, k)
    if fault == "twice":                                  # the first entry of a cut run's second piece is added again
        k = np.flatnonzero(np.isin(f[order], cut) & (np.arange(order.size) % C.piece_len(G) == 0))[0]
        order, piece = np.insert(order, k, order[k]), np.insert(piece, k, piece[k])
    grads = {}
    for name, t in (("V", tV), ("W", tW)):                # a piece in entry order, then a run's pieces in piece order
        grads[name] = so.segment_sum(so.segment_sum(t[order], piece, pfeat.size), pfeat, F)
    gpb = 256 // G
    keep = np.ones(n, bool)
    if fault == "mu_partial":
        keep[gpb:2 * gpb] = False                         # the second block's partial is missing
    grads["mu"] = np.sum(g[keep], dtype=F4)
    touched = cnt > 0
    new = {}
    if case["opt"] == "sgd":
        for name in FR.NAMES:
            w = np.array(st[name]["w"], F4)
            w2 = (w - F4(lr) * grads[name]).astype(F4)
            if name != "mu":
                w2[~touched] = w[~touched]
            new[name] = dict(w=w2)
        return new, yhat
    alpha = F4(R.alpha_f32(lr, *powers))
    omb1, omb2, eps = F4(1) - R.B1F, F4(1) - R.B2F, F4(so.EPSILON)
    for name in FR.NAMES:
        gr = np.asarray(grads[name], F4)
        w, m, v = (np.array(st[name][k], F4) for k in ("w", "m", "v"))
        if name == "mu":
            m2 = m + (gr - m) * omb1
            v2 = v + (gr * gr - v) * omb2
            w2 = w - (alpha * m2) / (np.sqrt(v2) + eps)
        else:
            m2 = _fma32(m, R.B1F, gr * omb1)
            v2 = _fma32(v, R.B2F, (gr * gr) * omb2)
            w2 = w - alpha * m2 / (np.sqrt(v2) + eps)
            for new_, old in ((m2, m), (v2, v), (w2, w)):
                new_[~touched] = old[~touched]
            if fault == "v_cut_head" and name == "V":     # the head piece of a cut run applies, its v stays
                v2[cut] = v[cut]
            if fault == "m_untouched" and name == "W":
                m2[np.flatnonzero(~touched)[0]] += F4(1e-6)
        new[name] = dict(w=np.asarray(w2, F4), m=np.asarray(m2, F4), v=np.asarray(v2, F4))
    return new, yhat


def _two_device_steps(case, fault=None):
    t = C.tables_of(case)
    adam = case["opt"] == "adam"
    st = {k: dict(w=np.asarray(t[k], F4)) for k in FR.NAMES}
    if adam:
        for k in FR.NAMES:
            st[k].update(m=np.zeros(np.shape(t[k]), F4), v=np.zeros(np.shape(t[k]), F4))
    lr, lam = C.hyper_of(case)
    powers = (R.B1F, R.B2F)
    bad = []
    for s in range(2):
        csr, y = C.batch_of(case, s)
        new, yhat = _device_step(st, csr, y, case, powers, fault)
        bad += FR.check_fm_step(st, new, csr, y, opt=case["opt"], loss=case["loss"], lam=lam, lr=lr, powers=powers, fresh=s == 0,
                                pred=yhat)
        st, powers = new, (F4(powers[0] * R.B1F), F4(powers[1] * R.B2F))
    return bad


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_the_device_stand_in_passes_every_check(case):
    bad = _two_device_steps(case)
    assert not bad, bad


FAULT_CASE = [c for c in C.CASES if c["id"] == "edges-F400-D100-n701-nll_adam"][0]
# fault -> the table the violated statement must name
FAULTS = {
    "drop": "V", "twice": "V", "no_lamW": "W", "no_x2": "V", "neighbour_s": "V", "v_cut_head": "V", "m_untouched": "W.m",
    "mu_partial": "mu",
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_rejected(fault):
    """Each fault, planted in the stand-in's two lazy-Adam steps at D = 100 (G = 32: pieces of 32 entries), is rejected, and
    a violated statement names the table:

      drop          an entry of a feature with three entries lost                 V (and W) gradient, short runs
      twice         an entry of a cut run counted twice                           V (and W) gradient, long runs
      no_lamW       lam * W_j missing from every entry                            W gradient
      no_x2         the - g x^2 V_j term missing (b = lam)                        V gradient
      neighbour_s   s_r taken from the next row                                   V gradient
      v_cut_head    v not updated on the features whose run is cut                V: v does not follow from g
      m_untouched   m of a feature outside the batch changed                      W.m: rows outside the batch changed
      mu_partial    mu's gradient without one block's partial                     mu gradient"""
    bad = _two_device_steps(FAULT_CASE, fault)
    print("fault %s: %d statements violated, first: %s" % (fault, len(bad), bad[:1]))
    assert any(b.startswith(FAULTS[fault]) for b in bad), "fault %s passes, or no statement names %s: %s" % (fault, FAULTS[fault], bad)


def test_cases_cover_what_the_issue_names():
    kinds = {c["kind"] for c in C.CASES}
    assert kinds == {"edges", "empty", "stride"}
    for d in (64, 100):
        assert {(c["loss"], c["opt"]) for c in C.CASES if c["D"] == d and c["kind"] == "edges"} == set(C.PAIRS)
    stride = [c for c in C.CASES if c["kind"] == "stride"][0]
    G, _ = C.geometry(stride["D"])
    assert -(-stride["n"] // (256 // G)) > 4096            # more blocks than fm_grid's cap for the training forward
