"""WARP steps on the device (tfr_warp_*) against tests/warp_ref.py and tests/warp_step_ref.py.

1. the search on exact tables equals the float64 reference; the weights to 2 ulp      (tests/warp_cases.py EXACT)
2. the search on random tables: every decision outside the rounding band                (RANDOM)
3. the step per row, with the negatives and trial counts the device reports             (BPR's run-edge batches)
4. the forms agree bit for bit      5. refusals      6. it learns a planted ranking as the float64 trainer does"""
import time

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import bpr_cases as BC
from tests import bpr_step_ref as BS
from tests import step_ref as R
from tests import warp_cases as C
from tests import warp_ref as WR
from tests import warp_step_ref as S
from tests import widths as W

pytestmark = pytest.mark.gpu

ALL = ("mu", "bu", "bi", "P", "Q")
assert {c["D"] for c in C.EXACT if c["kind"] == "random" and c["I"] == 200} >= set(W.BPR)


def _world_model(w, case, **kw):
    t = w["t"]
    m = T.SvdModel(w["U"], t["Q"].shape[0], case["D"], item_abs=case["item_abs"], **kw)
    m.set_tables(*(t[k] for k in ALL))
    m.set_positives(w["pos"])
    m.set_bpr_sampler(C.SEED, case["attempts"])
    m.set_warp(case["margin"])
    return m


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- 1. exact search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.EXACT, ids=lambda c: c["id"])
def test_the_search_on_exact_tables_equals_the_reference(case):
    """every product and partial sum is exact in float32 in any order: the negatives and trial counts equal the float64
    reference's.  In the planted worlds an SGD step with lr 1 and lam 0 leaves each triple's weight in P'[u, 0] (P[u, 0] = 0
    and Q'[i] - Q'[j] is 1 there): it matches log(max(1, (I - 1) // N)) to 2 ulp, and is +0 for a skipped triple."""
    w, e = C.exact_world(case), C.exact_reference(case)
    with _world_model(w, case, optimizer="sgd", lr=1.0, reg=0.0) as m:
        neg, trials = m.warp_negatives(w["u"], w["i"], step=C.STEP)
        assert np.array_equal(neg, e["neg"]), np.flatnonzero(neg != e["neg"])[:10]
        assert np.array_equal(trials, e["trials"]), np.flatnonzero(trials != e["trials"])[:10]
        if case["margin"] == C.INF:
            assert np.array_equal(neg, m.bpr_negatives(w["u"], step=C.STEP)) and np.array_equal(trials, (neg >= 0).astype(np.int32))
        if case["margin"] == -C.INF:
            assert (neg == -1).all() and (trials == 0).all()
        if not case["kind"].startswith("planted"):
            return
        m.set_step(C.STEP, 0.9, 0.999)
        neg2, trials2, lossv, _, skipped = m.train_warp_step(w["u"], w["i"])
        assert np.array_equal(neg2, neg) and np.array_equal(trials2, trials) and skipped == int((neg < 0).sum())
        wgt = m.get_table(L.P)[:, 0]
    want = WR.weights(case["I"], e["trials"])
    print("%s: N in %s, weights %.4f..%.4f, worst %d ulp" % (case["id"], sorted(set(e["trials"].tolist())), want.min(), want.max(),
                                                             int(_ulps(wgt, want.astype(np.float32)).max())))
    assert (_ulps(wgt, want.astype(np.float32)) <= 2).all()
    assert not wgt[e["neg"] < 0].view(np.uint32).any()
    # x = 0 for every live triple: the data term is sum w (margin - 0)
    assert abs(lossv - want.sum() * case["margin"]) <= 1e-5 * max(1.0, want.sum())


# ---- 2. random tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.RANDOM, ids=lambda c: c["id"])
def test_the_search_on_random_tables_decides_as_the_reference_outside_the_band(case):
    w, e = C.random_world(case), C.random_reference(case)
    with _world_model(w, case, optimizer="sgd") as m:
        neg, trials = m.warp_negatives(w["u"], w["i"], step=C.STEP)
    bad, share = WR.check_search(e, neg, trials)
    print("%s: in-band share %.4f (reference %.4f), live %.3f, differing from the reference %d of %d"
          % (case["id"], share, WR.in_band_share(e), np.mean(neg >= 0), int(((neg != e["neg"]) | (trials != e["trials"])).sum()), neg.size))
    assert not bad, bad
    assert share <= C.BAND_CAP


# ---- 3. the step per row -----------------------------------------------------------------------------------------------
def _snapshot(m, adam):
    out = {}
    for name in ALL:
        tid = BS.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        out[name] = d
    return out


def _step_model(case):
    lr, lam = BC.hyper_of(case, 0)
    t = BC.tables_of(case)
    m = T.SvdModel(case["U"], case["I"], case["D"], item_abs=case["item_abs"], reg_bias=case["reg_bias"], optimizer=case["opt"],
                   adam_mode="lazy", lr=lr, reg=lam)
    m.set_tables(*(t[k] for k in ALL))
    m.set_positives(BC.positives(case["kind"]))
    if case["kind"] == "skip":
        m.set_bpr_sampler(BC.SEED, 1)
    if case["frozen"]:
        m.set_frozen(case["frozen"])
    m.set_warp(C.margin_of(case))
    return m


@pytest.mark.parametrize("case", C.STEP_CASES, ids=lambda c: c["id"])
def test_two_warp_steps_per_row(case):
    """two successive steps on a fresh model, every table and its m and v read before, between and after; the negatives
    and trial counts are the ones the device reports (searched in the skip cases and held there against ``check_search``)"""
    adam = case["opt"] == "adam"
    margin = C.margin_of(case)
    sampled = case["kind"] == "skip"
    pos = BC.positives(case["kind"])
    report = {}
    t0 = time.time()
    try:
        with _step_model(case) as m:
            before = _snapshot(m, adam)
            for s in range(2):
                if s == 1 and case["hyper2"]:
                    m.set_hyper(*case["hyper2"])
                lr, lam = BC.hyper_of(case, s)
                u, i, j = BC.batch_of(case, s)
                _, b1p, b2p = m.get_step()
                neg, trials, lossv, regv, skipped = m.train_warp_step(u, i, None if sampled else j)
                after = _snapshot(m, adam)
                assert m.get_step()[0] == s + 1 and skipped == (int((neg < 0).sum()) if sampled else 0)
                if sampled:
                    tabs = {k: before[k]["w"] for k in ("P", "Q", "bi")}
                    e = WR.examine(C.tid_tables(tabs), *pos, u, i, margin, seed=BC.SEED, step=s, attempts=1, item_abs=case["item_abs"])
                    bad, _ = WR.check_search(e, neg, trials)
                    assert not bad, bad
                    live = neg >= 0
                    nu = np.bincount(u[live], minlength=case["U"]) * np.bincount(u[~live], minlength=case["U"])
                    assert nu.any() and (neg[u == BC.FULL] < 0).all(), "no user run mixes live and skipped triples"
                else:
                    assert np.array_equal(neg, j) and (trials == 1).all()
                rep = report.setdefault("step%d" % s, {})
                bad = S.check_warp_step(before, after, u, i, neg, trials, margin=margin, opt=case["opt"], item_abs=case["item_abs"],
                                        reg_bias=case["reg_bias"], lam=lam, lr=lr, powers=(b1p, b2p), fresh=s == 0,
                                        frozen=case["frozen"], lossv=lossv, regv=regv, report=rep)
                assert not bad, "%s, step %d:\n  %s" % (case["id"], s, "\n  ".join(bad))
                before = after
    finally:
        for step, rep in sorted(report.items()):
            for name, v in rep.items():
                print("RATIO %s %s %s dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
                    case["id"], step, name, v["dev"]["short"], v["dev"]["long"], v["c_ref"]["short"], v["c_ref"]["long"]))
        print("TIME %s %.1f s" % (case["id"], time.time() - t0))


# ---- 4. the forms agree bit for bit ------------------------------------------------------------------------------------
FORM_CASE = C.RANDOM[0]


def _form_model():
    w = C.random_world(FORM_CASE)
    m = _world_model(w, FORM_CASE, optimizer="adam", adam_mode="lazy", lr=1e-2, reg=0.01)
    return m, w


def _bits(m):
    return {k: m.get_table(BS.TID[k] | s).tobytes() for k in ALL for s in (0, L.SLOT_M, L.SLOT_V)}


def test_a_repeat_and_the_device_form_give_the_same_bits():
    torch = pytest.importorskip("torch")
    res = []
    for how in ("host", "host", "dev"):
        m, w = _form_model()
        with m:
            out = []
            for s in range(2):
                if how == "host":
                    ahead = m.warp_negatives(w["u"], w["i"], step=m.step)
                    neg, trials = m.train_warp_step(w["u"], w["i"])[:2]
                    assert np.array_equal(ahead[0], neg) and np.array_equal(ahead[1], trials)   # what the next step reports
                else:
                    d = [torch.from_numpy(a).cuda() for a in (w["u"], w["i"])]
                    neg, trials = m.train_warp_step_dev(d[0], d[1], want_negatives=True)
                    m.sync()
                    torch.cuda.synchronize()
                    neg, trials = neg.cpu().numpy(), trials.cpu().numpy()
                out.append((neg.tobytes(), trials.tobytes()))
            assert m.step == 2
            res.append((out, _bits(m)))
    assert res[0] == res[1], "a repeat of the same steps differs"
    assert res[0] == res[2], "train_warp_step_dev differs from train_warp_step"


def test_the_drawn_form_equals_explicit_steps_on_the_pairs_the_generator_draws():
    B, steps = 700, 3
    res = []
    for drawn in (True, False):
        m, w = _form_model()
        indptr, items = w["pos"]
        nnz = int(indptr[-1])
        rowof = np.repeat(np.arange(w["U"]), np.diff(indptr)).astype(np.int32)
        with m:
            np.random.seed(2024)
            if drawn:
                m.rng_from_numpy()
                loss = m.train_warp_steps_drawn(B, steps, want_loss=True)
                k, p = m.rng_get_state()
                np.random.randint(0, nnz, (steps, B))
                want = np.random.get_state()
                assert np.array_equal(k, want[1]) and p == want[2]
            else:
                loss = []
                for _ in range(steps):
                    e = np.random.randint(0, nnz, B)
                    loss.append(m.train_warp_step(rowof[e], items[e])[2])
                loss = np.asarray(loss, np.float32)
            assert m.step == steps
            res.append((loss.tobytes(), _bits(m)))
    assert res[0] == res[1]


def test_the_drawn_form_draws_the_pairs_the_bpr_drawn_form_draws():
    """from one generator state tfr_warp_train_steps_drawn and tfr_bpr_train_steps_drawn leave the same generator state"""
    states = []
    for warp in (True, False):
        m, _ = _form_model()
        with m:
            m.rng_seed(11)
            (m.train_warp_steps_drawn if warp else m.train_bpr_steps_drawn)(700, 2)
            k, p = m.rng_get_state()
            states.append((k.tobytes(), p))
    assert states[0] == states[1]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def _small(U=20, I=10, D=8, pos=True, **kw):
    rs = np.random.RandomState(0)
    f = lambda *s: rs.normal(0, 0.3, s).astype(np.float32)
    t = dict(mu=np.float32(0.1), bu=f(U), bi=f(I), P=f(U, D), Q=f(I, D))
    m = T.SvdModel(U, I, D, **kw)
    m.set_tables(*(t[k] for k in ALL))
    if pos:
        m.set_positives((np.arange(U + 1, dtype=np.int64), (np.arange(U) % I).astype(np.int32)))
    return m, t


def test_tf1_adam_and_unset_positives_are_refused():
    m, _ = _small(optimizer="adam", adam_mode="tf1")
    with m:
        m.rng_seed(1)
        for call in (lambda: m.train_warp_step([0, 1], [2, 3]), lambda: m.train_warp_steps_drawn(4, 2)):
            with pytest.raises(L.TfrError) as e:
                call()
            assert e.value.code == L.ERR_STATE
        assert m.step == 0
    m, _ = _small(pos=False, optimizer="sgd")
    with m:
        m.rng_seed(0)
        for call in (lambda: m.warp_negatives([0, 1], [1, 2]), lambda: m.train_warp_step([0], [1]),
                     lambda: m.train_warp_step([0], [1], [2]), lambda: m.train_warp_steps_drawn(4, 1)):
            with pytest.raises(L.TfrError) as e:
                call()
            assert e.value.code == L.ERR_STATE


def test_one_item_is_refused():
    m, _ = _small(U=5, I=1, optimizer="sgd")
    with m:
        m.rng_seed(0)
        for call in (lambda: m.warp_negatives([0], [0]), lambda: m.train_warp_step([0], [0]),
                     lambda: m.train_warp_step([0], [0], [0]), lambda: m.train_warp_steps_drawn(4, 1)):
            with pytest.raises(L.TfrError) as e:
                call()
            assert e.value.code == L.ERR_ARG
        assert m.step == 0


def test_an_out_of_range_id_voids_the_step():
    import torch
    m, t = _small(U=30, I=20, optimizer="adam", adam_mode="lazy")
    with m:
        m.set_warp(1.0)
        for u, i, j in (([0, 30], [1, 2], None), ([0, 1], [1, 20], None), ([0, -1], [1, 2], None), ([0, 1], [1, -3], None),
                        ([0, 1], [1, 2], [3, 20]), ([0, 1], [1, 2], [3, -1])):
            with pytest.raises(L.OutOfRangeError):
                m.train_warp_step(u, i, j)
            assert m.step == 0
        with pytest.raises(L.OutOfRangeError):
            m.warp_negatives([0, 30], [1, 2])
        d = torch.device("cuda")
        m.train_warp_step_dev(torch.tensor([0, 1], dtype=torch.int32, device=d), torch.tensor([1, 25], dtype=torch.int32, device=d))
        with pytest.raises(L.OutOfRangeError):
            m.sync()
        for k in ALL:
            for s in (0, L.SLOT_M, L.SLOT_V):
                got = m.get_table(BS.TID[k] | s)
                assert R.same_bits(got, t[k] if s == 0 else np.zeros_like(got)), (k, s)


def test_a_model_with_a_live_trainer_is_not_destroyed():
    lib = L.load()
    m, t = _small(optimizer="sgd")
    m.set_warp(0.5)
    assert lib.tfr_destroy(m._h) == L.ERR_STATE and b"WARP" in lib.tfr_last_error()
    neg, trials = m.warp_negatives([0, 1], [1, 2])           # both intact
    assert neg.shape == (2,) and R.same_bits(m.get_table(L.Q), t["Q"])
    with pytest.raises(L.TfrError) as e:
        m.set_warp(float("nan"))
    assert e.value.code == L.ERR_ARG
    m.close()
    assert m._h is None and m._warp is None


# ---- 6. it learns ------------------------------------------------------------------------------------------------------
def _planted(U=300, I=200, rank=4, train=20, held=10, beta=4.0, seed=0):
    """each user's items drawn from softmax(beta a_u . b_i / sqrt(rank)) of a rank-4 truth: 20 to train on, 10 held out"""
    rs = np.random.RandomState(seed)
    s = rs.normal(0, 1, (U, rank)) @ rs.normal(0, 1, (I, rank)).T / np.sqrt(rank)
    tr, te = [], []
    for u in range(U):
        p = np.exp(beta * (s[u] - s[u].max()))
        it = rs.choice(I, train + held, replace=False, p=p / p.sum())
        tr.append(np.sort(it[:train]))
        te.append(np.sort(it[train:]))
    return tr, te


def _recall10(P, Q, bi, tr, te):
    hits = 0
    for u in range(P.shape[0]):
        s = P[u] @ Q.T + bi
        s[tr[u]] = -np.inf
        top = np.lexsort((np.arange(s.size), -s))[:10]
        hits += np.intersect1d(top, te[u]).size
    return hits / float(sum(len(r) for r in te))


def test_warp_learns_a_planted_ranking_as_the_float64_trainer_does():
    U, I, D, B, steps, seed = 300, 200, 16, 1000, 300, 77
    tr, te = _planted(U, I)
    pos = C._csr(tr)
    nnz = int(pos[0][-1])
    rowof = np.repeat(np.arange(U), np.diff(pos[0])).astype(np.int32)
    tu = np.repeat(np.arange(U), [r.size for r in te]).astype(np.int32)
    ti = np.concatenate(te).astype(np.int32)
    H = ti.size
    rs = np.random.RandomState(1)
    t = dict(mu=np.float32(0), bu=np.zeros(U, np.float32), bi=np.zeros(I, np.float32),
             P=rs.normal(0, .1, (U, D)).astype(np.float32), Q=rs.normal(0, .1, (I, D)).astype(np.float32))
    kw = dict(optimizer="adam", lr=0.02, reg=0.002)
    excl = T.rated_matrix(rowof, pos[1], U, I)
    with T.SvdModel(U, I, D, adam_mode="lazy", **kw) as m:
        m.set_tables(*(t[k] for k in ALL))
        m.set_positives(pos)
        m.set_bpr_sampler(seed, 16)
        m.set_warp(1.0)
        r0 = T.evaluate_ranking(m, tu, ti, exclude=excl)["mean"]["recall@10"]
        np.random.seed(3)
        m.rng_from_numpy()
        m.train_warp_steps_drawn(B, steps)
        r1 = T.evaluate_ranking(m, tu, ti, exclude=excl)["mean"]["recall@10"]
    ref = WR.WarpRef(U, I, D, margin=1.0, seed=seed, attempts=16, **kw)
    ref.set_tables({WR.MU: t["mu"], WR.BU: t["bu"], WR.BI: t["bi"], WR.PF: t["P"], WR.QF: t["Q"]})
    ref.set_positives(*pos)
    np.random.seed(3)
    t0 = time.time()
    for e in np.random.randint(0, nnz, (steps, B)):
        ref.train_step(rowof[e], pos[1][e])
    rr = _recall10(ref.t[WR.PF], ref.t[WR.QF], ref.t[WR.BI], tr, te)
    se = np.sqrt(rr * (1 - rr) / H)
    print("Recall@10: untrained %.4f, device %.4f, float64 trainer %.4f (3 se = %.4f, H = %d); reference %.1f s"
          % (r0, r1, rr, 3 * se, H, time.time() - t0))
    assert r1 > r0
    assert r1 >= rr - 3 * se


def test_the_driver_runs_two_epochs(capsys):
    from tfrecomm_amd import svd_train_val
    tr, te = _planted(300, 200)
    mk = lambda rows: {"user": np.repeat(np.arange(300), [r.size for r in rows]).astype(np.int32),
                       "item": np.concatenate(rows).astype(np.int32)}
    rows = svd_train_val.warp(mk(tr), mk(te), user_num=300, item_num=200, dim=8, batch_size=500, epoch_max=2)
    out = capsys.readouterr().out
    assert "warp_loss" in out and "recall@10" in out
    assert len(rows) == 2 and all(np.isfinite(x) for row in rows for x in row)
