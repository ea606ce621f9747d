"""The per-row step checks of tests/step_ref.py, themselves tested on the CPU: the float32 oracle stays inside the
gradient bound on the GPU test's own inputs, a float32 NumPy restatement of two steps passes every check, the same
restatement with one planted fault is rejected, and the case list reaches every step path."""
import numpy as np
import pytest

from oracle import svd_oracle as so
from tests import step_cases as S
from tests import step_ref as R
from tests.util import dup_heavy_ids, make_oracle, rand_tables, rel_err

F = np.float32


def test_segment_sums_agree():
    rs = np.random.RandomState(0)
    ids = dup_heavy_ids(rs, 900, 5000).astype(np.int64)
    vals = rs.normal(size=(5000, 24))
    assert vals.size > 1 << 16                                         # the sort + reduceat form
    assert np.allclose(R.seg_sum(vals, ids, 900), so.segment_sum(vals, ids, 900), rtol=1e-13, atol=1e-13)
    assert np.array_equal(R.seg_sum(vals[:100], ids[:100], 900), so.segment_sum(vals[:100], ids[:100], 900))


# ----------------------------------------------------------------------------- the float32 oracle inside the bound
HOST_CASES = [c for c in S.CASES if c["B"] * c["D"] <= 700000 and not c["frozen"] and not c["hyper2"]]


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c["id"])
def test_float32_oracle_stays_inside_the_bound(case):
    """A sequential float32 sum of n terms is off by at most (n - 1) eps32 sum|terms| beyond the first-order bound E, so
    its ratio is at most n: 64 for the short class, the longest run for the long one.  That is a worst case (the sum
    behaves like ~1.5 sqrt(n)); what it guards is E itself - without the delta term the float32 oracle is off by
    10^3..10^5 x eps32 x sum|occ| on rows where x - r cancels.  The figures are printed (run with -s)."""
    t = S.tables_of(case)
    u, i, r = S.batch_of(case, 0)
    flags = (case["loss"], case["item_abs"], case["reg_bias"], S.REG)
    ref, _, _ = R.step_grads(t, u, i, r, *flags)
    f32 = R.f32_oracle_grads(t, u, i, r, *flags)
    for name in R.NAMES:
        G, E, n = ref[name]
        c = R.ratio(f32[name], G, E, n)
        print("%s %s: c_ref short %.2f long %.2f (longest run %d)" % (case["id"], name, c["short"], c["long"], int(np.max(n))))
        assert c["short"] <= R.LONG_RUN and c["long"] <= np.max(n), (name, c)


@pytest.mark.parametrize("case", [c for c in S.CASES if c["tables"] == "zeros"], ids=lambda c: c["id"])
def test_zero_cases_hold_what_they_were_built_for(case):
    """planted zeros of both signs in Q rows both steps touch, the float64 gradient there exactly lam * 0"""
    S.assert_zero_edges(case)


# ----------------------------------------------------------------------------- a float32 restatement with planted faults
U_, I_, D_, B_ = 300, 200, 20, 4000                 # hot rows hold ~90 (users) and ~140 (items) entries
LR_, LAM_ = 3e-3, 0.02


def _grads32(w, u, i, r, fault):
    """float32, batch order - with the gradient faults (a)-(e), (k)"""
    P, Q, bu, bi, mu = (w[k] for k in ("P", "Q", "bu", "bi", "mu"))
    x = so.forward(P, Q, bu, bi, mu, u, i, True)
    g = so.dlogits(x, r, so.MSE).astype(F)
    oP, oQ, obu, obi, _ = so.occurrence_grads(P, Q, bu, bi, u, i, g, LAM_, True, fault == "d")
    if fault == "c":
        oP = so.occurrence_grads(P, Q, bu, bi, u, i, g, 0.0, True, False)[0]
    if fault == "e":
        oQ = g[:, None] * P[u] + F(LAM_) * Q[i]
    iu, ii, oQ2, oP2 = u, i, oQ, oP
    if fault == "a":                                                   # the last entry of the longest item run is lost
        k = np.flatnonzero(i == np.bincount(i).argmax())[-1]
        ii, oQ2 = np.delete(i, k), np.delete(oQ, k, axis=0)
    if fault == "b":                                                   # the first 64 entries of the longest user run, twice
        k = np.flatnonzero(u == np.bincount(u).argmax())[:64]
        iu, oP2 = np.concatenate((u[k], u)), np.concatenate((oP[k], oP))
    out = dict(P=so.segment_sum(oP2, iu, U_), Q=so.segment_sum(oQ2, ii, I_), bu=so.segment_sum(obu, u, U_),
               bi=so.segment_sum(obi, i, I_), mu=np.cumsum(g, dtype=F)[-1])
    if fault == "k":
        out["P"][:, D_ - 1] = out["P"][:, D_ - 2]
    return out, x


def _fma32(a, b, c):
    return (a.astype(np.float64) * float(b) + c.astype(np.float64)).astype(F)


def _restated_step(st, u, i, r, mode, powers, fault):
    """one Adam step in float32 in the kernels' operation order (csrc/svd_kernels.hip adam_sparse, finalize.inc.h)"""
    w = {k: st[k]["w"] for k in R.NAMES}
    grads, _ = _grads32(w, u, i, r, fault)
    b1p, b2p = powers
    if fault == "g":
        b1p, b2p = F(b1p * R.B1F), F(b2p * R.B2F)
    alpha = F(R.alpha_f32(LR_, b1p, b2p))
    omb1, omb2, eps = F(1) - R.B1F, F(1) - R.B2F, F(so.EPSILON)
    new = {}
    for name in R.NAMES:
        g = np.asarray(grads[name], F)
        wv, m, v = (np.array(st[name][k], F) for k in ("w", "m", "v"))
        if name == "mu":
            m2 = m + (g - m) * omb1
            v2 = v + (g * g - v) * omb2
            w2 = wv - (alpha * m2) / (np.sqrt(v2) + eps)
        else:
            ids = u if name in ("P", "bu") else i
            hit = np.zeros(wv.shape[0], bool)
            hit[ids] = True
            gsq = g * g
            if fault == "j":                                           # sum of squares instead of the sum's square
                occ = so.occurrence_grads(w["P"], w["Q"], w["bu"], w["bi"], u, i, so.dlogits(so.forward(
                    w["P"], w["Q"], w["bu"], w["bi"], w["mu"], u, i, True), r, so.MSE).astype(F), LAM_, True, False)
                gsq = so.segment_sum(occ[dict(P=0, Q=1, bu=2, bi=3)[name]] ** 2, ids, wv.shape[0])
            m2 = _fma32(m, R.B1F, g * omb1)
            v2 = _fma32(v, R.B2F, gsq * omb2)
            den = np.sqrt(v2 + eps) if fault == "f" else np.sqrt(v2) + eps
            w2 = wv - alpha * m2 / den
            lazy_rows = mode == so.LAZY or fault == "h"
            if fault == "i":                                           # lazy, but the moments of every row decay
                w2[~hit] = wv[~hit]
            elif lazy_rows:
                for new_, old in ((m2, m), (v2, v), (w2, wv)):
                    new_[~hit] = old[~hit]
        new[name] = dict(w=w2.astype(F), m=m2.astype(F), v=v2.astype(F))
    return new


def _two_restated_steps(mode, fault):
    rs = np.random.RandomState(5)
    t = rand_tables(rs, U_, I_, D_)
    st = {k: dict(w=np.asarray(t[k], F), m=np.zeros(np.shape(t[k]), F), v=np.zeros(np.shape(t[k]), F)) for k in R.NAMES}
    orc = make_oracle(U_, I_, D_, t, loss="mse", item_abs=True, reg_bias=False, optimizer="adam", adam_mode=mode, lr=LR_, reg=LAM_)
    powers = (R.B1F, R.B2F)
    bad = []
    for s in range(2):
        u, i = dup_heavy_ids(rs, U_, B_).astype(np.int64), dup_heavy_ids(rs, I_, B_).astype(np.int64)
        r = rs.randint(1, 6, B_).astype(F)
        new = _restated_step(st, u, i, r, mode, powers, fault)
        bad += R.check_step(st, new, u, i, r, opt="adam", mode=mode, loss="mse", item_abs=True, reg_bias=False, lam=LAM_,
                            lr=LR_, powers=powers, fresh=s == 0)
        orc.train_step(u, i, r)
        st, powers = new, (F(powers[0] * R.B1F), F(powers[1] * R.B2F))
    # the suite's earlier metric on the same result: every table within 2e-4 * max(1, sqrt(run / 64)) of the float64 oracle's,
    # scale-relative (tests/test_gpu_parity.py test_random_shapes_two_steps)
    tol = 2e-4 * max(1.0, np.sqrt(7.0 * B_ / min(U_, I_) / 64))
    old_passes = all(rel_err(st[k]["w"], orc.tables()[R.TID[k]]) <= tol for k in R.NAMES)
    return bad, old_passes


@pytest.mark.parametrize("mode", ["tf1", "lazy"])
def test_the_restated_step_passes_every_check(mode):
    bad, old_passes = _two_restated_steps(mode, None)
    assert not bad, bad
    assert old_passes


# fault -> (Adam mode it is planted in, whether the table-level metric lets it through)
FAULTS = {
    "a": ("tf1", True), "b": ("tf1", True), "c": ("tf1", True), "d": ("tf1", True), "e": ("tf1", False), "f": ("tf1", False),
    "g": ("tf1", False), "h": ("tf1", False), "i": ("lazy", True), "j": ("tf1", False), "k": ("tf1", False),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_rejected(fault):
    """Each fault, planted in the float32 restatement of two Adam steps (300 x 200 rows, D = 20, B = 4000, item_abs on,
    reg_bias off), is rejected by the per-row checks.  Beside it, what the table-level metric (every table within
    2e-4 * max(1, sqrt(run / 64)) of the float64 oracle's, scale-relative) says of the same wrong result:

      (a) the last entry of the longest run dropped                      gradient, long runs      table metric: passes
      (b) the first 64 entries of the longest run added twice            gradient, long runs      table metric: passes
      (c) lam terms dropped from P only                                  gradient                 table metric: passes
      (d) lam * bias added although reg_bias is off                      gradient (bu, bi)        table metric: passes
      (e) sign(q) omitted under item_abs                                 gradient (Q)             table metric: fails
      (f) sqrt(v + eps) instead of sqrt(v) + eps                         apply                    table metric: fails
      (g) alpha from the next step's beta powers                         apply                    table metric: fails
      (h) TF1 mode, untouched rows left alone                            gradient (m not decayed) table metric: fails
      (i) lazy mode, untouched rows' moments decayed                     identical bits           table metric: passes
      (j) v from the sum of g_k^2 instead of (sum g_k)^2                 moments                  table metric: fails
      (k) element D - 1 of a row's gradient taken from element D - 2     gradient (P)             table metric: fails

    The last column is asserted too, so the table cannot go stale."""
    mode, old = FAULTS[fault]
    bad, old_passes = _two_restated_steps(mode, fault)
    print("fault (%s): %d statements violated, first: %s; table metric passes: %s" % (fault, len(bad), bad[:1], old_passes))
    assert bad, "fault (%s) passes every per-row check" % fault
    assert old_passes == old, "fault (%s): the docstring's table is out of date" % fault


# ----------------------------------------------------------------------------- the case list reaches every path
def test_every_case_takes_the_path_it_names():
    for c in S.CASES:
        assert S.path_of(c["U"], c["I"], c["B"], c["opt"], c["mode"]) == c["path"], c["id"]


def test_cases_reach_every_branch_under_every_optimiser():
    got = {(c["path"].rstrip("0123456789"), c["opt"], c["mode"]) for c in S.CASES}
    opts = (S.ADAM_TF1, S.ADAM_LAZY, S.SGD)
    want = {("tiles",) + o for o in opts} | {("csort",) + o for o in opts}                   # any optimiser
    want |= {("fused_big",) + o for o in (S.ADAM_LAZY, S.SGD)}                              # touched-rows optimisers only
    want |= {("tf1_big",) + S.ADAM_TF1}
    want |= {("tf1_small",) + S.ADAM_TF1, ("fused_small",) + S.ADAM_LAZY}                    # small_tables without csort_path
    assert not want - got, sorted(want - got)
    tiles = {c["path"] for c in S.CASES if c["path"].startswith("tiles")}
    assert tiles == {"tiles4", "tiles8", "tiles10", "tiles12", "tiles16"}, tiles            # every k_dense_tiles tile count
    zeros = {(c["path"].rstrip("0123456789"), c["D"]) for c in S.CASES if c["tables"] == "zeros" and c["item_abs"]}
    assert {("tiles", 64), ("tiles", 15), ("csort", 32), ("tf1_big", 12), ("fused_big", 16), ("fused_big", 20)} <= zeros, zeros
    frozen = {c["path"].rstrip("0123456789") for c in S.CASES if c["frozen"]}
    assert {"tiles", "csort", "tf1_big", "fused_big"} <= frozen, frozen
    # the restated rule itself at its edges: 16 tiles / 17, 16384 rows / 16385, bins x tiles at 2^20
    assert S.path_of(6040, 3952, 16384, "adam", "tf1") == "tiles16" and S.path_of(6040, 3952, 16385, "adam", "tf1") == "csort"
    assert S.path_of(16384, 10, 1000, "adam", "tf1") == "tiles4" and S.path_of(16385, 10, 1000, "adam", "tf1") == "tf1_big"
    assert S.path_of(6040, 3952, 131072, "sgd", "tf1") == "csort" and S.path_of(6040, 3952, 131073, "sgd", "tf1") == "fused_small"
