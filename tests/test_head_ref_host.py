"""tests/head_ref.py and tests/head_cases.py, themselves tested on the CPU: the float32 stand-ins stay within the stated
bounds, the references reject the heads we fear, and every copy of the head in csrc/ is listed with the GPU test that runs
it."""
import os
import re

import numpy as np
import pytest

from tests import head_cases as C
from tests import head_ref as H
from tests import step_cases as S
from tests import step_ref as R

F = np.float32
SMALL = C.SVD_CONFIGS[0]                                   # 200 x 200, D = 16, B = 140


def test_standins_stay_within_the_bounds_on_random_logits():
    """2000 logits per level and label: the __expf model reaches 0.93 x E_g and 0.96 x E_l at the worst (level -25 with
    z = 0), correctly rounded expf 0.54 x E_g and 0.36 x E_l.  Printed (run with -s), and copied into DESIGN.md."""
    rs = np.random.RandomState(0)
    worst = {}
    for lev in C.LEVELS:
        x = (lev + rs.uniform(-1, 1, 2000)).astype(F)
        for z in (0.0, 1.0):
            zz = np.full(x.size, z, F)
            for fast in (True, False):
                g, l, inf = H.standin(x, zz, fast)
                rg = H.ratio(g, H.grad(x, zz), H.E_g(x, zz))
                rl = H.ratio(l, H.loss(x, zz), H.E_l(x, zz))
                print("RATIO stand-in %s level %+d z %d: g %.2f l %.2f" % ("__expf" if fast else "expf", lev, z, rg, rl))
                worst[fast] = np.maximum(worst.get(fast, 0), (rg, rl))
                assert rg <= 1 and rl <= 1, (lev, z, fast, rg, rl)
                assert H.infer_wrong(inf, x).size == 0
    print("RATIO stand-in worst: __expf g %.2f l %.2f | expf g %.2f l %.2f" % (*worst[True], *worst[False]))


def test_the_tie_rule_is_exact():
    """sigmoid(2^-20) lies four float32 spacings (2^-24) above 0.5 and the bound on s there is 1.5; e >= 1 gives s <= 0.5"""
    s = H.sigmoid(F(H.TIE))
    assert 3.9 < float((s - 0.5) / 2.0 ** -24) <= 4.0
    E_s = H.E_g(F(H.TIE), 0) - 2 * float(s)               # E_g without the subtraction and the reading through m
    assert float(H.bound(E_s)) < 1.6 * 2.0 ** -24
    x = np.array([0.0, -0.0, -2.0 ** -20, -2.0 ** -30, -1e-38, 2.0 ** -20, 2.0 ** -10], F)
    for fast in (True, False):
        assert H.standin(x, np.zeros(x.size, F), fast)[2].tolist() == [0, 0, 0, 0, 0, 1, 1]
    assert H.infer(np.array([2.0 ** -21], F))[0] == -1


ALL_TRAINING = [("svd", SMALL)] + [("fm", d) for d in C.FM_DIMS] + [("svdpp", C.SVDPP_DIMS[0]), ("bpr", C.BPR_DIMS[0])]


def _cases(kind, arg):
    return dict(svd=C.svd_cases, fm=C.fm_cases, svdpp=C.svdpp_cases, bpr=C.bpr_cases)[kind](arg)


@pytest.mark.parametrize("kind,arg", ALL_TRAINING, ids=lambda a: a if isinstance(a, str) else str(a if isinstance(a, int) else a[0]))
def test_both_standins_pass_every_training_check(kind, arg):
    """and stay within 1 x the bound on every case of head_cases"""
    for c in _cases(kind, arg):
        for fast in (True, False):
            rep = {}
            bad = C.check_training(c, C.standin_readings(c, fast), rep)
            assert not bad, (c["id"], fast, bad)
            assert all(v["dev"] <= 1 and v["c_ref"] <= 1 for v in rep.values()), (c["id"], rep)


def test_every_svd_configuration_builds_and_names_its_path():
    for cfg in C.SVD_CONFIGS + C.SVD_SGD_CONFIGS:
        name, path, U, I, D, B, opt, mode = cfg
        assert S.path_of(U, I, B, opt, mode) == path, name
        for c in C.svd_cases(cfg, mixes=("mixed",)):
            assert not C.check_training(c, C.standin_readings(c)), c["id"]
    # 17 tiles is the first batch past the tile path; 16384 + 77 rows are past the counting sort's bins
    assert S.path_of(500, 500, 16384, "adam", "tf1") == "tiles16" and S.path_of(16384, 300, 140, "adam", "tf1") == "tiles4"


@pytest.mark.parametrize("model,n", [("svd", 30001), ("svdpp", 30001), ("fm", 5000)])
def test_both_standins_pass_the_eval_checks(model, n):
    c = C.eval_case(model, n)
    for fast in (True, False):
        assert not C.check_eval(c, **C.standin_eval(c, fast))
        assert not C.check_eval(c, infer=H.standin(c["x"], c["z"], fast)[2])


# ----------------------------------------------------------------------------- the heads we fear
# mutant -> the statement that must reject it, and a case on which it must
MUTANTS = {
    "neglog": ("loss", "L+17", "z0"),             # 1 - s has one significant bit left: -log(2^-24) = 16.6 for a loss of 17
    "clamp": ("g from m of the first bias slot", "L-25", "z0"),      # s = 1e-7 where sigmoid(-25) = 1.4e-11
    "oneminus": ("g from m of the first bias slot", "L-80", "z0"),   # 1 - 1 = 0 where sigmoid(-80) = 1.8e-35
    "floor": ("n_equal", None, None),             # floor(0.5 + 0.5) = 1 at x = +-0 where half to even gives 0
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_heads_are_rejected(mutant):
    """l = -log(s) / -log(1 - s); s clamped to [1e-7, 1 - 1e-7]; g = 1 - sigmoid(-x) - z; infer = floor(s + 0.5): each fails
    the statement named in MUTANTS on the case named there (and is printed with everything else it fails)."""
    statement, probe, mix = MUTANTS[mutant]
    failed = {}
    for c in C.svd_cases(SMALL):
        for b in C.check_training(c, C.standin_readings(c, True, mutant)):
            failed.setdefault(b.split(":")[0], []).append(c["probe"] + "/" + c["mix"])
    ev = C.eval_case("svd", 30001)
    for b in C.check_eval(ev, **C.standin_eval(ev, True, mutant)) + C.check_eval(ev, infer=H.standin(ev["x"], ev["z"], True, mutant)[2]):
        failed.setdefault(b.split(":")[0], []).append("eval")
    for k, v in sorted(failed.items()):
        print("mutant %s fails %r on %d cases: %s" % (mutant, k, len(v), " ".join(v[:12])))
    assert statement in failed, (mutant, sorted(failed))
    if probe:
        assert probe + "/" + mix in failed[statement], (mutant, failed[statement])
    if mutant == "floor":
        assert set(failed) == {"n_equal", "sse", "infer"}          # a tie rule is all it breaks
        x = np.array([0.0, -0.0], F)
        assert H.standin(x, np.zeros(2, F), True, "floor")[2].tolist() == [1, 1]


def test_sign_of_zero_is_rejected_on_every_zeros_case():
    """sign(0) = 1 under item_abs leaves g p at a planted zero where the gradient is lam * 0: the Q gradient statement of
    step_ref fails on every "zeros" case of step_cases, by orders of magnitude"""
    for case in [c for c in S.CASES if c["tables"] == "zeros"]:
        t = S.tables_of(case)
        u, i, r = S.batch_of(case, 0)
        G, E, n = R.step_grads(t, u, i, r, case["loss"], True, case["reg_bias"], S.REG)[0]["Q"]
        f = {k: np.asarray(t[k], F) for k in t}
        x = R.so.forward(f["P"], f["Q"], f["bu"], f["bi"], f["mu"], u, i, True)
        g = R.so.dlogits(x, r.astype(F), case["loss"]).astype(F)
        rows = np.array([row for row, _, _ in S.zero_plan(case)])
        sel = np.flatnonzero(np.isin(i, rows))
        got = {}
        for mutant in (False, True):
            occ = g[sel, None] * f["P"][u[sel]] * H.sign0(f["Q"][i[sel]], mutant) + F(S.REG) * f["Q"][i[sel]]
            got[mutant] = R.ratio(R.so.segment_sum(occ.astype(F), i[sel], case["I"]), G, E, n, rows)
        c_ref = got[False]
        lim = R.limit_from(c_ref)
        print("%s: sign(0) = 0 reaches %s, sign(0) = 1 %s" % (case["id"], c_ref, got[True]))
        assert all(c_ref[k] <= lim[k] for k in lim)
        assert max(got[True].values()) > 1000 * max(lim.values()), (case["id"], got[True])


# ----------------------------------------------------------------------------- every copy of the head is listed
def test_every_copy_of_the_head_is_listed_with_its_test():
    """A new copy of the head (a line with log1pf(, sigmoidf_(, binary_infer( or sigmoid_xent( in csrc/*.hip, csrc/*.h)
    fails here until head_cases.HEAD_COPIES lists it with the GPU test that runs it."""
    found = C.head_lines()
    want = {k: v[0] for k, v in C.HEAD_COPIES.items()}
    assert found == want, "csrc states or calls the head on %s, HEAD_COPIES lists %s" % (found, want)
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_heads.py")).read()
    for name, (_, tests) in C.HEAD_COPIES.items():
        for t in tests:
            assert re.search(r"^def %s\(" % t, src, re.M), "%s: tests/test_gpu_heads.py has no %s" % (name, t)
    assert [k for k, v in C.HEAD_COPIES.items() if not v[1]] == ["finetune.hip"]
