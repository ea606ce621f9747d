"""The stage checks of the row-sharded step (tests/shard_world.py), themselves tested on the CPU: the in-process world with
the oracle-backed stand-in passes every stage statement and equals one global oracle step; a float32 restatement of the
staged order (per-rank slot sums, added in rank order at the owner) stays inside the unchanged limit; the same
restatement with one planted fault is rejected by the check named for it; the case lists reach what they say."""
import numpy as np
import pytest

from tests import shard_cases as C
from tests import shard_world as SW
from tests import step_cases as S
from tests import step_ref as R
from tests.fake_shard_backend import OracleShard
from tests.util import make_oracle

F = np.float32
B1, B2 = float(R.B1F), float(R.B2F)                 # the float32 betas, so that "m decays by b1" is the same number on both sides


def _flags(case):
    return dict(loss=case["loss"], item_abs=case["item_abs"], reg_bias=case["reg_bias"])


def _factory(case):
    lr, reg = C.hyper_of(case, 0)

    def make(ur, ir, d):
        be = OracleShard(ur, ir, d, optimizer=case["opt"], adam_mode=case["mode"], lr=lr, reg=reg, **_flags(case))
        be.o.b1, be.o.b2 = B1, B2
        be.o.reset_optimizer()
        return be
    return make


def _cpu_world(case):
    return SW.World(case["U"], case["I"], case["D"], case["world"], _factory(case))


HOST_CASES = C.CASES                                # no case is large enough to need a reduced form on the CPU


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c["id"])
def test_cpu_world_passes_every_stage_check_and_equals_one_global_step(case):
    lr, reg = C.hyper_of(case, 0)
    ref = make_oracle(case["U"], case["I"], case["D"], C.tables_of(case), optimizer=case["opt"], adam_mode=case["mode"], lr=lr, reg=reg,
                      frozen=case["frozen"], beta1=B1, beta2=B2, **_flags(case))
    with _cpu_world(case) as w:
        recs, final = SW.run_two_steps(w, case, C, exact=SW.exact_any)
        # every sample reached exactly one rank, the owner of its user row
        own = np.concatenate(recs[1]["own"])
        assert np.array_equal(np.sort(own), np.arange(case["B"]))
    for s in range(2):
        if s == 1 and case["hyper2"]:
            ref.lr, ref.reg = case["hyper2"]
        ref.train_step(*C.batch_of(case, s))
        ref.b1p, ref.b2p = (np.float64(np.float32(x)) for x in (ref.b1p, ref.b2p))      # float32 power accumulators, as the world's
    for name in R.NAMES:
        want = ref.tables()[R.TID[name]]
        assert np.allclose(final[name]["w"], want, rtol=1e-9, atol=1e-12), name
        if case["opt"] == "adam":
            assert np.allclose(final[name]["m"], ref.slots[R.TID[name]].m, rtol=1e-9, atol=1e-15), name
            assert np.allclose(final[name]["v"], ref.slots[R.TID[name]].v, rtol=1e-9, atol=1e-18), name


# ----------------------------------------------------------------------------- the staged order in float32
def _staged32(case, rec, world, tabs, u, i, r, lam, fault=None):
    """the gradient stages restated in float32: every rank's slot sums in batch order (the float32 oracle on its samples), laid
    out in the exchange buffer; the chunks exchanged; the owner adding what it received in rank order; fresh Adam's m from
    that sum.  Returns the record with grad, grad_recv and item_side replaced.  ``fault`` plants one fault."""
    D, W, cap = case["D"], case["world"], rec["slot_cap"]
    flags = (case["loss"], case["item_abs"], case["reg_bias"], lam)
    stride = rec["grad"][0].shape[1]
    G = SW.geometry(D)[0]
    out = dict(rec)
    grad = []
    for k in range(W):
        own = rec["own"][k]
        uk, ik, rk = u[own], i[own], r[own]
        if fault == "piece" and own.size:                 # the hottest slot loses its second piece
            hot = np.flatnonzero(ik == np.bincount(ik).argmax())
            drop = hot[1024 // G: 2 * (1024 // G)]
            uk, ik, rk = (np.delete(a, drop) for a in (uk, ik, rk))
        f32 = R.f32_oracle_grads(tabs, uk, ik, rk, *flags)
        if fault == "l2_once":                            # lam q once per slot, not once per occurrence
            no_l2 = R.f32_oracle_grads(tabs, uk, ik, rk, *(flags[:3] + (0.0,)))
            touched = np.bincount(ik, minlength=case["I"]) > 0
            f32["Q"] = no_l2["Q"] + F(lam) * np.asarray(tabs["Q"], F) * touched[:, None]
        gid = SW.slot_gids(rec, k, world)
        rows = np.zeros((W * cap, stride), F)
        used = gid >= 0
        rows[used, :D] = f32["Q"][gid[used]]
        rows[used, D] = f32["bi"][gid[used]]
        if fault == "padding":
            rows[used, D + 1] = F(0.25)
        grad.append(rows)
    out["grad"] = grad
    recv = [np.concatenate([grad[w].reshape(W, cap, stride)[k] for w in range(W)]) for k in range(W)]
    out["grad_recv"] = recv
    side = []
    for k in range(W):
        sh = world.sh[k]
        n = sh.i_hi - sh.i_lo
        ids = rec["req_recv"][k].astype(np.int64)
        rows = recv[k]
        if fault == "other_slot":                         # rows added one slot further than requested
            rows = np.roll(rows, 1, axis=0)
        if fault == "rank_left_out" and W > 1:
            ids = ids.copy()
            ids[(W - 1) * cap:] = -1
        ok = ids >= 0
        gq, gb = np.zeros((n, D), F), np.zeros(n, F)
        np.add.at(gq, ids[ok], rows[ok, :D])
        np.add.at(gb, ids[ok], rows[ok, D + 1 if fault == "bias_offset" else D])
        if fault == "padding":
            np.add.at(gq[:, D - 1], ids[ok], rows[ok, D + 1])
        omb1 = F(1) - R.B1F
        side.append(dict(Q=dict(m=gq * omb1), bi=dict(m=gb * omb1)))
    out["item_side"] = side
    return out


def _restated(case, fault=None):
    """(violations by check name, global float32 figures) of the first step of a case, restated"""
    adam_case = dict(case, opt="adam", mode="lazy", frozen=0)
    lr, reg = C.hyper_of(adam_case, 0)
    tabs = C.tables_of(case)
    u, i, r = C.batch_of(case, 0)
    with _cpu_world(adam_case) as w:
        w.set_tables(tabs)
        before = w.snapshot(True)
        rec = w.step(u, i, r, form=case["form"], adam=True)
        w.finish()
        rec = _staged32(case, rec, w, tabs, u, i, r, reg, fault)
        bad = dict(
            gradient_rows=SW.check_forward(dict(rec, logits=rec["logits"], scal=rec["scal"]), before, w, u, i, r, 0, lam=reg, **_flags(case)),
            owner_sum=SW.check_apply_items(rec, before, w, opt="adam", mode="lazy", lr=lr, fresh=True, frozen=0))
        # the whole sum, split by rank: against the float64 sum over the global batch, limit from the float32 oracle on it
        ref, _, _ = R.step_grads(tabs, u, i, r, case["loss"], case["item_abs"], case["reg_bias"], reg)
        f32 = R.f32_oracle_grads(tabs, u, i, r, case["loss"], case["item_abs"], case["reg_bias"], reg)
        figures = {}
        for name in ("Q", "bi"):
            back = [R.grad_from_fresh_adam(rec["item_side"][k][name]["m"]) for k in range(case["world"]) if w.sh[k].i_hi > w.sh[k].i_lo]
            g, extra = (np.concatenate([b[j] for b in back]) for j in (0, 1))
            Gv, E, n = ref[name]
            figures[name] = (R.ratio(g, Gv, E + extra, n), R.limit_from(R.ratio(f32[name], Gv, E, n)))
    return bad, figures


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c["id"])
def test_the_staged_float32_order_stays_inside_the_unchanged_limit(case):
    """per-rank slot sums in float32, added in rank order at the owner: every stage check passes and the whole sum stays
    inside limit_from of the float32 oracle on the global batch - the limit is attainable for a sum split by rank"""
    bad, figures = _restated(case)
    assert not bad["gradient_rows"] and not bad["owner_sum"], bad
    for name, (got, lim) in figures.items():
        print("%s %s: staged float32 short %.2f long %.2f, limit %.1f / %.1f" % (case["id"], name, got["short"], got["long"], lim["short"], lim["long"]))
        assert got["short"] <= lim["short"] and got["long"] <= lim["long"], (name, got, lim)


FAULT_CASE = next(c for c in HOST_CASES if c["ids"] == "hot" and c["world"] == 3)
# fault -> (the check that must reject it, words of its message)
FAULTS = {
    "piece": ("gradient_rows", "gradient rows"),          # a cut slot that loses one piece
    "bias_offset": ("owner_sum", "bi: the owner's sum"),  # the bias gradient taken from offset D + 1 instead of D
    "other_slot": ("owner_sum", "Q: the owner's sum"),    # gradient rows added in a different slot than requested
    "rank_left_out": ("owner_sum", "the owner's sum"),    # one rank's rows left out at the owner
    "padding": ("gradient_rows", "behind the bias"),      # a non-zero padding word, added into the last feature
    "l2_once": ("gradient_rows", "Q gradient rows"),      # the L2 term once per slot instead of once per occurrence
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_rejected(fault):
    check, words = FAULTS[fault]
    bad, _ = _restated(FAULT_CASE, fault)
    print("fault %s: %s" % (fault, {k: v[:2] for k, v in bad.items()}))
    assert any(words in line for line in bad[check]), "fault %s passes the %s check: %r" % (fault, check, bad)


# ----------------------------------------------------------------------------- what the case lists reach
def test_cases_reach_what_they_name():
    from tests import widths as W
    assert {c["D"] for c in C.CASES} >= set(W.SHARD)
    assert {c["world"] for c in C.CASES} == {1, 2, 3, 4}
    for opt in C.OPTS:
        assert any((c["opt"], c["mode"]) == opt for c in C.CASES)
    assert {c["form"] for c in C.CASES} == {"route", "route_ids", "recs"}
    assert any(min(c["U"], c["I"]) < c["world"] for c in C.CASES)                  # a rank that owns no rows
    assert any(c["U"] % c["world"] and c["I"] % c["world"] for c in C.CASES)
    assert {c["ids"] for c in C.CASES} >= {"dup", "hot", "one_item", "low_users"}
    assert any(c["frozen"] == S.FROZEN_ITEM_SIDE for c in C.CASES) and any(c["frozen"] == S.FROZEN_USER_SIDE for c in C.CASES)
    assert any(c["hyper2"] for c in C.CASES) and C.PAIR_CASES
    assert {SW.geometry(D)[1] for D in C.VOID_WIDTHS} == {1, 4}


def test_a_rank_with_rows_and_no_samples():
    case = next(c for c in C.CASES if c["ids"] == "low_users")
    u, _, _ = C.batch_of(case, 0)
    per_u = -(-case["U"] // case["world"])
    assert per_u * (case["world"] - 1) < case["U"] and (u // per_u).max() < case["world"] - 1


def test_a_hot_case_turned_uniform_fails_the_whole_and_cut_assertion():
    case = next(c for c in HOST_CASES if c["ids"] == "hot")
    for ids, passes in (("hot", True), ("uniform", False)):
        c = dict(case, ids=ids)
        with _cpu_world(c) as w:
            w.set_tables(C.tables_of(c))
            rec = w.step(*C.batch_of(c, 0))
            if passes:
                SW.assert_hot(c, [rec])
            else:
                with pytest.raises(AssertionError):
                    SW.assert_hot(c, [rec])


def test_dp_cases_take_the_path_they_name():
    from tests import widths as W
    for path in ("tiles", "sort"):
        assert {c["D"] for c in C.DP_CASES if c["path"] == path} == set(W.DP)
        for form in ("columns", "store"):
            for opt in (S.ADAM_TF1, S.SGD):
                assert any(c["path"] == path and c["form"] == form and (c["opt"], c["mode"]) == opt for c in C.DP_CASES), (path, form, opt)
    for c in C.DP_CASES:
        got = S.path_of(c["U"], c["I"], c["B"], c["opt"], c["mode"])
        assert got.startswith("tiles") == (c["path"] == "tiles"), (c["id"], got)
        if c["path"] == "sort":
            assert max(c["U"], c["I"]) > S.CSORT_MAX_BINS
