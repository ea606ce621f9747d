"""One fine-tune step of one user (csrc/finetune.hip k_finetune, SvdModel.finetune_users) stated with the per-row machinery
of tests/step_ref.py.  NumPy only.

A round on user ``user`` with prefix L is an SVD step on the batch u = full(L, user), i = items[:L], r = rates[:L] with
everything but P and bu frozen.  With ``nsteps = 1`` and one round per user in a call, every number the call leaves behind
is a function of the tables read before it, so the call is judged by

  per user     ``step_ref.check_table`` on the user's row of P and of bu: the gradient the device used within
               ``limit_from(c_ref)`` x eps32 x E of the float64 sum (c_ref from the float32 oracle, which adds in row order
               as the kernel does), v from g and the previous v, w from the device's own m and v - with lr_t from the beta
               powers at that round's own position in the call;
  outputs      the ask logits, the round losses and the final logits over each prefix against float64 ``so.forward`` /
               ``so.data_loss`` at 2 * RTOL, scale-relative over the users judged together; NaN past each prefix;
  untouched    identical bits in every slot of a frozen table, of a user outside the call and of a user without rounds.

``execute`` is a float32 restatement of a whole call in the kernel's operation order.  tests/test_finetune_step_ref_host.py
runs the statements on it, with and without planted errors; it is never compared with the device bit for bit.

A schedule is the tuple ``finetune_users`` takes: (users, row_ptr, items, rates, round_ptr, ask, prefix, nsteps)."""
import numpy as np

from oracle import svd_oracle as so
from tests import step_ref as R
from tests import widths as W
from tests.util import RTOL, rel_err

F = np.float32
USER_TABLES = ("P", "bu")
OUT_RTOL = 2 * RTOL                              # tests/test_gpu_step_gradients.py holds logits and loss of a first step to it


# the GPU test's one-step cases (tests/test_gpu_finetune_step.py): every width of widths.FINETUNE under both optimisers; the
# loss, item_abs and reg_bias rotate across the widths (tests/test_finetune_step_ref_host.py counts what they reach)
STEP_CASES = [(D, ("mse", "nll")[(x + y) % 2], ("sgd", "lazy")[y], bool((x // 2 + y) % 2), (x + y) % 3 == 0)
              for x, D in enumerate(W.FINETUNE) for y in range(2)]


def powers_at(b1p, b2p, b1, b2, n):
    """the model's float32 beta-power recurrence, n steps on"""
    b1p, b2p, b1, b2 = np.float32(b1p), np.float32(b2p), np.float32(b1), np.float32(b2)
    for _ in range(n):
        b1p, b2p = np.float32(b1p * b1), np.float32(b2p * b2)
    return float(b1p), float(b2p)


def copy_state(st):
    return {k: {s: np.array(a, F) for s, a in d.items()} for k, d in st.items()}


def zero_state(t, adam):
    """{name: dict(w=, m=, v=)} of a fresh model holding the tables ``t`` (m, v absent under SGD)"""
    out = {}
    for k in R.NAMES:
        out[k] = dict(w=np.array(t[k], F))
        if adam:
            out[k]["m"], out[k]["v"] = np.zeros(np.shape(t[k]), F), np.zeros(np.shape(t[k]), F)
    return out


def draw_rows(rs, I, rows, binary):
    """(row_ptr, items, rates): ``rows[x]`` training rows per user, items drawn with repeats"""
    row_ptr = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
    n = int(row_ptr[-1])
    items = rs.randint(0, I, n).astype(np.int32)
    rates = (rs.rand(n) < 0.5).astype(F) if binary else rs.randint(1, 6, n).astype(F)
    return row_ptr, items, rates


def schedule(rs, users, I, drawn, prefixes, nsteps=1):
    """the schedule in which user x runs one round per entry of ``prefixes[x]`` (none for an empty list) on rows ``drawn``"""
    row_ptr, items, rates = drawn
    round_ptr = np.concatenate(([0], np.cumsum([len(p) for p in prefixes]))).astype(np.int64)
    prefix = np.asarray([n for p in prefixes for n in p], np.int32)
    ask = rs.randint(0, I, prefix.size).astype(np.int32)
    return np.asarray(users, np.int32), row_ptr, items, rates, round_ptr, ask, prefix, nsteps


def round_of(sched, x):
    """(user, k, items, rates, ask) of the single round of schedule user x over its prefix, or None without a round"""
    users, row_ptr, items, rates, round_ptr, ask, prefix, _ = sched
    k0, k1 = int(round_ptr[x]), int(round_ptr[x + 1])
    if k0 == k1:
        return None
    assert k1 == k0 + 1, "one round per user and call"
    r0, n = int(row_ptr[x]), int(prefix[k0])
    return int(users[x]), k0, np.asarray(items[r0:r0 + n], np.int64), np.asarray(rates[r0:r0 + n], F), int(ask[k0])


# ----------------------------------------------------------------------------- the statements
def check_user_step(bad, before, after, sched, x, *, adam, loss, item_abs, reg_bias, lam, lr, powers, fresh, frozen=0,
                    report=None):
    """The gradient, moments and apply statements on user x's row of P and bu.  ``powers`` = (b1p, b2p) at the position of
    the user's round; ``fresh``: the user's slots were zero before.  Appends the violated statements to ``bad``."""
    user, _, it, rt, _ = round_of(sched, x)
    tabs = {k: before[k]["w"] for k in R.NAMES}
    u = np.full(it.size, user, np.int64)
    ref, _, _ = R.step_grads(tabs, u, it, rt, loss, item_abs, reg_bias, lam)
    f32 = R.f32_oracle_grads(tabs, u, it, rt, loss, item_abs, reg_bias, lam)
    alpha = R.alpha_f32(lr, *powers) if adam else 0.0
    row = slice(user, user + 1)
    for name in USER_TABLES:
        G, E, n = ref[name]
        b, a = ({s: v[row] for s, v in d[name].items()} for d in (before, after))
        rep = {} if report is not None else None
        mine = []
        R.check_table(mine, name, G[row], E[row], n[row], b, a, f32[name][row], adam=adam, tf1=False, fresh=fresh, lr=lr,
                      alpha=alpha, frozen=frozen >> R.TID[name] & 1, report=rep)
        bad += ["user %d (%d rows): %s" % (user, it.size, s) for s in mine]
        if report is not None and rep:
            report[(user, name)] = rep[name]


def check_outputs(bad, before, sched, outs, *, loss, item_abs, groups=None):
    """ask logits, round losses and final logits of a call of one step per user against float64 on the tables the call
    started from.  ``groups``: lists of schedule users judged together, scale-relative (None = all in one) - a user with
    logits of +-25 would hide the others behind its scale."""
    users, row_ptr, items, rates, round_ptr, ask, prefix, nsteps = sched
    assert nsteps == 1
    ask_out, loss_out, final = outs
    w = R.f64_tables({k: before[k]["w"] for k in R.NAMES})
    nan_ok = np.ones(len(users), bool)
    want = {}
    for x in range(len(users)):
        r0, r1 = int(row_ptr[x]), int(row_ptr[x + 1])
        rd = round_of(sched, x)
        n = 0
        if rd is not None:
            user, k, it, rt, a = rd
            n = it.size
            both = so.forward(w["P"], w["Q"], w["bu"], w["bi"], w["mu"], np.full(n + 1, user, np.int64), np.append(it, a), item_abs)
            want[x] = (k, both[n], both[:n], so.data_loss(both[:n], rt.astype(np.float64), loss))
        if final is not None and not np.isnan(final[r0 + n:r1]).all():
            nan_ok[x] = False
    if not nan_ok.all():
        bad.append("final logits: rows past the prefix are not NaN (schedule users %s)" % np.flatnonzero(~nan_ok).tolist())
    for grp in ([sorted(want)] if groups is None else groups):
        grp = [x for x in grp if x in want]
        if not grp:
            continue
        ks = [want[x][0] for x in grp]
        e = rel_err(ask_out[ks], [want[x][1] for x in grp])
        if not e <= OUT_RTOL:
            bad.append("ask logit of schedule users %s: scale-relative error %.3e > %.1e" % (grp, e, OUT_RTOL))
        if loss_out is not None:
            e = rel_err(loss_out[ks], [want[x][3] for x in grp])
            if not e <= OUT_RTOL:
                bad.append("round loss of schedule users %s: scale-relative error %.3e > %.1e" % (grp, e, OUT_RTOL))
        if final is not None:
            got = np.concatenate([final[int(row_ptr[x]):int(row_ptr[x]) + want[x][2].size] for x in grp])
            e = rel_err(got, np.concatenate([want[x][2] for x in grp]))
            if not e <= OUT_RTOL:                           # a NaN inside a prefix lands here too
                bad.append("final logits of schedule users %s: scale-relative error %.3e > %.1e" % (grp, e, OUT_RTOL))


def check_untouched(bad, before, after, sched, frozen):
    """identical bits: every slot of a table named in ``frozen``, and in P and bu every slot of the users outside the call
    and of the users of the call without rounds"""
    users, round_ptr = np.asarray(sched[0], np.int64), np.asarray(sched[4], np.int64)
    for name in R.NAMES:
        if frozen >> R.TID[name] & 1:
            for slot in before[name]:
                if not R.same_bits(before[name][slot], after[name][slot]):
                    bad.append("%s.%s: a frozen table changed" % (name, slot))
    active = users[np.diff(round_ptr) > 0]
    idle = users[np.diff(round_ptr) == 0]
    for name in USER_TABLES:
        outside = np.ones(before[name]["w"].shape[0], bool)
        outside[users] = False
        for slot in before[name]:
            b, a = before[name][slot], after[name][slot]
            if not R.same_bits(b[outside], a[outside]):
                bad.append("%s.%s: users outside the call changed" % (name, slot))
            if not R.same_bits(b[idle], a[idle]):
                bad.append("%s.%s: users of the call without rounds changed" % (name, slot))
    return active


def check_call(before, after, sched, outs, *, adam, loss, item_abs, reg_bias, lam, lr, powers0, b1=so.BETA1, b2=so.BETA2,
               fresh, frozen, round_seq=None, groups=None, report=None):
    """Every statement about one ``finetune_users`` call of one step and at most one round per user.  ``powers0``: the
    model's beta powers before the call; round k runs at position ``round_seq[k]`` (None: k).  Returns the violated
    statements (empty = the call is right)."""
    bad = []
    check_untouched(bad, before, after, sched, frozen)
    for x in range(len(sched[0])):
        rd = round_of(sched, x)
        if rd is None:
            continue
        pos = rd[1] if round_seq is None else int(round_seq[rd[1]])
        check_user_step(bad, before, after, sched, x, adam=adam, loss=loss, item_abs=item_abs, reg_bias=reg_bias, lam=lam,
                        lr=lr, powers=powers_at(powers0[0], powers0[1], b1, b2, pos) if adam else powers0, fresh=fresh,
                        frozen=frozen, report=report)
    check_outputs(bad, before, sched, outs, loss=loss, item_abs=item_abs, groups=groups)
    for what, a in (("ask logits", outs[0]), ("round losses", outs[1])):
        if a is not None and not np.isfinite(a).all():
            bad.append("%s: not finite" % what)
    for name in USER_TABLES:
        for slot, a in after[name].items():
            if not np.isfinite(a).all():
                bad.append("%s.%s: not finite" % (name, slot))
    return bad


def print_ratios(tag, report):
    """RATIO lines as tests/test_gpu_step_gradients.py prints them, one per (user, table)"""
    for (user, name), v in sorted(report.items()):
        print("RATIO %s user %d %s dev short %.2f long %.2f | c_ref short %.2f long %.2f" % (
            tag, user, name, v["dev"]["short"], v["dev"]["long"], v["c_ref"]["short"], v["c_ref"]["long"]))


# ----------------------------------------------------------------------------- a float32 executor in the kernel's order
def _fma(a, b, c):
    """fmaf through float64: the product of two float32 is exact there, the sum rounds once and then once more"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _dot_chain(p, q):
    """s = fmaf(p_f, q_kf, s) over f ascending from +0, for every row k of q at once"""
    s = np.zeros(q.shape[0], F)
    for f in range(p.size):
        s = _fma(p[f], q[:, f], s)
    return s


def execute(st, sched, *, adam, loss, item_abs, reg_bias, lam, lr, powers0, b1=so.BETA1, b2=so.BETA2, frozen=0,
            round_seq=None, fault=None):
    """One ``finetune_users`` call in float32 NumPy in k_finetune's operation order: the fmaf chain over f ascending, the logit
    ((s + mu) + bu) + bi, g_f accumulated row by row as g += fmaf(d_k, q'_kf, lam * p_f), ``adam_sparse`` of
    csrc/svd_kernels.h.  Returns (new state, (ask, loss, final), powers after the call).

    ``fault`` plants one error: "drop_row64" (row 64 of a prefix missing from the gradient sums), "lam_once" (lam * p once
    per step), "late_powers" (lr_t from the next step's powers), "no_reg_bias" (lam * bu left out), "v_with_b1" (v decays by
    b1), "ask_no_abs" (the asked row without |.|)."""
    users, row_ptr, items, rates, round_ptr, ask, prefix, nsteps = sched
    new = copy_state(st)
    P, bu, Q, bi, mu = new["P"]["w"], new["bu"]["w"], st["Q"]["w"], st["bi"]["w"], np.reshape(st["mu"]["w"], -1).astype(F)[0]
    lam, lr, b1, b2, one = F(lam), F(lr), F(b1), F(b2), F(1)
    omb1, omb2, eps = one - b1, one - b2, F(so.EPSILON)
    n_rounds = int(round_ptr[-1])
    seq = np.arange(n_rounds) * nsteps if round_seq is None else np.asarray(round_seq)
    ask_out, loss_out = np.empty(n_rounds, F), np.empty(n_rounds, F)
    final = np.full(int(row_ptr[-1]), np.nan, F)
    fr_rows, fr_bias = frozen >> so.PF & 1, frozen >> so.BU & 1
    for x, user in enumerate(np.asarray(users, np.int64)):
        r0 = int(row_ptr[x])
        k0, k1 = int(round_ptr[x]), int(round_ptr[x + 1])
        p, b = P[user].copy(), F(bu[user])
        if adam:
            m, v = new["P"]["m"][user].copy(), new["P"]["v"][user].copy()
            bm, bv = F(new["bu"]["m"][user]), F(new["bu"]["v"][user])
        for kr in range(k0, k1):
            L = int(prefix[kr])
            it = np.asarray(items[r0:r0 + L], np.int64)
            rt = np.asarray(rates[r0:r0 + L], F)
            q = np.abs(Q[it]) if item_abs else Q[it]
            aq = Q[ask[kr]][None, :]
            if item_abs and fault != "ask_no_abs":
                aq = np.abs(aq)
            ask_out[kr] = ((_dot_chain(p, aq)[0] + mu) + b) + bi[ask[kr]]
            b1p, b2p = (F(a) for a in powers_at(powers0[0], powers0[1], b1, b2, int(seq[kr])))
            for step in range(nsteps):
                x_ = ((_dot_chain(p, q) + mu) + b) + bi[it]
                if loss == so.MSE:
                    d = x_ - rt
                    l = F(0.5) * d * d
                else:
                    d = one / (one + np.exp(-x_)) - rt
                    l = np.maximum(x_, F(0)) - x_ * rt + np.log1p(np.exp(-np.abs(x_)))
                lp, lbu = lam * p, lam * b
                g, gb = np.zeros(p.size, F), F(0)
                for kk in range(L):
                    if fault == "drop_row64" and kk == 64:
                        continue
                    g = g + _fma(d[kk], q[kk], np.zeros_like(lp) if fault == "lam_once" and kk else lp)
                    gb = gb + (d[kk] + lbu if reg_bias and fault != "no_reg_bias" else d[kk])
                if adam:
                    if fault == "late_powers":
                        alpha = lr * np.sqrt(one - b2p * b2) / (one - b1p * b1)
                    else:
                        alpha = lr * np.sqrt(one - b2p) / (one - b1p)
                    bv_ = b1 if fault == "v_with_b1" else b2
                    if not fr_rows:
                        m = _fma(m, b1, g * omb1)
                        v = _fma(v, bv_, (g * g) * omb2)
                        p = p - alpha * m / (np.sqrt(v) + eps)
                    if not fr_bias:
                        bm = _fma(bm, b1, gb * omb1)
                        bv = _fma(bv, bv_, (gb * gb) * omb2)
                        b = F(b - alpha * bm / (np.sqrt(bv) + eps))
                    b1p, b2p = F(b1p * b1), F(b2p * b2)
                else:
                    if not fr_rows:
                        p = p - lr * g
                    if not fr_bias:
                        b = F(b - lr * gb)
                if step + 1 == nsteps:
                    loss_out[kr] = np.cumsum(l, dtype=F)[-1]
                    if kr + 1 == k1:
                        final[r0:r0 + L] = x_
        if k1 > k0:
            if not fr_rows:
                P[user] = p
                if adam:
                    new["P"]["m"][user], new["P"]["v"][user] = m, v
            if not fr_bias:
                bu[user] = b
                if adam:
                    new["bu"]["m"][user], new["bu"]["v"][user] = bm, bv
    end = powers_at(powers0[0], powers0[1], b1, b2, n_rounds * nsteps) if adam else tuple(powers0)
    return new, (ask_out, loss_out, final), end
