"""The cases of tests/test_gpu_heads.py as plain data: batches whose logits are known without a device, at the values where
a head that is right in its flat middle goes wrong, with the checks that hold a device's (or a stand-in's) readings against
tests/head_ref.py.  Shared with tests/test_head_ref_host.py, which runs the float32 stand-in and its mutants through the
same checks.

Every factor row the batch multiplies on one side is zero (user rows for SVD and BPR, P and Y for SVD++, V for the FM), so
a logit is ((+0 + mu) + bu) + bi with mu = level and bu, bi multiples of 2^-6 in [-0.5, 0.5] (zero for the tie probes):
exact in float32, so the pre-update logits a step returns must equal the planted ones bit for bit.  The other side's rows
are random at the usual scale: dP = g q' is a second reading of g across the row.  (+0 + -0 = +0: the probe "-0" plants
a negative zero in mu and the paths turn it into +0, as the planted value computed here in float32 does.)

reg_bias is off in every case: lam * bu would bury g at bu ~ 25."""
import os
import re
import zlib

import numpy as np

from tests import head_ref as H
from tests import step_ref as R

F = np.float32
LEVELS = (0, 1, -1, 12, -12, 17, -17, 25, -25, 80, -80, 100, -100)
TIES = (("+0", 0.0), ("-0", -0.0), ("+2^-20", 2.0 ** -20), ("-2^-20", -2.0 ** -20), ("+2^-10", 2.0 ** -10), ("-2^-10", -2.0 ** -10))
PROBES = tuple(("L%+d" % v, F(v), False) for v in LEVELS) + tuple((n, F(v), True) for n, v in TIES)
MIXES = ("mixed", "z0", "z1")            # one mixed batch (the per-example gradient), two class-pure ones (the loss sum)
NP = 70                                   # singleton probes per class: more than a wave, no multiple of a lane group
LAM, ADAM_LR, SGD_LR = 0.02, 3e-3, 2.0 ** -10
V_NORMAL = 2.0 ** -116                    # (1 - b2) g^2 at or above it: v and the roundings on the way to it are normal
QMIN = 2.0 ** -4                          # |q'| below it: g q' (1 - b1) of the +-80 levels may leave the normal range


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _steps(rs, n, tie):
    """n multiples of 2^-6 in [-0.5, 0.5]; zeros for a tie probe"""
    return np.zeros(n, F) if tie else (rs.randint(-32, 33, n) / 64.0).astype(F)


def _labels(rs, mix, n_probe, n_fill):
    if mix == "mixed":
        return np.concatenate((np.zeros(n_probe // 2), np.ones(n_probe - n_probe // 2), rs.rand(n_fill) < 0.5)).astype(F)
    return np.full(n_probe + n_fill, 1.0 if mix == "z1" else 0.0, F)


def _singletons(rs, n):
    """(2 NP distinct rows with the table's last row among them, the other rows)"""
    perm = rs.permutation(n)
    k = int(np.flatnonzero(perm == n - 1)[0])
    perm[[0, k]] = perm[[k, 0]]
    return perm[:2 * NP], perm[2 * NP:]


def _fill(rs, rest, n):
    hot = rest[:max(1, rest.size // 10)]
    return np.where(rs.rand(n) < 0.7, hot[rs.randint(0, hot.size, n)], rest[rs.randint(0, rest.size, n)])


def svd_case(model, U, I, D, B, probe, mix, item_abs=False):
    """A batch for SvdModel / SvdppModel (``model`` = "svd" / "svdpp"): 2 NP probe entries, each on a user and an item no
    other entry names, and B - 2 NP fillers on the other rows (their logits are planted just the same)."""
    name, val, tie = probe
    rs = np.random.RandomState(_seed(model, U, I, D, B, name, mix))
    t = dict(mu=F(val), bu=_steps(rs, U, tie), bi=_steps(rs, I, tie), P=np.zeros((U, D), F),
             Q=rs.normal(0, 0.3 / np.sqrt(max(D, 16) / 16), (I, D)).astype(F))
    if model == "svdpp":
        t["Y"] = np.zeros((I, D), F)
    pu, ru = _singletons(rs, U)
    pi, ri = _singletons(rs, I)
    nf = B - 2 * NP
    u = np.concatenate((pu, _fill(rs, ru, nf))).astype(np.int32)
    i = np.concatenate((pi, _fill(rs, ri, nf))).astype(np.int32)
    z = _labels(rs, mix, 2 * NP, nf)
    order = rs.permutation(B)
    u, i, z = u[order], i[order], z[order]
    x = ((F(0) + t["mu"]) + t["bu"][u]) + t["bi"][i]                   # float32 throughout, the kernels' order
    c = dict(id="%s-U%d-I%d-D%d-B%d-%s-%s" % (model, U, I, D, B, name, mix), model=model, U=U, I=I, D=D, B=B, probe=name,
             level=float(val), tie=tie, mix=mix, item_abs=item_abs, tables=t, u=u, i=i, z=z, x=x.astype(F),
             pos=np.argsort(order)[:2 * NP])
    c["a_rows"], c["b_rows"] = u[c["pos"]], i[c["pos"]]                # the probes' bu and bi slots
    q = t["Q"][c["b_rows"]]
    c["qd"] = np.abs(q) if item_abs else q                             # what the probe users' P rows multiply g with
    _assert_edges(c, (u, U, c["a_rows"]), (i, I, c["b_rows"]))
    return c


def svdpp_implicit(U, I):
    """N(u) of the SVD++ world: one to three items per user, rows strictly increasing (Y = 0: they add nothing)"""
    rows = [np.unique(np.array([k % I, (k + 7) % I, (3 * k + 1) % I][:1 + k % 3])) for k in range(U)]
    indptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def fm_case(F_, D, probe, mix, n=2 * NP):
    """n rows of 1-3 one-valued entries: a probe feature (W = 0, in this row only) and up to two bias features; V = 0."""
    name, val, tie = probe
    rs = np.random.RandomState(_seed("fm", F_, D, n, name, mix))
    pf, rest = _singletons(rs, F_)
    pf = pf[:n]
    W = _steps(rs, F_, tie)
    W[pf] = 0
    t = dict(mu=F(val), W=W, V=np.zeros((F_, D), F))
    rows = [np.concatenate(([pf[k]], rs.choice(rest, k % 3, replace=False))) for k in range(n)]
    rows = [r[rs.permutation(r.size)] for r in rows]
    indptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    z = _labels(rs, mix, n, 0)[rs.permutation(n)]
    lin = np.array([np.sum(W[r], dtype=F) for r in rows], F)
    x = (t["mu"] + lin).astype(F)
    assert np.array_equal(x.astype(np.float64), float(val) + np.array([W[r].astype(np.float64).sum() for r in rows]))
    c = dict(id="fm-F%d-D%d-n%d-%s-%s" % (F_, D, n, name, mix), model="fm", F=F_, D=D, B=n, probe=name, level=float(val),
             tie=tie, mix=mix, tables=t, csr=(indptr, indices, np.ones(indices.size, F)), z=z, x=x, pos=np.arange(n),
             a_rows=pf, b_rows=None, qd=None)
    _assert_edges(c, (indices, F_, pf))
    return c


def bpr_case(U, I, D, probe, item_abs=False, B=2 * NP):
    """B triples (u, i, j), every user, positive and negative named once; the logit is x = bi[i] - bi[j] with
    bi[i] = level / 2 + a, bi[j] = -level / 2 - b (a, b multiples of 2^-6 in [-0.25, 0.25]).  The z = 1 form throughout."""
    name, val, tie = probe
    rs = np.random.RandomState(_seed("bpr", U, I, D, B, name))
    users, _ = _singletons(rs, U)
    items = np.concatenate(_singletons(rs, I))[:2 * B]                 # I >= 4 NP
    pos_i, neg_i = items[:B], items[B:]
    half = F(val) / F(2)
    bi = _steps(rs, I, tie)
    bi[pos_i] = half + _steps(rs, B, tie) / F(2)
    bi[neg_i] = -half - _steps(rs, B, tie) / F(2)
    t = dict(mu=F(0.2), bu=_steps(rs, U, False), bi=bi, P=np.zeros((U, D), F),
             Q=rs.normal(0, 0.3 / np.sqrt(max(D, 16) / 16), (I, D)).astype(F))
    x = ((F(0) + bi[pos_i]) - (F(0) + bi[neg_i])).astype(F)
    assert np.array_equal(x.astype(np.float64), bi[pos_i].astype(np.float64) - bi[neg_i].astype(np.float64))
    q = np.abs(t["Q"]) if item_abs else t["Q"]
    c = dict(id="bpr-U%d-I%d-D%d-B%d-%s" % (U, I, D, B, name), model="bpr", U=U, I=I, D=D, B=B, probe=name, level=float(val),
             tie=tie, mix="z1", item_abs=item_abs, tables=t, u=users.astype(np.int32), i=pos_i.astype(np.int32),
             j=neg_i.astype(np.int32), z=np.ones(B, F), x=x, pos=np.arange(B), a_rows=pos_i, b_rows=neg_i,
             qd=(q[pos_i] - q[neg_i]).astype(F))                       # the kernel's float32 difference q'_i - q'_j
    _assert_edges(c, (users, U, users), (items, I, items))
    return c


def _assert_edges(c, *sides):
    """what a case was built for holds"""
    x, z, pos = c["x"], c["z"], c["pos"]
    if c["mix"] == "mixed":
        assert np.sum(z[pos] == 0) == NP and np.sum(z[pos] == 1) == NP                  # every class is present
    else:
        assert np.all(z == (1.0 if c["mix"] == "z1" else 0.0)) and pos.size == 2 * NP
    for ids, n, probes in sides:                                                         # every probe occurs once
        assert probes.size >= 2 * NP and np.all(np.bincount(ids, minlength=n)[probes] == 1)
    assert not np.any((x > 0) & (x < F(H.TIE)))                                          # infer is specified everywhere
    assert np.all(np.abs(x - F(c["level"])) <= 1)
    c["v_ok"] = v_readable(x[pos], z[pos])
    assert c["v_ok"].all() or abs(c["level"]) in (80.0, 100.0), c["id"]


def v_readable(x, z):
    """(1 - b2) g^2 of the float64 reference is exactly 0 or a normal float32 with room for its roundings: v is read"""
    w = R.OMB2 * np.asarray(H.grad(x, z), np.float64) ** 2
    return (w == 0) | (w >= V_NORMAL)


# ----------------------------------------------------------------------------- the checks of one training step
def _through_m(g):
    """a float32 gradient as it is read back from a fresh Adam slot: m = fl(g (1 - b1)), g = m / (1 - b1)"""
    return (np.asarray(g, F) * (F(1) - R.B1F)).astype(np.float64) / R.OMB1


def standin_readings(c, fast=True, mutant=None):
    """what ``check_training`` takes, from the float32 stand-in of tests/head_ref.py instead of a device"""
    x, z, pos = c["x"], c["z"], c["pos"]
    g, l, _ = H.standin(x, z, fast, mutant)
    gp = g[pos]
    out = dict(logits=x.copy(), loss=float(np.cumsum(l, dtype=F)[-1]), g_a=_through_m(gp), finite=True,
               g_b=_through_m(gp) if c["b_rows"] is not None else None,
               g_mu=float(_through_m(np.cumsum(g, dtype=F)[-1])) if c["model"] != "bpr" else None,
               v_a=((gp * gp) * (F(1) - R.B2F)).astype(F))
    if c["qd"] is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            out["g_rows"] = _through_m(gp[:, None] * c["qd"]) / c["qd"].astype(np.float64)
    return out


def check_training(c, got, report=None):
    """The statements about one fresh-slot training step on a case.  ``got``: logits (None where the step returns none),
    loss, g_a / g_b (the probes' g read from m of their two bias slots; g_b None for the FM), g_rows (from the probes'
    factor rows, divided by ``c["qd"]``; absent for the FM), g_mu (None for BPR), v_a (v of the first bias slot),
    finite.  Returns the violated statements.  The limit of each is ``step_ref.limit_from`` of what the float32 stand-in
    reaches on this very case - never of ``got``."""
    bad = []
    x, z, pos = c["x"], c["z"], c["pos"]
    ref = standin_readings(c)
    xp, zp = x[pos], z[pos]
    G, E = np.asarray(H.grad(xp, zp), np.float64), H.E_g(xp, zp)
    rep = {}

    def hold(what, dev, c_ref):
        lim = R.limit_from({"short": c_ref})["short"]
        rep[what] = dict(dev=dev, c_ref=c_ref)
        if not dev <= lim:
            bad.append("%s: %.2f x eps32 x E, limit %.1f (float32 stand-in %.2f)" % (what, dev, lim, c_ref))

    if got["logits"] is not None and not R.same_bits(got["logits"], x):
        bad.append("logits: %d of %d differ from the planted ones" % (int(np.sum(np.asarray(got["logits"], F).view(np.uint32)
                                                                               != x.view(np.uint32))), x.size))
    if got.get("g_a") is not None:                                     # (an SGD step is held to its logits, loss and finiteness)
        hold("g from m of the first bias slot", H.ratio(got["g_a"], G, E), H.ratio(ref["g_a"], G, E))
    if got.get("g_b") is not None:
        hold("g from m of the second bias slot", H.ratio(got["g_b"], G, E), H.ratio(ref["g_b"], G, E))
    if c["qd"] is not None and got.get("g_rows") is not None:
        qd = np.abs(c["qd"].astype(np.float64))
        ok = qd >= QMIN
        Gr = np.broadcast_to(G[:, None], qd.shape)[ok]
        # the product g q' rounds once more (|g|); a flush of the product or of m is TINY / |q'| and TINY / ((1 - b1) |q'|)
        Er = np.broadcast_to((E + np.abs(G))[:, None], qd.shape)[ok] + (H.TINY / H.EPS32) * 11 / qd[ok]
        hold("g from the factor row", H.ratio(np.asarray(got["g_rows"])[ok], Gr, Er), H.ratio(ref["g_rows"][ok], Gr, Er))
    if got.get("g_mu") is not None:
        Gs = float(np.sum(np.asarray(H.grad(x, z), np.float64)))
        Es = H.E_g_sum(x, z) + abs(Gs) + (H.TINY / H.EPS32) * x.size
        hold("sum of g from m of mu", H.ratio(got["g_mu"], Gs, Es), H.ratio(ref["g_mu"], Gs, Es))
    Ls = float(np.sum(np.asarray(H.loss(x, z), np.float64)))
    El = H.E_l_sum(x, z) + (H.TINY / H.EPS32) * x.size
    hold("loss", H.ratio(got["loss"], Ls, El), H.ratio(ref["loss"], Ls, El))
    if got.get("v_a") is not None:
        ok = c["v_ok"]
        ex = R.moments_excess(np.zeros(int(ok.sum())), np.asarray(got["v_a"])[ok], np.asarray(got["g_a"])[ok])
        if not ex <= 1:
            bad.append("v of the first bias slot does not follow from g (%.2f x its allowance)" % ex)
    if not got["finite"]:
        bad.append("a slot is not finite after the step")
    if report is not None:
        report.update(rep)
    return bad


# ----------------------------------------------------------------------------- evaluation: every class in one set
def eval_case(model, n, U=500, I=500, D=16):
    """One labelled set holding every probe with both labels.  mu = +0; a user's bias is its probe's value (user k carries
    probe k mod 19); items 0..49 have bias zero and serve the tie users alone, the others a multiple of 2^-6.  For the FM
    ("fm"): feature k < 19 carries probe k in W, the next 50 features are zero, a row is one probe feature and up to two
    others."""
    rs = np.random.RandomState(_seed("eval", model, n, U, I, D))
    k = len(PROBES)
    val = np.array([p[1] for p in PROBES], F)
    tie = np.array([p[2] for p in PROBES])
    z = (rs.rand(n) < 0.5).astype(F)
    if model == "fm":
        W = _steps(rs, U, False)
        W[:k], W[k:k + 50] = val, 0
        pr = rs.randint(0, k, n)
        rows = [np.concatenate(([pr[r]], rs.choice(np.arange(k, k + 50) if tie[pr[r]] else np.arange(k + 50, U), r % 3, replace=False)))
                for r in range(n)]
        indptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
        indices = np.concatenate(rows).astype(np.int32)
        lin = np.zeros(n, F)
        for j in range(3):                                             # fmaf(1, w, lin) entry by entry
            has = np.diff(indptr) > j
            lin[has] = lin[has] + W[indices[indptr[:-1][has] + j]]
        c = dict(model=model, tables=dict(mu=F(0), W=W, V=np.zeros((U, D), F)), csr=(indptr, indices, np.ones(indices.size, F)),
                 F=U, D=D, z=z, x=(F(0) + lin).astype(F), cls=pr)
    else:
        bu = val[np.arange(U) % k]
        bi = _steps(rs, I, False)
        bi[:50] = 0
        u = rs.randint(0, U, n).astype(np.int32)
        i = np.where(tie[u % k], rs.randint(0, 50, n), rs.randint(50, I, n)).astype(np.int32)
        t = dict(mu=F(0), bu=bu, bi=bi, P=np.zeros((U, D), F), Q=rs.normal(0, 0.3, (I, D)).astype(F))
        if model == "svdpp":
            t["Y"] = np.zeros((I, D), F)
        for a in (bu, bi):                                             # every planted value survives a round trip to bf16
            assert not np.any(a.view(np.uint32) & 0xFFFF)
        c = dict(model=model, tables=t, u=u, i=i, U=U, I=I, D=D, z=z, x=((F(0) + t["mu"]) + bu[u]) + bi[i], cls=u % k)
    x = c["x"]
    assert x.dtype == F and not np.any((x > 0) & (x < F(H.TIE)))
    assert {(a, b) for a, b in zip(c["cls"].tolist(), z.tolist())} == {(a, b) for a in range(k) for b in (0.0, 1.0)}
    for a in np.flatnonzero(tie):                                      # a tie probe's logit is the probe's value itself
        assert np.all(x[c["cls"] == a] == val[a])
    c["n_equal"] = int(np.sum(H.infer(x) == z))
    c["id"] = "eval-%s-n%d" % (model, n)
    return c


def standin_eval(c, fast=True, mutant=None):
    _, l, inf = H.standin(c["x"], c["z"], fast, mutant)
    return dict(n_equal=int(np.sum(inf == c["z"])), sse=float(np.sum((inf - c["z"]).astype(np.float64) ** 2)),
                nll_sum=float(np.sum(l, dtype=np.float64)))


def check_eval(c, n_equal=None, sse=None, nll_sum=None, infer=None, report=None):
    """n_equal is exactly #(infer(x_k) == z_k), sse under the nll head exactly sum (infer - z)^2 = n - n_equal, nll_sum within
    the bound of a sum of losses; ``infer``: per-example inferences.  Returns the violated statements."""
    bad = []
    n = c["x"].size
    if n_equal is not None and n_equal != c["n_equal"]:
        bad.append("n_equal: %d, the rule says %d" % (n_equal, c["n_equal"]))
    if sse is not None and sse != n - c["n_equal"]:
        bad.append("sse: %r, the rule says %d" % (sse, n - c["n_equal"]))
    if infer is not None:
        w = H.infer_wrong(infer, c["x"])
        if w.size:
            bad.append("infer: %d wrong, first at x = %r" % (w.size, float(c["x"][w[0]])))
    if nll_sum is not None:
        Ls = float(np.sum(np.asarray(H.loss(c["x"], c["z"]), np.float64)))
        El = H.E_l_sum(c["x"], c["z"]) + (H.TINY / H.EPS32) * n
        c_ref = H.ratio(standin_eval(c)["nll_sum"], Ls, El)
        dev, lim = H.ratio(nll_sum, Ls, El), R.limit_from({"short": c_ref})["short"]
        if report is not None:
            report["nll_sum"] = dict(dev=dev, c_ref=c_ref)
        if not dev <= lim:
            bad.append("nll_sum: %.2f x eps32 x E, limit %.1f" % (dev, lim))
    return bad


# ----------------------------------------------------------------------------- the training configurations
# (name, the step_cases path it must take, U, I, D, B, optimiser, Adam mode): the smallest shapes that reach each copy
SVD_CONFIGS = tuple(
    [("tile-D%d-%s" % (d, m), "tiles4", 200, 200, d, 2 * NP, "adam", m) for d in (16, 5) for m in ("tf1", "lazy")]
    + [("front-D16", "csort", 500, 500, 16, 16385, "adam", "tf1"),             # 17 tiles: the counting-sort path, k_front
       ("forward-D12", "tf1_big", 16384 + 77, 300, 12, 2 * NP, "adam", "tf1"),  # k_forward TRAIN + k_adam_dense
       ("segreduce-D16", "fused_big", 16384 + 77, 300, 16, 2 * NP, "adam", "lazy"),     # three-round loads
       ("segreduce-D20", "fused_big", 16384 + 77, 300, 20, 2 * NP, "adam", "lazy")])    # the general load form
SVD_SGD_CONFIGS = (("tile-sgd", "tiles4", 200, 200, 16, 2 * NP, "sgd", "tf1"),
                   ("front-sgd", "csort", 500, 500, 16, 16385, "sgd", "tf1"),
                   ("segreduce-sgd", "fused_big", 16384 + 77, 300, 20, 2 * NP, "sgd", "tf1"))
FM_F, FM_DIMS = 400, (16, 13)
SVDPP_WORLD, SVDPP_DIMS = (200, 200), (33, 64)
BPR_WORLD, BPR_DIMS = (300, 300), (33, 64)


def svd_cases(cfg, mixes=MIXES):
    _, _, U, I, D, B, _, _ = cfg
    return [svd_case("svd", U, I, D, B, p, mix, item_abs=bool(k & 1)) for k, p in enumerate(PROBES) for mix in mixes]


def svdpp_cases(D, mixes=MIXES):
    U, I = SVDPP_WORLD
    return [svd_case("svdpp", U, I, D, 2 * NP, p, mix, item_abs=bool(k & 1)) for k, p in enumerate(PROBES) for mix in mixes]


def fm_cases(D, mixes=MIXES):
    return [fm_case(FM_F, D, p, mix) for p in PROBES for mix in mixes]


def bpr_cases(D):
    U, I = BPR_WORLD
    return [bpr_case(U, I, D, p, item_abs=bool(k & 1)) for k, p in enumerate(PROBES)]


# ----------------------------------------------------------------------------- every copy of the head, and what runs it
# source file -> (lines that state or call the head, the tests of tests/test_gpu_heads.py that run that copy)
HEAD_COPIES = {
    "svd_kernels.h": (4, ("test_svd_training_heads", "test_svd_eval_heads")),           # sigmoidf_, binary_infer, sigmoid_xent
    "svd_kernels.hip": (4, ("test_svd_training_heads",)),                                # k_tile_step, k_seg_reduce
    "forward_body.h": (4, ("test_svd_training_heads", "test_svd_eval_heads")),          # k_front, k_forward, k_forward_bf16
    "fm_kernels.hip": (1, ("test_fm_training_heads",)),
    "fm_fit.hip": (2, ("test_fm_eval_heads",)),
    "svdpp.hip": (1, ("test_svdpp_training_heads", "test_svdpp_eval_heads")),
    "bpr.hip": (1, ("test_bpr_training_heads",)),
    # fine-tune returns no pre-update logits for its training rows: its saturated users stay under step_ref's bound
    "finetune.hip": (1, ()),
}
HEAD_WORDS = re.compile(r"log1pf\(|\bsigmoidf_\(|\bbinary_infer\(|\bsigmoid_xent\(")
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tf-recomm_amd", "csrc")


def head_lines():
    """{source file: number of lines that state or call the head} over csrc/*.hip and csrc/*.h"""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                n = sum(1 for line in f if HEAD_WORDS.search(line.split("//")[0]))
            if n:
                out[name] = n
    return out
