"""The instantiations of the gather-dot forward (csrc/forward_body.h) that a small table never reaches: the non-temporal
user-row loads of k_forward<G, VEC, MODE, 4, true> and k_forward_bf16<G, MODE, UNR, true>, and the LDS-staged group sum.

Each test first reads tfr_forward_plan, which answers by the functions the launch calls, so that it knows which kernel it
ran.  Cases: tests/forward_cases.py (held to their claims on the CPU by tests/test_forward_paths_host.py); widths:
tests/widths.py FORWARD_PNT and BF16_PNT (tests/test_width_coverage.py).  User tables sit one row above 256 MB with 40 rows
filled - row 0, row U - 1, the rows around the 2^28-byte offset, the rest spread - and every other row zero.

The exact case (tests/bf16_cases.py) has one right answer in float32 whatever the order of the sums, so the float64 values
are compared bit for bit.  The random case is compared with the float64 oracle at the forward's tolerance (tests/util.py
RTOL), and between two kernels that add the same numbers in the same order bit for bit."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import bf16_cases as BC
from tests import forward_cases as F
from tests import widths as W
from tests.util import RTOL, assert_close, make_oracle, rand_tables

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = BC.EXACT_TABLES


def model_from(U, I, D, t, **kw):
    kw.setdefault("optimizer", "sgd")                      # no Adam slots next to a 256 MB table
    m = T.SvdModel(U, I, D, **kw)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    return m


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def forward_from_device_ids(m, u, i, snapshot=False):
    import torch
    du, di = torch.from_numpy(np.ascontiguousarray(u)).cuda(), torch.from_numpy(np.ascontiguousarray(i)).cuda()
    out = torch.full((len(u),), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    (m.forward_bf16_dev if snapshot else m.forward_dev)(du.data_ptr(), di.data_ptr(), len(u), out.data_ptr())
    m.sync()
    return out.cpu().numpy()


def assert_plan(D, U, rows, B, pnt):
    """INFER and EVAL of this shape launch the PNT (or the plain) instantiation of the width's geometry"""
    for mode in (F.INFER, F.EVAL):
        name, args, grid = F.plan(D, U, mode, rows, B)
        if rows == F.F32:
            assert (name, args) == ("k_forward", F.geometry(D) + (mode, 4, pnt)), (D, U, mode, name, args)
        else:
            g = BC.lanes(D)
            assert (name, args) == ("k_forward_bf16", (g, mode, BC.unroll(g), pnt)), (D, U, mode, name, args)
    return grid


def alternate(listed, D, bit=0):
    return bool((listed.index(D) >> bit) & 1)


class bf16_pnt_env:
    """TFR_BF16_PNT for the length of a with block (the library reads it at every launch)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("TFR_BF16_PNT")
        if self.value is None:
            os.environ.pop("TFR_BF16_PNT", None)
        else:
            os.environ["TFR_BF16_PNT"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("TFR_BF16_PNT", None)
        else:
            os.environ["TFR_BF16_PNT"] = self.old


def check_random(got, ev, evb, t, u, i, r, D, loss, item_abs, what):
    """logits and evaluation of the random case against the float64 oracle on the compact tables"""
    orc = make_oracle(t["P"].shape[0], t["Q"].shape[0], D, t, loss=loss, item_abs=item_abs)
    x, inf = orc.forward(u, i), orc.infer(u, i)
    assert_close(got, x, what="%s D %d logits" % (what, D))
    want_sse, want_neq = float(np.sum((inf - r) ** 2)), int(np.sum(inf == r))
    sse, neq = ev[0], ev[1]
    print("%s D %d %s: sse %r want %r, neq %d want %d" % (what, D, loss, sse, want_sse, neq, want_neq))
    if loss == "mse":
        assert abs(sse - want_sse) <= RTOL * want_sse and neq == want_neq
    else:
        # no logit within 1e-4 of 0 (tests/test_forward_paths_host.py): the rounded sigmoid cannot flip, the counts are exact
        assert sse == want_sse and neq == want_neq
        want_nll = F.nll_sum(x, r)
        nll = ev[2] if evb is None else evb["mean_nll"] * len(u)
        print("    nll %r want %r" % (nll, want_nll))
        assert abs(nll - want_nll) <= RTOL * want_nll
        if evb is not None:
            assert evb["acc"] == want_neq / len(u)


# ---------------------------------------------------------------- 1. float32 rows, non-temporal: the exact case
@pytest.mark.parametrize("D", W.FORWARD_PNT)
def test_float32_pnt_is_exact_on_a_table_above_256_mb(D):
    item_abs = alternate(W.FORWARD_PNT, D)
    U = F.pnt_rows(D, 4 * D)
    big, u, i, r, want, want_sse, want_neq, pos = F.exact_big_case(D, item_abs, U, 4 * D)
    assert_plan(D, U, F.F32, len(u), True)
    with model_from(U, N_ITEMS, D, big, item_abs=item_abs) as m:
        got, dev, ev = m.forward(u, i), forward_from_device_ids(m, u, i), m.eval(u, i, r)
    print("D %d U %d: sse %r want %r, neq %d want %d" % (D, U, ev[0], want_sse, ev[1], want_neq))
    assert same_bits(got, want) and same_bits(dev, want)
    assert ev == (want_sse, want_neq)


def test_float32_pnt_is_exact_past_the_2_31_byte_offset():
    """the one table of this file that is not just above 256 MB: 2 GB of rows, read either side of the offset where a
    32-bit byte offset would wrap"""
    D, item_abs = 256, False
    U = (1 << 21) + 2
    big, u, i, r, want, want_sse, want_neq, pos = F.exact_big_case(D, item_abs, U, 4 * D)
    edge = (1 << 31) // (4 * D)
    assert {edge - 1, edge, U - 1} <= set(u.tolist())
    assert_plan(D, U, F.F32, len(u), True)
    with model_from(U, N_ITEMS, D, big, item_abs=item_abs) as m:
        got, ev = m.forward(u, i), m.eval(u, i, r)
    assert same_bits(got, want) and ev == (want_sse, want_neq)


PARTIAL = [D for D in W.FORWARD_PNT if D != F.geometry(D)[0] * F.geometry(D)[1]]


@pytest.mark.parametrize("D", PARTIAL)
def test_float32_pnt_reads_nothing_past_the_end_of_a_row(D):
    """below full width the lanes with d0 >= D must not load: the row that follows each filled row is NaN here, and a
    lane that read it would carry NaN * 0 into the group's sum.  The exact case still comes out bit for bit."""
    item_abs = not alternate(W.FORWARD_PNT, D)
    U = F.pnt_rows(D, 4 * D)
    big, u, i, r, want, want_sse, want_neq, pos = F.exact_big_case(D, item_abs, U, 4 * D)
    canaries = F.plant_canaries(big, pos)
    assert len(canaries) >= 30 and not set(canaries.tolist()) & set(u.tolist()) and np.isnan(big["P"][canaries]).all()
    assert_plan(D, U, F.F32, len(u), True)
    with model_from(U, N_ITEMS, D, big, item_abs=item_abs) as m:
        got, ev = m.forward(u, i), m.eval(u, i, r)
    assert not np.isnan(got).any(), "a lane read past its row: %d logits are NaN" % int(np.isnan(got).sum())
    assert same_bits(got, want) and ev == (want_sse, want_neq)


# ---------------------------------------------------------------- 2. float32 rows: PNT == plain, random
@pytest.mark.parametrize("D", W.FORWARD_PNT)
def test_float32_pnt_equals_the_plain_loads_bit_for_bit(D):
    """two models with the same rows, one exactly at 256 MB (plain loads) and one a row above (non-temporal): the loads
    differ in nothing but the cache policy, so logits and evaluation are the same bits; both against the oracle"""
    item_abs = alternate(W.FORWARD_PNT, D, 1)
    U1 = F.pnt_rows(D, 4 * D)
    U0 = U1 - 1
    for loss in ("mse", "nll"):
        t, uc, i, r = F.random_case(D, loss, item_abs)
        big1, u, pos = F.embed(t, uc, U1, 4 * D, spread_over=U0)       # rows of the smaller table: both models hold them
        assert pos[-1] == U0 - 1 and (U0 - 1) in u
        big = dict(big1, P=big1["P"][:U0], bu=big1["bu"][:U0])
        out = []
        for U, tables, pnt in ((U0, big, False), (U1, big1, True)):
            assert_plan(D, U, F.F32, len(u), pnt)
            with model_from(U, F.RANDOM_I, D, tables, loss=loss, item_abs=item_abs) as m:
                out.append((m.forward(u, i), m.eval(u, i, r), m.eval_binary(u, i, r) if loss == "nll" else None))
        (g0, e0, b0), (g1, e1, b1) = out
        assert same_bits(g0, g1) and e0 == e1
        if loss == "nll":
            assert b0 == b1 and not np.isnan(b0["auc"])
        for g, e, b, what in ((g0, e0, b0, "plain"), (g1, e1, b1, "non-temporal")):
            check_random(g, e, b, t, uc, i, r, D, loss, item_abs, what)


# ---------------------------------------------------------------- 3. grid stride under PNT
@pytest.mark.parametrize("D", F.GRID_STRIDE)
def test_grid_stride_under_pnt(D):
    pb = F.per_block(D)
    B = F.INFER_CAP * pb + 1                               # one rating into the second turn of the 8192 blocks
    Be = F.EVAL_CAP * pb * 2 + 1                           # EVAL: two turns of its 2048 blocks and one rating
    U = F.pnt_rows(D, 4 * D)
    t, uc, i, r = F.random_case(D, "mse", B=B)
    big, u, pos = F.embed(t, uc, U, 4 * D)
    assert assert_plan(D, U, F.F32, Be, True) == F.EVAL_CAP and F.plan(D, U, F.INFER, F.F32, B)[2] == F.INFER_CAP
    assert F.plan(D, U, F.INFER, F.F32, B - 1)[2] == F.INFER_CAP and F.plan(D, U, F.INFER, F.F32, B - 1 - pb)[2] == F.INFER_CAP - 1
    alone_at = (0, F.INFER_CAP * pb - 1, B - 1)
    with model_from(U, F.RANDOM_I, D, big) as m:
        got = m.forward(u, i)
        alone = np.concatenate([m.forward(u[k:k + 1], i[k:k + 1]) for k in alone_at])
        sse, neq = m.eval(u[:Be], i[:Be], r[:Be])
    x = make_oracle(N_USERS, F.RANDOM_I, D, t).forward(uc, i)
    assert_close(got, x, what="D %d every logit" % D)
    assert same_bits(alone, got[list(alone_at)])
    want_sse = float(np.sum((x[:Be] - r[:Be]) ** 2))
    print("D %d: sse %r want %r neq %d" % (D, sse, want_sse, neq))
    assert abs(sse - want_sse) <= RTOL * want_sse and neq == int(np.sum(x[:Be] == r[:Be]))


# ---------------------------------------------------------------- 4. out-of-range ids under PNT
def test_out_of_range_user_ids_under_pnt_raise_and_leave_everything_as_it_was():
    D = 13
    U = F.pnt_rows(D, 4 * D)
    t, uc, i, r = F.random_case(D, "mse")
    big, u, pos = F.embed(t, uc, U, 4 * D)
    assert_plan(D, U, F.F32, len(u), True)
    lib = L.load()
    with model_from(U, F.RANDOM_I, D, big) as m:
        good, good_eval = m.forward(u, i), m.eval(u, i, r)
        for bad in (U, -1):
            ub = u.copy()
            ub[100] = bad
            out = np.full(len(u), np.float32(-77.0))
            rc = lib.tfr_forward(m._h, L.ptr_i32(ub), L.ptr_i32(i), len(u), L.ptr_f32(out))
            assert rc == L.ERR_OOB and (out == np.float32(-77.0)).all()          # the caller's buffer is not written
            with pytest.raises(T.OutOfRangeError) as e:
                m.forward(ub, i)
            assert e.value.code == L.ERR_OOB
            assert same_bits(m.forward(u, i), good)
            with pytest.raises(T.OutOfRangeError):
                m.eval(ub, i, r)
            assert m.eval(u, i, r) == good_eval
        for w, k in ((L.MU, "mu"), (L.BU, "bu"), (L.BI, "bi"), (L.P, "P"), (L.Q, "Q")):
            assert np.array_equal(m.get_table(w), big[k]), k
    check_random(good, good_eval, None, t, uc, i, r, D, "mse", False, "before the bad ids")


# ---------------------------------------------------------------- 5. snapshot rows, non-temporal
@pytest.mark.parametrize("D", W.BF16_PNT)
def test_bf16_pnt_is_exact(D):
    item_abs = alternate(W.BF16_PNT, D)
    t, u, i, r, want, want_sse, want_neq = BC.exact_reference(D, item_abs)
    with model_from(N_USERS, N_ITEMS, D, t, item_abs=item_abs) as m:
        m.snapshot_bf16()
        with bf16_pnt_env("1"):
            assert_plan(D, N_USERS, F.BF16, len(u), True)
            got, dev, ev = m.forward_bf16(u, i), forward_from_device_ids(m, u, i, snapshot=True), m.eval_bf16(u, i, r)
    print("D %d: sse %r want %r, neq %d want %d" % (D, ev[0], want_sse, ev[1], want_neq))
    assert same_bits(got, want) and same_bits(dev, want)
    assert ev == (want_sse, want_neq)


@pytest.mark.parametrize("loss", ["mse", "nll"])
@pytest.mark.parametrize("D", W.BF16_PNT)
def test_bf16_pnt_equals_the_plain_loads_bit_for_bit(D, loss):
    item_abs = alternate(W.BF16_PNT, D, 1)
    t, u, i, r = F.random_case(D, loss, item_abs)
    out = []
    with model_from(N_USERS, F.RANDOM_I, D, t, loss=loss, item_abs=item_abs) as m:
        m.snapshot_bf16()
        for flag in ("0", "1"):
            with bf16_pnt_env(flag):
                assert_plan(D, N_USERS, F.BF16, len(u), flag == "1")
                out.append((m.forward_bf16(u, i), m.eval_bf16(u, i, r)))
    (g0, e0), (g1, e1) = out
    assert same_bits(g0, g1) and e0 == e1 and len(e0) == (3 if loss == "nll" else 2)
    check_random(g1, e1, None, BC.snapshot_tables(t), u, i, r, D, loss, item_abs, "snapshot")


def test_bf16_takes_the_non_temporal_loads_by_the_rule_on_a_snapshot_above_256_mb():
    D = 256
    U = F.pnt_rows(D, F.row_bytes(D, F.BF16))
    assert U == F.pnt_rows(256, 512)
    with bf16_pnt_env(None):
        big, u, i, r, want, want_sse, want_neq, pos = F.exact_big_case(D, False, U, 512)
        assert_plan(D, U, F.BF16, len(u), True)
        assert F.plan_pnt(D, U, F.INFER, F.F32) is True    # its float32 table is 512 MB
        with model_from(U, N_ITEMS, D, big) as m:
            m.snapshot_bf16()
            got, ev, f32 = m.forward_bf16(u, i), m.eval_bf16(u, i, r), m.forward(u, i)
        assert same_bits(got, want) and same_bits(f32, want) and ev == (want_sse, want_neq)
        del big
        t, uc, i, r = F.random_case(D, "mse")
        big, u, pos = F.embed(t, uc, U, 512)
        with model_from(U, F.RANDOM_I, D, big) as m:
            m.snapshot_bf16()
            got, ev = m.forward_bf16(u, i), m.eval_bf16(u, i, r)
    check_random(got, ev, None, BC.snapshot_tables(t), uc, i, r, D, "mse", False, "snapshot above 256 MB")


def test_bf16_pnt_is_exact_past_the_2_31_byte_offset():
    """2 GB of snapshot rows (and 4 GB of float32 rows behind them), read either side of the 2^31-byte offset"""
    D = 256
    U = (1 << 22) + 2
    with bf16_pnt_env(None):
        big, u, i, r, want, want_sse, want_neq, pos = F.exact_big_case(D, False, U, 512)
        edge = (1 << 31) // 512
        assert {edge - 1, edge, U - 1} <= set(u.tolist())
        assert_plan(D, U, F.BF16, len(u), True)
        with model_from(U, N_ITEMS, D, big) as m:
            m.snapshot_bf16()
            got, ev = m.forward_bf16(u, i), m.eval_bf16(u, i, r)
    assert same_bits(got, want) and ev == (want_sse, want_neq)


# ---------------------------------------------------------------- 6. the LDS-staged group sum
TRAIN_SHAPE = (16384 + 77, 300, 3000)                      # tests/test_gpu_parity.py: the SVD_BIG shape
TRAIN_WIDTHS = (33, 100)                                   # of W.SVD_BIG: a VEC = 1 and a VEC = 4 geometry below full width


def _hex(a):
    return np.ascontiguousarray(a, np.float32).tobytes().hex()


def _unhex(s):
    return np.frombuffer(bytes.fromhex(s), np.float32)


def _train_case(D):
    U, I, B = TRAIN_SHAPE
    rs = np.random.RandomState(500 + D)
    t = rand_tables(rs, U, I, D, scale=0.3 / np.sqrt(max(D, 16) / 16))
    return t, rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32), rs.randint(1, 6, B).astype(np.float32)


def group_sum_run():
    """INFER and EVAL at the ten geometries on the exact and on the random case, and one TF1-Adam step at the SVD_BIG
    shape: one line per case.  Runs in the child with TFR_LDS_REDUCE=1 and in the parent as the process found it."""
    lines = []
    for D in W.SVD_SMALL:
        item_abs = alternate(W.SVD_SMALL, D)
        t, u, i, r, _, _, _ = BC.exact_reference(D, item_abs)
        with model_from(N_USERS, N_ITEMS, D, t, item_abs=item_abs) as m:
            logits, (sse, neq) = m.forward(u, i), m.eval(u, i, r)
        lines.append("EXACT %d %s %r %d" % (D, hashlib.sha256(logits.tobytes()).hexdigest(), sse, neq))
        loss = ("mse", "nll")[alternate(W.SVD_SMALL, D, 1)]
        t, u, i, r = F.random_case(D, loss, item_abs)
        with model_from(N_USERS, F.RANDOM_I, D, t, loss=loss, item_abs=item_abs) as m:
            logits, (sse, neq) = m.forward(u, i), m.eval(u, i, r)
            nll = m.eval_binary(u, i, r)["mean_nll"] * len(u) if loss == "nll" else 0.0
        lines.append("RANDOM %d %s %r %d %r" % (D, _hex(logits), sse, neq, nll))
    U, I, B = TRAIN_SHAPE
    for D in TRAIN_WIDTHS:
        with T.SvdModel(U, I, D, optimizer="sgd") as m:
            lines.append("PLAN sgd %d %s" % (D, ";".join("%s=%s" % kv for kv in m.kernel_plan(B).items())))
        t, u, i, r = _train_case(D)
        with model_from(U, I, D, t, optimizer="adam", adam_mode="tf1", lr=3e-3, reg=0.02) as m:
            lines.append("PLAN adam-tf1 %d %s" % (D, ";".join("%s=%s" % kv for kv in m.kernel_plan(B).items())))
            logits, lossv, regv = m.train_step(u, i, r)
        lines.append("TRAIN %d %s %r %r" % (D, _hex(logits), lossv, regv))
    return lines


def test_lds_group_sum_matches_the_float64_values_and_the_butterfly():
    """TFR_LDS_REDUCE=1 (read once per process: a fresh child) sums a group's partials through LDS in lane order instead
    of by the cross-lane butterfly.  On the exact case both orders have to give the float64 values; on the random case
    the oracle's at the forward's tolerance.

    TRAIN: a step of an SGD model at the SVD_BIG shape computes its forward inside k_seg_reduce (tfr_kernel_plan names no
    k_forward there, which the test asserts), so TRAIN does not reach k_forward on that path.  The TF1-Adam step of the
    same shape does launch k_forward<G, VEC, 1, 4, false>, so one such step runs in the child: logits, loss and
    regulariser of a first step are the forward's own sums, compared with the float64 oracle at the forward's tolerance."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFR_LDS_REDUCE="1")
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_forward_paths as X; print('\\n'.join(X.group_sum_run()))" % root
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    child = [l for l in p.stdout.decode().splitlines() if l.split(" ")[0] in ("EXACT", "RANDOM", "PLAN", "TRAIN")]
    here = group_sum_run()
    assert len(child) == len(here) == 2 * len(W.SVD_SMALL) + 3 * len(TRAIN_WIDTHS)
    for line, mine in zip(child, here):
        f = line.split(" ")
        D = int(f[2]) if f[0] == "PLAN" else int(f[1])
        if f[0] == "EXACT":
            item_abs = alternate(W.SVD_SMALL, D)
            _, _, _, _, want, want_sse, want_neq = BC.exact_reference(D, item_abs)
            want_line = "EXACT %d %s %r %d" % (D, hashlib.sha256(want.tobytes()).hexdigest(), want_sse, want_neq)
            assert line == want_line, (line, want_line)
            assert mine == want_line, (mine, want_line)    # and without the variable
        elif f[0] == "RANDOM":
            item_abs, loss = alternate(W.SVD_SMALL, D), ("mse", "nll")[alternate(W.SVD_SMALL, D, 1)]
            t, u, i, r = F.random_case(D, loss, item_abs)
            for g in (f, mine.split(" ")):
                ev = (float(g[3]), int(g[4]), float(g[5]))
                check_random(_unhex(g[2]), ev, None, t, u, i, r, D, loss, item_abs, "group sum")
        elif f[0] == "PLAN":
            assert line == mine
            g, vec = F.geometry(D)
            if f[1] == "sgd":
                assert "k_forward<" not in line and "k_seg_reduce<%d, %d, " % (g, vec) in line, line
            else:
                assert "forward=k_forward<%d, %d, 1, 4, false>" % (g, vec) in line, line
        else:
            U, I, B = TRAIN_SHAPE
            t, u, i, r = _train_case(D)
            wl, wloss, wreg = make_oracle(U, I, D, t, optimizer="adam", adam_mode="tf1", lr=3e-3, reg=0.02).train_step(u, i, r)
            for g in (f, mine.split(" ")):
                assert_close(_unhex(g[2]), wl, what="D %d step logits" % D)
                assert_close(float(g[3]), wloss, what="D %d step loss" % D)
                assert_close(float(g[4]), wreg, what="D %d step reg" % D)
