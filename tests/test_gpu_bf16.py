"""The bf16 snapshot on the device: conversion bit for bit, and predict / evaluate from it against the float64 oracle fed
the round-tripped tables.  The products of two bf16 values are exact in float32 and the sum is the float32 forward's
chain, so the oracle comparison holds at the float32 forward's own tolerance (tests/util.py RTOL).

Geometry, restated from csrc/bf16_rows.h (tests/bf16_cases.py): a row of D elements sits at a stride of
DP = 8 * ceil(D / 8); a rating is spread over the smallest power of two >= DP / 8 lanes (1 ... 32), min(lanes, 4) ratings
in flight per group; a block is 4 waves."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import bf16
from tests import bf16_cases as C
from tests.util import RTOL, assert_close, dup_heavy_ids, make_oracle, rand_tables

pytestmark = pytest.mark.gpu


def model_from(U, I, D, t, **kw):
    m = T.SvdModel(U, I, D, **kw)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    return m


def snapshot_oracle(U, I, D, t, **kw):
    return make_oracle(U, I, D, C.snapshot_tables(t), **kw)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def nll_sum(x, r):
    x = np.asarray(x, np.float64)
    return float(np.sum(np.maximum(x, 0) - x * r + np.log1p(np.exp(-np.abs(x)))))


# ---------------------------------------------------------------- 1. conversion
@pytest.mark.parametrize("D", C.WIDTHS)
def test_conversion_is_pack_rows_bit_for_bit(D):
    rs = np.random.RandomState(1000 + D)
    U, I = 37, 29
    t = rand_tables(rs, U, I, D)
    t["P"], t["Q"] = C.planted_table(rs, U, D), C.planted_table(rs, I, D)
    with model_from(U, I, D, t) as m:
        m.snapshot_bf16()
        got = {L.P: m.bf16_rows(L.P), L.Q: m.bf16_rows(L.Q)}
    for which, src in ((L.P, t["P"]), (L.Q, t["Q"])):
        want, g = bf16.pack_rows(src), got[which]
        assert g.shape == want.shape == (src.shape[0], C.row_stride(D)) and g.dtype == np.uint16
        nan = np.zeros(want.shape, bool)
        nan[:, :D] = np.isnan(src)
        assert nan.sum() == C.NAN_BITS.size
        assert np.array_equal(g[~nan], want[~nan])
        assert np.isnan(bf16.from_bits(g[nan])).all() and np.array_equal(g[nan] >> 15, want[nan] >> 15)


# ---------------------------------------------------------------- 2. forward against the oracle
@pytest.mark.parametrize("item_abs", [False, True])
@pytest.mark.parametrize("D", C.WIDTHS)
def test_forward_matches_oracle_on_round_tripped_tables(D, item_abs):
    U, I = 300, 200
    rs = np.random.RandomState(D * 2 + int(item_abs))
    t = rand_tables(rs, U, I, D)
    orc = snapshot_oracle(U, I, D, t, item_abs=item_abs)
    with model_from(U, I, D, t, item_abs=item_abs) as m:
        m.snapshot_bf16()
        for B in (1, 63, 257, 1000):
            u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
            got = m.forward_bf16(u, i)
            assert got.dtype == np.float32 and got.shape == (B,)
            assert_close(got, orc.forward(u, i), what="D %d B %d logits" % (D, B))


# ---------------------------------------------------------------- 2a. one body, two row types: exact agreement
@pytest.mark.parametrize("item_abs", [False, True])
@pytest.mark.parametrize("D", C.WIDTHS)
def test_float32_and_snapshot_entries_agree_bit_for_bit_on_the_exact_case(D, item_abs):
    """tests/bf16_cases.py exact_case: every partial sum is exact in float32 in any order (tests/test_bf16_host.py
    holds the inputs to that), so nothing but the float64 values can come out of either row type"""
    t, u, i, r, want, want_sse, want_neq = C.exact_reference(D, item_abs)
    U, I = C.EXACT_TABLES
    with model_from(U, I, D, t, item_abs=item_abs) as m:
        m.snapshot_bf16()
        f32, h = m.forward(u, i), m.forward_bf16(u, i)
        ev, evh = m.eval(u, i, r), m.eval_bf16(u, i, r)
    print("D %d: sse %r / %r want %r, neq %d / %d want %d" % (D, ev[0], evh[0], want_sse, ev[1], evh[1], want_neq))
    assert same_bits(f32, want) and same_bits(h, want)
    assert ev == (want_sse, want_neq) and evh == (want_sse, want_neq)


# ---------------------------------------------------------------- 3. grid stride
def test_grid_stride_infer_and_eval():
    U, I, D = 300, 200, 128
    assert C.per_block(D) == 64
    rs = np.random.RandomState(33)
    t = rand_tables(rs, U, I, D)
    orc = snapshot_oracle(U, I, D, t)
    B = 8192 * 64 + 1                                      # INFER: the 8192-block cap, one rating into the second turn
    Be = 2048 * 64 * 2 + 1                                 # EVAL: the 2048-block cap
    u, i = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
    r = rs.randint(1, 6, B).astype(np.float32)
    perm = rs.permutation(B)
    with model_from(U, I, D, t) as m:
        m.snapshot_bf16()
        got = m.forward_bf16(u, i)
        again = m.forward_bf16(u[perm], i[perm])
        sse, neq = m.eval_bf16(u[:Be], i[:Be], r[:Be])
        pe = rs.permutation(Be)
        sse_p, neq_p = m.eval_bf16(u[:Be][pe], i[:Be][pe], r[:Be][pe])
    pick = np.concatenate([rs.choice(B, 4094, replace=False), [B - 1, 8192 * 64 - 1]])
    assert_close(got[pick], orc.forward(u[pick], i[pick]), what="sampled logits")
    assert same_bits(again, got[perm])
    # the sums of EVAL are those of the logits just checked; a permuted batch adds them in another order
    want_sse = float(np.sum((got[:Be].astype(np.float64) - r[:Be]) ** 2))
    want_neq = int(np.sum(got[:Be] == r[:Be]))
    assert abs(sse - want_sse) <= RTOL * want_sse and neq == want_neq
    assert abs(sse_p - want_sse) <= RTOL * want_sse and neq_p == want_neq


# ---------------------------------------------------------------- 4. position independence
@pytest.mark.parametrize("D", [15, 128])
def test_a_pair_scores_the_same_alone_in_a_batch_and_from_device_ids(D):
    import torch
    U, I, B = 300, 200, 1000
    rs = np.random.RandomState(40 + D)
    t = rand_tables(rs, U, I, D)
    u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    with model_from(U, I, D, t) as m:
        m.snapshot_bf16()
        batch = m.forward_bf16(u, i)
        alone = np.concatenate([m.forward_bf16(u[k:k + 1], i[k:k + 1]) for k in (0, 517, B - 1)])
        du, di = torch.from_numpy(u).cuda(), torch.from_numpy(i).cuda()
        out = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m.forward_bf16_dev(du.data_ptr(), di.data_ptr(), B, out.data_ptr())
        m.sync()
        dev = out.cpu().numpy()
    assert same_bits(alone, batch[[0, 517, B - 1]])
    assert same_bits(dev, batch)


# ---------------------------------------------------------------- 5. eval
@pytest.mark.parametrize("loss", ["mse", "nll"])
def test_eval_from_the_snapshot(loss):
    U, I, D, N = C.EVAL_SHAPE
    t, u, i, r = C.eval_case(loss)
    orc = snapshot_oracle(U, I, D, t, loss=loss)
    with model_from(U, I, D, t, loss=loss) as m:
        m.snapshot_bf16()
        res = m.eval_bf16(u, i, r)
    inf = orc.infer(u, i)
    want_sse = float(np.sum((inf - r) ** 2))
    if loss == "mse":
        sse, neq = res
        print("sse %.9g want %.9g" % (sse, want_sse))
        assert abs(sse - want_sse) <= RTOL * want_sse
    else:
        sse, neq, nll = res
        x = orc.forward(u, i)
        assert np.abs(x).min() >= 1e-4                     # no logit where round(sigmoid(x)) could flip: the +-2 is never used up
        want_nll = nll_sum(x, r)
        print("neq %d want %d sse %.9g want %.9g nll %.9g want %.9g" % (neq, int(np.sum(inf == r)), sse, want_sse, nll, want_nll))
        assert abs(neq - int(np.sum(inf == r))) <= 2
        assert abs(sse - want_sse) <= 2
        assert abs(nll - want_nll) <= RTOL * N


# ---------------------------------------------------------------- 6. closeness to the float32 model
@pytest.mark.parametrize("D", [8, 64, 256])
def test_bf16_logits_stay_within_the_quantisation_bound_of_the_float32_ones(D):
    U, I, B = 300, 200, 1000
    rs = np.random.RandomState(60 + D)
    t = rand_tables(rs, U, I, D)
    u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    with model_from(U, I, D, t) as m:
        m.snapshot_bf16()
        f32, h = m.forward(u, i), m.forward_bf16(u, i)
    diff = np.abs(h.astype(np.float64) - f32)
    bound = C.QBOUND * C.sum_abs(t, u, i) + 1e-5 * np.abs(f32).max()
    print("D %d: worst %.3f of the bound" % (D, float((diff / bound).max())))
    assert (diff <= bound).all()
    assert diff.max() > 0                                  # it is the snapshot that was read


# ---------------------------------------------------------------- 7. snapshot semantics
def test_snapshot_is_a_copy_that_only_a_snapshot_moves():
    U, I, D, B = 300, 200, 20, 500
    rs = np.random.RandomState(70)
    t = rand_tables(rs, U, I, D)
    u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    r = rs.randint(1, 6, B).astype(np.float32)
    with model_from(U, I, D, t, lr=0.05) as m:
        for call in (lambda: m.forward_bf16(u, i), lambda: m.eval_bf16(u, i, r), lambda: m.bf16_rows(L.P)):
            with pytest.raises(T.TfrError) as e:
                call()
            assert e.value.code == L.ERR_STATE and "tfr_bf16_snapshot" in str(e.value)
        m.drop_bf16()                                      # nothing to drop: fine
        m.snapshot_bf16()
        first = m.forward_bf16(u, i)
        first_eval = m.eval_bf16(u, i, r)
        assert_close(first, snapshot_oracle(U, I, D, t).forward(u, i), what="first snapshot")
        m.train_step(u, i, r)
        assert same_bits(m.forward_bf16(u, i), first)
        m.set_table(L.P, t["P"] * 2)
        m.set_table(L.MU, np.float32(3.0))
        assert same_bits(m.forward_bf16(u, i), first)
        m.init_tables(seed=5, feature_stddev=0.3)
        assert same_bits(m.forward_bf16(u, i), first) and m.eval_bf16(u, i, r) == first_eval
        now = {k: m.get_table(w) for k, w in (("mu", L.MU), ("bu", L.BU), ("bi", L.BI), ("P", L.P), ("Q", L.Q))}
        m.snapshot_bf16()
        second = m.forward_bf16(u, i)
        assert_close(second, snapshot_oracle(U, I, D, now).forward(u, i), what="second snapshot")
        assert not same_bits(second, first)
        m.drop_bf16()
        with pytest.raises(T.TfrError) as e:
            m.forward_bf16(u, i)
        assert e.value.code == L.ERR_STATE


def test_snapshot_reads_item_rows_where_the_big_table_step_left_them():
    U = I = 20000                                          # above CSORT_MAX_BINS = 16384: the big-table path, second item table
    D, B = 8, 4096
    rs = np.random.RandomState(71)
    with T.SvdModel(U, I, D, optimizer="adam", adam_mode="lazy", lr=0.01) as m:
        m.init_tables(seed=3, feature_stddev=0.3)
        before = m.get_table(L.Q)
        for _ in range(2):
            m.train_step(rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32),
                         rs.randint(1, 6, B).astype(np.float32), want_logits=False)
        m.snapshot_bf16()
        rows = m.bf16_rows(L.Q)
        after = m.get_table(L.Q)
    assert not np.array_equal(before, after)
    assert np.array_equal(rows, bf16.pack_rows(after))


# ---------------------------------------------------------------- 8. errors
def test_out_of_range_ids_raise_and_leave_everything_as_it_was():
    U, I, D, B = 300, 200, 33, 257
    rs = np.random.RandomState(80)
    t = rand_tables(rs, U, I, D)
    u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    r = rs.randint(1, 6, B).astype(np.float32)
    want = snapshot_oracle(U, I, D, t).forward(u, i)
    with model_from(U, I, D, t) as m:
        m.snapshot_bf16()
        rows = m.bf16_rows(L.P), m.bf16_rows(L.Q)
        good_eval = m.eval_bf16(u, i, r)
        for col, bad in ((0, U), (0, -1), (1, I), (1, 2 ** 31 - 1)):
            ub, ib = u.copy(), i.copy()
            (ub if col == 0 else ib)[100] = bad
            with pytest.raises(T.OutOfRangeError) as e:
                m.forward_bf16(ub, ib)
            assert e.value.code == L.ERR_OOB
            assert_close(m.forward_bf16(u, i), want, what="after a bad forward")
            with pytest.raises(T.OutOfRangeError):
                m.eval_bf16(ub, ib, r)
            assert m.eval_bf16(u, i, r) == good_eval
        assert np.array_equal(m.bf16_rows(L.P), rows[0]) and np.array_equal(m.bf16_rows(L.Q), rows[1])
        for w, k in ((L.MU, "mu"), (L.BU, "bu"), (L.BI, "bi"), (L.P, "P"), (L.Q, "Q")):
            assert np.array_equal(m.get_table(w), t[k])


# ---------------------------------------------------------------- 9. determinism
@pytest.mark.parametrize("loss", ["mse", "nll"])
def test_two_calls_give_the_same_bytes(loss):
    U, I, D, B = 300, 200, 100, 30001
    rs = np.random.RandomState(90)
    t = rand_tables(rs, U, I, D)
    u, i = dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B)
    r = (rs.rand(B) < 0.5).astype(np.float32) if loss == "nll" else rs.randint(1, 6, B).astype(np.float32)
    with model_from(U, I, D, t, loss=loss) as m:
        m.snapshot_bf16()
        a, b = m.forward_bf16(u, i), m.forward_bf16(u, i)
        ea, eb = m.eval_bf16(u, i, r), m.eval_bf16(u, i, r)
    assert same_bits(a, b)
    assert ea == eb and len(ea) == (3 if loss == "nll" else 2)
