"""Top-K from the bf16 snapshot on the device (tfr_bf16_topk / tfr_bf16_topk_dev, SvdModel.recommend_bf16*): bit for bit
against the contract where every score is exact (tests/test_bf16_topk_host.py holds the cases to that on the CPU), against
float64 on the round-tripped tables elsewhere, and the entries' state and error handling.

The tile (csrc/score_tile.h mfma_tile_dot_bf16) and the classes of widths it treats differently are restated in
tests/bf16_topk_cases.py; WIDTHS reaches every class."""
import ctypes as C_

import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import bf16_cases
from tests import bf16_topk_cases as C
from tests import sliced_cases as SC
from tests import widths as W
from tests.test_gpu_sliced_block import assert_same, check_plan
from tests.test_gpu_topk import check_oracle, make, random_excl, ref_for

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def model_from(U, I, D, t, **kw):
    m = T.SvdModel(U, I, D, **kw)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    m.snapshot_bf16()
    return m


# ---------------------------------------------------------------- 1. bit for bit on dyadic tables
@pytest.mark.parametrize("D", C.WIDTHS)
def test_exact_on_dyadic_tables(D):
    rs = np.random.RandomState(D)
    U, I = 70, 900
    for item_abs in (False, True):
        m, t = make(U, I, D, rs, item_abs=item_abs)
        assert C.dyadic_faults(t) == []
        m.snapshot_bf16()
        users = rs.randint(0, U, 40).astype(np.int32)
        for k in W.TOPK_KS:
            for with_excl in (False, True):
                ex, rows = random_excl(rs, users.size, I) if with_excl else (None, None)
                items, scores = m.recommend_bf16(users, k, exclude=ex)
                wi, ws = ref_for(m, t, users, k, rows)
                what = "D %d k %d item_abs %d excl %d" % (D, k, item_abs, with_excl)
                assert_same((items, scores), (wi, ws), what)
                fi, fs = m.recommend(users, k, exclude=ex)
                assert np.array_equal(fi, items) and np.array_equal(bits(fs), bits(scores)), what
        m.close()


# ---------------------------------------------------------------- 2. the block's hard paths
@pytest.mark.parametrize("c", SC.CASES, ids=repr)
def test_sliced_cases_on_round_tripped_tables(c):
    check_plan(c)
    t = c.tables()
    m = model_from(SC.NU, c.I, c.D, t)
    got = m.recommend_bf16(c.rows(), c.k, exclude=c.excl_csr())
    m.close()
    assert_same(got, C.sliced_expected(c.name), c.name)


# ---------------------------------------------------------------- 3. the missing half fragment leaks nothing
@pytest.mark.parametrize("item_abs,planted", [(False, np.inf), (True, -np.inf)])
@pytest.mark.parametrize("D", [8, 17, 100])
def test_no_nan_from_the_missing_half_fragment(D, item_abs, planted):
    """NF is odd: the upper half-wave's loads of the last step are aimed at the row's first fragment, which here holds an
    infinity on the item side.  Zeroing one operand alone would give 0 * inf = NaN in every score of such a tile."""
    assert C.tile_class(D)[0]
    rs = np.random.RandomState(300 + D)
    U, I, k = 70, 900, 100
    t = C.dyadic_tables(rs, U, I, D)
    t["P"][:, 0] = np.abs(t["P"][:, 0]) + np.float32(0.125)
    hot = np.sort(rs.choice(I, 37, replace=False))
    t["Q"][hot, 0] = planted
    m = model_from(U, I, D, t, item_abs=item_abs)
    users = rs.randint(0, U, 40).astype(np.int32)
    for with_excl in (False, True):
        ex, rows = random_excl(rs, users.size, I) if with_excl else (None, None)
        items, scores = m.recommend_bf16(users, k, exclude=ex)
        with np.errstate(invalid="ignore"):
            wi, ws = ref_for(m, t, users, k, rows)
        assert_same((items, scores), (wi, ws), "D %d excl %d" % (D, with_excl))
        assert np.all(items >= 0) and not np.isnan(scores).any()      # no row lost items to NaN
        for r in range(users.size):
            lead = hot if rows is None else hot[~np.isin(hot, rows[r])]
            assert np.array_equal(items[r, :lead.size], lead) and np.all(scores[r, :lead.size] == np.inf)
            assert np.all(np.isfinite(scores[r, lead.size:]))
    m.close()


# ---------------------------------------------------------------- 4. random tables
def test_random_tables_ml1m_shape():
    rs = np.random.RandomState(3)
    U, I, D, k = 6040, 3706, 64, 10
    m, t = make(U, I, D, rs, dyad=False)
    m.snapshot_bf16()
    snap = bf16_cases.snapshot_tables(t)
    users = np.arange(0, U, 7, dtype=np.int32)
    ex, rows = random_excl(rs, users.size, I, 0.05)
    items, scores = m.recommend_bf16(users, k, exclude=ex)
    fw = m.forward_bf16(np.repeat(users, k), items.reshape(-1)).reshape(users.size, k)
    S64 = snap["P"].astype(np.float64)[users] @ snap["Q"].astype(np.float64).T + float(t["mu"]) \
        + t["bu"].astype(np.float64)[users][:, None] + t["bi"].astype(np.float64)[None, :]
    tol = 1e-5 * np.abs(S64).max()
    err = np.abs(scores - np.take_along_axis(S64, items.astype(np.int64), 1)).max()
    print("largest score error %.3g = %.3f of the tolerance %.3g; against forward_bf16 %.3g = %.3f of 1e-5 max|score|" % (
        err, err / tol, tol, np.abs(fw - scores).max(), np.abs(fw - scores).max() / (1e-5 * np.abs(scores).max())))
    check_oracle(m, snap, users, items, scores, k, rows)
    assert np.abs(fw - scores).max() <= 1e-5 * np.abs(scores).max()
    m.close()


# ---------------------------------------------------------------- 5. composition
def test_bit_identical_across_batches_chunks_and_queue_sizes():
    rs = np.random.RandomState(4)
    U, I, D, k = 300, 200, 64, 10
    m, t = make(U, I, D, rs, dyad=False)
    m.snapshot_bf16()
    lds, upb, sl, ch = C_.c_int64(), C_.c_int32(), C_.c_int32(), C_.c_int64()
    n3 = 2 * 65536 + 100
    L.check(L.load().tfr_topk_plan(D, k, n3, I, C_.byref(lds), C_.byref(upb), C_.byref(sl), C_.byref(ch)))
    assert n3 > 2 * ch.value
    u0 = np.int32(17)
    alone = m.recommend_bf16([u0], k)
    b7 = np.array([3, u0, 9, 250, u0, 0, 299], np.int32)
    in7 = m.recommend_bf16(b7, k)
    big = rs.randint(0, U, 5000).astype(np.int32)
    big[[5, 999, 4321]] = u0
    in5000 = m.recommend_bf16(big, k)
    huge = rs.randint(0, U, n3).astype(np.int32)
    pos = [3, ch.value + 11, 2 * ch.value + 50]
    huge[pos] = u0
    inhuge = m.recommend_bf16(huge, k)
    for it, sc in [(in7[0][[1, 4]], in7[1][[1, 4]]), (in5000[0][[5, 999, 4321]], in5000[1][[5, 999, 4321]]),
                   (inhuge[0][pos], inhuge[1][pos])]:
        for r in range(it.shape[0]):
            assert np.array_equal(it[r], alone[0][0])
            assert np.array_equal(bits(sc[r]), bits(alone[1][0]))
    uniq = np.unique(huge[:64])
    ref = m.recommend_bf16(uniq, k)
    lut = {int(u): r for r, u in enumerate(uniq)}
    for r in range(64):
        assert np.array_equal(inhuge[0][r], ref[0][lut[int(huge[r])]])
        assert np.array_equal(bits(inhuge[1][r]), bits(ref[1][lut[int(huge[r])]]))
    # k = 10 runs k_topk_score_bf16<32, 256>, k = 200 <16, 512>: the same scores, so the short list is the long one's start
    assert W.TOPK_KS and (10 + 128 <= 256 < 200 + 128)
    long_i, long_s = m.recommend_bf16(b7, 200)
    assert np.array_equal(long_i[:, :k], in7[0]) and np.array_equal(bits(long_s[:, :k]), bits(in7[1]))
    again = m.recommend_bf16(b7, 200)
    assert np.array_equal(again[0], long_i) and np.array_equal(bits(again[1]), bits(long_s))
    m.close()


# ---------------------------------------------------------------- 6. device entry
def test_device_variant_equals_host():
    import torch
    rs = np.random.RandomState(9)
    U, I = 500, 2000
    m, t = make(U, I, 64, rs, dyad=False)
    m.snapshot_bf16()
    users = rs.randint(0, U, 300).astype(np.int32)
    ex, rows = random_excl(rs, users.size, I)
    hi, hs = m.recommend_bf16(users, 25, exclude=ex)
    dev = torch.device("cuda", 0)
    di, ds = m.recommend_bf16_dev(torch.from_numpy(users).to(dev), 25,
                                  exclude=(torch.from_numpy(ex[0]).to(dev), torch.from_numpy(ex[1]).to(dev)))
    m.sync()
    only = m.recommend_bf16_dev(torch.from_numpy(users).to(dev), 25, return_scores=False)
    m.sync()
    assert np.array_equal(di.cpu().numpy(), hi)
    assert np.array_equal(bits(ds.cpu().numpy()), bits(hs))
    assert np.array_equal(only.cpu().numpy(), m.recommend_bf16(users, 25, return_scores=False))
    for r in range(users.size):
        assert not set(hi[r].tolist()) & set(rows[r].tolist())
    m.close()


# ---------------------------------------------------------------- 7. state and errors
def test_no_snapshot_is_a_state_error_also_for_zero_users():
    rs = np.random.RandomState(20)
    m, t = make(20, 30, 16, rs)
    lib = L.load()
    items = np.full((2, 4), 77, np.int32)
    u = np.array([0, 1], np.int32)

    def refused():
        for n in (2, 0):
            assert lib.tfr_bf16_topk(m._h, L.ptr_i32(u), n, 4, None, None, L.ptr_i32(items), None) == L.ERR_STATE
            assert "tfr_bf16_snapshot" in L.last_error()
            assert lib.tfr_bf16_topk_dev(m._h, None, n, 4, None, None, None, None) == L.ERR_STATE
            assert "tfr_bf16_snapshot" in L.last_error()
        with pytest.raises(T.TfrError) as e:
            m.recommend_bf16(u, 4)
        assert e.value.code == L.ERR_STATE and "tfr_bf16_snapshot" in str(e.value)
        assert np.all(items == 77)

    refused()
    m.snapshot_bf16()
    assert m.recommend_bf16(np.zeros(0, np.int32), 5)[0].shape == (0, 5)
    wi, ws = ref_for(m, t, u, 4)
    assert_same(m.recommend_bf16(u, 4), (wi, ws), "after a snapshot")
    m.drop_bf16()
    refused()
    assert_same(m.recommend(u, 4), (wi, ws), "the float32 entry after the refusals")
    m.close()


def test_errors_and_model_still_works():
    rs = np.random.RandomState(6)
    m, t = make(20, 30, 16, rs)
    m.snapshot_bf16()
    lib = L.load()
    items = np.full((2, 4), 77, np.int32)
    good = np.array([0, 1], np.int32)
    want = ref_for(m, t, good, 4)

    def still_works():
        assert np.all(items == 77)
        assert_same(m.recommend_bf16(good, 4), want, "after a refusal")

    u = np.array([0, 20], np.int32)
    assert lib.tfr_bf16_topk(m._h, L.ptr_i32(u), 2, 4, None, None, L.ptr_i32(items), None) == L.ERR_OOB
    still_works()
    ip, bad = np.array([0, 1, 2], np.int64), np.array([3, 30], np.int32)
    assert lib.tfr_bf16_topk(m._h, L.ptr_i32(good), 2, 4, L.ptr_i64(ip), L.ptr_i32(bad), L.ptr_i32(items), None) == L.ERR_OOB
    still_works()
    ip, uns = np.array([0, 0, 2], np.int64), np.array([5, 3], np.int32)
    assert lib.tfr_bf16_topk(m._h, L.ptr_i32(good), 2, 4, L.ptr_i64(ip), L.ptr_i32(uns), L.ptr_i32(items), None) == L.ERR_ARG
    still_works()
    for k in (0, 257, -1):
        assert lib.tfr_bf16_topk(m._h, L.ptr_i32(good), 2, k, None, None, L.ptr_i32(items), None) == L.ERR_ARG
    still_works()
    import torch
    dev = torch.device("cuda", 0)
    du = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    with pytest.raises(L.TfrError) as e:
        m.recommend_bf16_dev(du, 4, exclude=(torch.tensor([0, 0, 2], device=dev), torch.tensor([5, 3], dtype=torch.int32, device=dev)))
        m.sync()
    assert e.value.code == L.ERR_ARG
    with pytest.raises(L.OutOfRangeError):
        m.recommend_bf16_dev(du, 4, exclude=(torch.tensor([0, 1, 2], device=dev), torch.tensor([3, 30], dtype=torch.int32, device=dev)))
        m.sync()
    with pytest.raises(L.OutOfRangeError):
        m.recommend_bf16_dev(torch.tensor([0, 25], dtype=torch.int32, device=dev), 4)
        m.sync()
    still_works()
    logits, _, _ = m.train_step([0, 1], [2, 3], [1.0, 2.0])
    assert np.all(np.isfinite(logits))
    still_works()                                          # a training step does not move the snapshot
    m.close()


def test_the_snapshot_answers_until_another_snapshot():
    rs = np.random.RandomState(21)
    U, I, D, k = 70, 900, 24, 10
    m, t = make(U, I, D, rs)
    m.snapshot_bf16()
    users = rs.randint(0, U, 40).astype(np.int32)
    first = ref_for(m, t, users, k)
    assert_same(m.recommend_bf16(users, k), first, "first snapshot")
    t2 = C.dyadic_tables(rs, U, I, D)
    m.set_tables(t2["mu"], t2["bu"], t2["bi"], t2["P"], t2["Q"])
    second = ref_for(m, t2, users, k)
    assert not np.array_equal(first[0], second[0])
    assert_same(m.recommend_bf16(users, k), first, "after set_tables the snapshot still answers")
    assert_same(m.recommend(users, k), second, "the float32 entry reads the new tables")
    m.snapshot_bf16()
    assert_same(m.recommend_bf16(users, k), second, "second snapshot")
    m.close()


def test_state_untouched_and_training_unchanged():
    rs = np.random.RandomState(7)
    U, I, D = 200, 300, 32
    batches = [(rs.randint(0, U, 500), rs.randint(0, I, 500), rs.randint(1, 6, 500).astype(np.float32)) for _ in range(4)]
    res = []
    for interleave in (False, True):
        m, t = make(U, I, D, np.random.RandomState(70), dyad=False, adam_mode="lazy")
        if interleave:
            m.snapshot_bf16()
        for b, (u, i, r) in enumerate(batches):
            m.train_step(u, i, r)
            if interleave:
                ids = [L.MU, L.BU, L.BI, L.P, L.Q] + [w | s for w in (L.MU, L.BU, L.BI, L.P, L.Q) for s in (L.SLOT_M, L.SLOT_V)]
                before = {w: m.get_table(w).copy() for w in ids}
                step = m.get_step()
                m.recommend_bf16(np.arange(0, U, 3), 20, exclude=T.rated_matrix(u, i, U, I))
                for w in ids:
                    assert np.array_equal(m.get_table(w).view(np.uint32), before[w].view(np.uint32)), w
                assert m.get_step() == step
        res.append({w: m.get_table(w) for w in (L.MU, L.BU, L.BI, L.P, L.Q)})
        m.close()
    for w in res[0]:
        assert np.array_equal(res[0][w].view(np.uint32), res[1][w].view(np.uint32))
