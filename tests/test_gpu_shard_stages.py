"""Every stage of the row-sharded step with the real kernels, per row: W shards live in one process on one GPU
(tests/shard_world.py - HipShard takes device tensors and fences its own stream, and every exchange is an equal-split
all-to-all, here a reshuffle of tensor chunks).  Two successive steps per case on fresh models; after each stage the
statements of tests/shard_world.py, after the step tests/step_ref.check_step on the assembled global tables.  This reaches
what the two-process runs of tests/test_gpu_sharded.py do not: every (G, VEC, full width) class of k_gather_packed and of the
strided reduce, slots cut by a reduce-block boundary (k_apply_rows' emit form), the owner-side reduce of received rows,
and the peer error flag at both strides."""
import time

import numpy as np
import pytest
import torch

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tfrecomm_amd import sharded
from tests import shard_cases as C
from tests import shard_world as SW
from tests import step_ref as R
from tests.util import rand_tables

pytestmark = pytest.mark.gpu


def _world(case, world=None):
    lr, reg = C.hyper_of(case, 0)
    kw = dict(optimizer=case["opt"], adam_mode=case["mode"], lr=lr, reg=reg, loss=case["loss"], item_abs=case["item_abs"],
              reg_bias=case["reg_bias"])
    return SW.World(case["U"], case["I"], case["D"], world or case["world"], lambda ur, ir, d: sharded.HipShard(ur, ir, d, 0, **kw),
                    device=torch.device("cuda", 0))


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c["id"])
def test_two_sharded_steps_stage_by_stage(case):
    t0 = time.time()
    report = {}
    try:
        with _world(case) as w:
            SW.run_two_steps(w, case, C, report=report)
    finally:
        SW.print_report(case, report, time.time() - t0)


def _same_run(case, a, b, what):
    """two runs of the same two steps left the same bits: every stage output of every rank, every table and slot"""
    (recs_a, fin_a), (recs_b, fin_b) = a, b
    for s, (ra, rb) in enumerate(zip(recs_a, recs_b)):
        for key in ("req", "rows_out", "grad", "scal", "grad_recv"):
            for k in range(case["world"]):
                xa, xb = ra[key][k], rb[key][k]
                assert R.same_bits(xa, xb) if xa.dtype == np.float32 else np.array_equal(xa, xb), \
                    "%s: step %d, rank %d, %s differs (%s): %r, %r" % (case["id"], s, k, key, what, xa[:4], xb[:4])
        for k in range(case["world"]):
            n = ra["own"][k].size
            assert R.same_bits(ra["logits"][k][:n], rb["logits"][k][:n]), "%s: step %d, rank %d logits (%s)" % (case["id"], s, k, what)
    for name in R.NAMES:
        for slot in fin_a[name]:
            assert R.same_bits(fin_a[name][slot], fin_b[name][slot]), "%s: %s.%s differs (%s)" % (case["id"], name, slot, what)


@pytest.mark.parametrize("case", C.PAIR_CASES, ids=lambda c: c["id"])
def test_split_step_and_presort_leave_identical_bits(case):
    """forward_reduce on one world against forward_items + reduce_users on an identically seeded one, and presort(req_recv)
    ahead of the compute stages against none: tables, slots, logits and gradient rows bit for bit"""
    with _world(case) as wa, _world(case) as wb:
        fused = SW.run_two_steps(wa, case, C, stage_checks=False, presort=False)
        split = SW.run_two_steps(wb, case, C, stage_checks=False, presort=False, split=True)
    _same_run(case, fused, split, "forward_reduce against forward_items + reduce_users")
    with _world(case) as wc:
        pre = SW.run_two_steps(wc, case, C, stage_checks=False, presort=True, split=True)
    _same_run(case, split, pre, "with presort against without")


@pytest.mark.parametrize("D", C.VOID_WIDTHS)
def test_a_capacity_overflow_on_one_rank_voids_the_step_on_every_rank(D):
    """rank 1's sample capacity is one short of its samples (the library's own error word, as in
    test_capacity_overflow_voids_the_step_loudly): its flag rides at float D + 1 of every row it gathers, every rank adopts
    it before anything is updated - tables and slots bit-identical, sync() raising on each"""
    U, I, B, W = 300, 200, 900, 3
    rs = np.random.RandomState(D)
    t = rand_tables(rs, U, I, D)
    case = dict(U=U, I=I, D=D, world=W, opt="adam", mode="lazy", loss="mse", item_abs=False, reg_bias=False, hyper2=None)
    u, i = rs.randint(0, U, B).astype(np.int32), rs.randint(0, I, B).astype(np.int32)
    r = rs.randint(1, 6, B).astype(np.float32)
    with _world(case) as w:
        w.set_tables(t)
        before = w.snapshot(True)
        n1 = int(np.sum(u // w.per_u == 1))
        rec = w.step(u, i, r, sample_cap_of={1: n1 - 1})
        w.finish()
        for k in range(W):
            flags = rec["rows_out"][k][:, D + 1]
            assert np.all(flags == (1.0 if k == 1 else 0.0)), "rank %d gathered rows with flags %r" % (k, np.unique(flags))
            with pytest.raises(T.TfrError) as e:
                w.be[k].sync()
            assert e.value.code == L.ERR_OOB
            assert ("capacit" in str(e.value)) if k == 1 else ("another rank" in str(e.value)), str(e.value)
        after = w.snapshot(True)
        for name in R.NAMES:
            for slot in before[name]:
                assert R.same_bits(before[name][slot], after[name][slot]), "%s.%s moved in a void step" % (name, slot)
