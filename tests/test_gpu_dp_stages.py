"""The two stages of the data-parallel step with the real kernels, per row: two replicas with identical tables in one
process, the global batch cut in two halves, the all-reduce a torch add.

  dp_local_grads  writes [P | Q | bu | bi | loss, reg, sum g, 0]: each table's part against the float64 sum over that half
                  (tests/step_ref.step_grads) within limit_from of the float32 oracle on the same half; rows the half does
                  not touch exactly zero;
  dp_apply        on the summed buffer: m, v and w of every row follow from it (the moments and apply statements of
                  tests/step_ref.py, g = the summed buffer), bias_global from the summed sum g; the replicas stay
                  bit-identical and the buffer comes back all zero.

Two steps per case, on the tile path (k_dense_tiles with out_rows) and on the sort path (k_seg_reduce into dense_rows,
k_apply_rows' emit form), batch columns and store ids with dp_hint_next, TF1 Adam and SGD, one width per (G, VEC).
The statements are check_dp_local_grads and check_dp_apply of tests/shard_world.py."""
import time

import numpy as np
import pytest
import torch

from tfrecomm_amd import _lib as L
from tfrecomm_amd import dataparallel
from tests import shard_cases as C
from tests import shard_world as SW
from tests import step_cases as S
from tests import step_ref as R

pytestmark = pytest.mark.gpu


def _snapshot(m, adam):
    out = {}
    for name in R.NAMES:
        tid = R.TID[name]
        d = dict(w=m.get_table(tid))
        if adam:
            d["m"], d["v"] = m.get_table(tid | L.SLOT_M), m.get_table(tid | L.SLOT_V)
        out[name] = d
    return out


def _stage_store(case, reps, batches):
    """both steps' halves as rows of one store every replica holds, scattered among other rows; returns the device address
    of every replica's staged ids [step][B]"""
    U, I, B = case["U"], case["I"], case["B"]
    rs = np.random.RandomState(B)
    Ns = 4 * B + 53
    ids = rs.permutation(Ns)[:4 * B].astype(np.int64).reshape(2, 2, B)          # [step][replica][B]
    su, si = rs.randint(0, U, Ns).astype(np.int32), rs.randint(0, I, Ns).astype(np.int32)
    sr = rs.randint(1, 6, Ns).astype(np.float32)
    for s in range(2):
        for k in range(2):
            for col, x in zip((su, si, sr), batches[s]):
                col[ids[s, k]] = x[k * B:(k + 1) * B]
    base = []
    for k, be in enumerate(reps):
        be.model.upload_triples(su, si, sr)
        be.model.stage_ids(np.ascontiguousarray(ids[:, k]))
        base.append(be.model.staged_ids_devptr()[0])
    return base


def _local_grads(case, be, k, s, half, base, dev):
    """dp_local_grads of replica k on its half of step s, in the case's batch form; returns (the buffer, what must stay alive)"""
    B = case["B"]
    if case["form"] == "store":
        return be.local_grads(store_ids_ptr=base[k] + s * B * 8, batch=B, next_ids_ptr=base[k] + (s + 1) * B * 8 if s == 0 else None), None
    cols = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in half]
    return be.local_grads(*cols), cols


def _run(case, report):
    U, I, D, B = case["U"], case["I"], case["D"], case["B"]
    adam = case["opt"] == "adam"
    flags = dict(loss=case["loss"], item_abs=case["item_abs"], reg_bias=case["reg_bias"])
    lr, reg = S.hyper_of(case, 0)
    dev = torch.device("cuda", 0)
    t = C.tables_of(case)
    reps = [dataparallel.HipReplica(U, I, D, 0, optimizer=case["opt"], adam_mode=case["mode"], lr=lr, reg=reg, **flags) for _ in range(2)]
    try:
        g, vec = SW.geometry(D)
        for be in reps:
            be.model.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
            plan = ";".join("%s=%s" % kv for kv in be.model.kernel_plan(B).items())
            assert ("k_tile_step<%d, %d, " % (g, vec) in plan) == (case["path"] == "tiles"), "%s: plan %r" % (case["id"], plan)
        batches = [C.dp_batch_of(case, s) for s in range(2)]
        base = _stage_store(case, reps, batches) if case["form"] == "store" else None
        before = _snapshot(reps[0].model, adam)
        for s in range(2):
            tabs = {k: before[k]["w"] for k in R.NAMES}
            powers = reps[0].model.get_step()[1:]
            flats, keep = [], []
            for k, be in enumerate(reps):
                half = [x[k * B:(k + 1) * B] for x in batches[s]]
                flat, cols = _local_grads(case, be, k, s, half, base, dev)
                keep.append(cols)
                flats.append(flat)
                got = SW.dp_parts(flat.cpu().numpy().copy(), U, I, D)
                bad = SW.check_dp_local_grads(got, tabs, *half, s, lam=reg, report=report, tag="step%d replica%d " % (s, k), **flags)
                assert not bad, "%s, step %d, replica %d, dp_local_grads:\n  %s" % (case["id"], s, k, "\n  ".join(bad))
            # the all-reduce, then dp_apply on both replicas
            total = flats[0] + flats[1]
            gsum = SW.dp_parts(total.cpu().numpy().copy(), U, I, D)
            for be, flat in zip(reps, flats):
                flat.copy_(total)
                be.apply(flat)
            torch.cuda.synchronize()
            after = [_snapshot(be.model, adam) for be in reps]
            bad = SW.check_dp_apply(before, after[0], gsum, opt=case["opt"], lr=lr, powers=powers, fresh=s == 0)
            for name in R.NAMES:
                for slot in after[0][name]:
                    if not R.same_bits(after[0][name][slot], after[1][name][slot]):
                        bad.append("%s.%s differs between the replicas" % (name, slot))
            for k, be in enumerate(reps):
                if float(be.flat.abs().max()) != 0.0:
                    bad.append("replica %d: the buffer is not all zero after dp_apply" % k)
                if be.model.get_step()[0] != s + 1:
                    bad.append("replica %d: step counter %d after step %d" % (k, be.model.get_step()[0], s))
            assert not bad, "%s, step %d, dp_apply:\n  %s" % (case["id"], s, "\n  ".join(bad))
            before = after[0]
    finally:
        for be in reps:
            be.model.close()


@pytest.mark.parametrize("case", C.DP_CASES, ids=lambda c: c["id"])
def test_two_data_parallel_steps_stage_by_stage(case):
    t0 = time.time()
    report = {}
    try:
        _run(case, report)
    finally:
        SW.print_report(case, {"dp": report}, time.time() - t0)
