"""k_tile_step and k_dense_tiles take the operands of their first load round as leading scalar kernel parameters, which the
command processor preloads into SGPRs.  The same words reach the same instructions, so nothing may change:
every case runs three steps on tiny tables (300 users x 200 items) twice - staged ids (presorted blocks, look-ahead on:
the published records come through the hoisted ``srt`` pointers) and host-fed single steps (self-sorting blocks, the
struct's words) - and holds the tables, m and v of both bit for bit against each other, and every host-fed step to the
per-row statements of tests/step_ref.py.  The batch sizes sit on the edges of the hoisted geometry (one piece, a piece
edge, a tile edge, a short last tile, the headline's 784-entry last tile) and on every NT the sweep is compiled for."""
import numpy as np
import pytest

import tfrecomm_amd as T
from tfrecomm_amd import _lib as L
from tests import step_cases as S
from tests import step_ref as R
from tests.util import dup_heavy_ids, rand_tables

pytestmark = pytest.mark.gpu

U, I, K = 300, 200, 3
FLAGS = dict(loss="mse", item_abs=False, reg_bias=False)
EDGES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 10000)
NT_OF = {4096: 4, 8192: 8, 10000: 10, 12288: 12, 16384: 16}


def _tables(D):
    return rand_tables(np.random.RandomState(100 + D), U, I, D, scale=0.3 / np.sqrt(max(D, 16) / 16))


def _batches(B, steps=K):
    rs = np.random.RandomState(B)
    return [(dup_heavy_ids(rs, U, B), dup_heavy_ids(rs, I, B), rs.randint(1, 6, B).astype(np.float32)) for _ in range(steps)]


def _snapshot(m):
    out = {}
    for name in R.NAMES:
        tid = R.TID[name]
        out[name] = dict(w=m.get_table(tid), m=m.get_table(tid | L.SLOT_M), v=m.get_table(tid | L.SLOT_V))
    return out


def _model(D, mode):
    m = T.SvdModel(U, I, D, optimizer="adam", adam_mode=mode, lr=S.ADAM_LR, reg=S.REG, **FLAGS)
    t = _tables(D)
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    return m


def _same(a, b, what):
    for name in R.NAMES:
        for slot in ("w", "m", "v"):
            assert R.same_bits(a[name][slot], b[name][slot]), "%s: %s.%s differs" % (what, name, slot)


def _host_fed(D, B, mode, bat):
    """K train_step calls (self-sorting blocks), each held to tests/step_ref.py; returns the final snapshot and the plan"""
    with _model(D, mode) as m:
        plan = ";".join("%s=%s" % kv for kv in m.kernel_plan(B).items())
        before = _snapshot(m)
        for s, (u, i, r) in enumerate(bat):
            powers = m.get_step()[1:]
            m.train_step(u, i, r)
            after = _snapshot(m)
            bad = R.check_step(before, after, u, i, r, opt="adam", mode=mode, lam=S.REG, lr=S.ADAM_LR, powers=powers, fresh=s == 0, **FLAGS)
            assert not bad, "D %d B %d %s, step %d:\n  %s" % (D, B, mode, s, "\n  ".join(bad))
            before = after
    return before, plan


def _staged(D, B, mode, bat):
    """the same batches as rows of the resident store, one train_steps_staged call (presorted blocks, look-ahead on)"""
    with _model(D, mode) as m:
        m.upload_triples(*(np.concatenate([b[c] for b in bat]) for c in range(3)))
        m.stage_ids(np.arange(len(bat) * B, dtype=np.int64))
        m.train_steps_staged(0, B, len(bat))
        return _snapshot(m)


def _both_forms(D, B, mode):
    bat = _batches(B)
    single, plan = _host_fed(D, B, mode, bat)
    _same(_staged(D, B, mode, bat), single, "D %d B %d %s: staged against host-fed" % (D, B, mode))
    return plan


@pytest.mark.parametrize("B", EDGES)
def test_hoisted_geometry_at_its_edges(B):
    plan = _both_forms(64, B, "tf1")
    assert "reduce_item=k_tile_step<16, 4, " in plan, plan


@pytest.mark.parametrize("mode", ["tf1", "lazy"])
@pytest.mark.parametrize("B", sorted(NT_OF))
def test_every_nt_of_the_sweep(B, mode):
    plan = _both_forms(64, B, mode)
    assert "apply=k_dense_tiles<16, 4, false, %d>" % NT_OF[B] in plan, plan


@pytest.mark.parametrize("B", sorted(NT_OF))
def test_every_nt_of_the_sweep_data_parallel(B):
    """the WRITE form (k_dense_tiles<.., true, NT> fills the dense gradient buffer): one replica on host-fed columns, one on
    store rows with the next batch announced (presorted, look-ahead); buffers and tables bit for bit, the host-fed
    buffer within the limits of tests/shard_world.py"""
    import torch
    from tfrecomm_amd import dataparallel
    from tests import shard_world as SW
    D = 64
    bat = _batches(B)
    dev = torch.device("cuda", 0)
    t = _tables(D)
    reps = [dataparallel.HipReplica(U, I, D, 0, optimizer="adam", adam_mode="tf1", lr=S.ADAM_LR, reg=S.REG, **FLAGS) for _ in range(2)]
    try:
        for be in reps:
            be.model.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        reps[1].model.upload_triples(*(np.concatenate([b[c] for b in bat]) for c in range(3)))
        reps[1].model.stage_ids(np.arange(K * B, dtype=np.int64))
        base = reps[1].model.staged_ids_devptr()[0]
        for s, (u, i, r) in enumerate(bat):
            tabs = {k: v["w"] for k, v in _snapshot(reps[0].model).items()}
            cols = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (u, i, r)]
            f0 = reps[0].local_grads(*cols)
            f1 = reps[1].local_grads(store_ids_ptr=base + s * B * 8, batch=B, next_ids_ptr=base + (s + 1) * B * 8 if s + 1 < K else None)
            torch.cuda.synchronize()
            g0, g1 = f0.cpu().numpy().copy(), f1.cpu().numpy().copy()
            assert R.same_bits(g0, g1), "B %d step %d: the gradient buffers differ" % (B, s)
            bad = SW.check_dp_local_grads(SW.dp_parts(g0, U, I, D), tabs, u, i, r, s, lam=S.REG, **FLAGS)
            assert not bad, "B %d step %d:\n  %s" % (B, s, "\n  ".join(bad))
            for be, f in zip(reps, (f0, f1)):
                be.apply(f)
            torch.cuda.synchronize()
            del cols
        _same(_snapshot(reps[1].model), _snapshot(reps[0].model), "B %d: store rows against host-fed columns" % B)
    finally:
        for be in reps:
            be.model.close()


@pytest.mark.parametrize("D,B,kernel", [(128, 10000, "k_tile_step<32, 4, 4>"), (128, 16384, "k_tile_step<32, 4, 4>")])
def test_four_pieces_per_block(D, B, kernel):
    """wide rows past eight tiles: the EPG = 4 instantiation the launcher takes (csrc/svd_kernels.hip tile_step_epg)"""
    plan = _both_forms(D, B, "tf1")
    assert "reduce_item=%s" % kernel in plan, plan


@pytest.mark.parametrize("B", [1000, 1025])
def test_general_form(B):
    """D = 15: rows that do not fill their lane group, the sweep's row loop"""
    plan = _both_forms(15, B, "tf1")
    assert "apply=k_dense_tiles<16, 1, false, 4>" in plan, plan


@pytest.mark.parametrize("D", [64, 15])
def test_out_of_range_id_in_the_second_tile(D):
    """the step raises and the sweep leaves every table, m and v as they were: the error word is still looked at in front
    of every table-derived address"""
    B = 2049
    bat = _batches(B)
    with _model(D, "tf1") as m:
        m.train_step(*bat[0])
        before = _snapshot(m)
        u = bat[1][0].copy()
        u[1024 + 5] = U
        with pytest.raises(IndexError):
            m.train_step(u, bat[1][1], bat[1][2])
        _same(_snapshot(m), before, "D %d: after the voided step" % D)
        m.train_step(*bat[2])                                        # and still usable
        assert not R.same_bits(_snapshot(m)["P"]["w"], before["P"]["w"])


def test_drawn_call_equals_the_same_ids_staged():
    """5 drawn steps at B = 2049: the double-buffered srt / tab pair a step reads is picked on the host and now passed as
    scalars - step k must read what step k - 1 published"""
    B, steps, N = 2049, 5, 30011
    rs = np.random.RandomState(9)
    store = (rs.randint(0, U, N).astype(np.int32), rs.randint(0, I, N).astype(np.int32), rs.randint(1, 6, N).astype(np.float32))
    got = []
    for drawn in (True, False):
        with _model(64, "tf1") as m:
            m.upload_triples(*store)
            np.random.seed(4242)
            if drawn:
                m.rng_from_numpy()
                m.train_steps_drawn(B, steps)
            else:
                m.stage_ids(np.random.randint(0, N, (steps, B)))         # one draw per step, as the device draws them
                m.train_steps_staged(0, B, steps)
            got.append(_snapshot(m))
    _same(got[0], got[1], "drawn against staged")
