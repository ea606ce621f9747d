"""The small-table step's piece sums (k_tile_step) on batches built so that the runs of equal ids in a tile's sorted order
cover 1, 2, 15 and all 16 waves of a piece, cross piece and tile boundaries, and fill a whole tile with one id: against
the float64 oracle, look-ahead (published sort) against self-sorting single steps bit for bit, and every A/B switch of
the step (TFR_ONE_BARRIER, TFR_ITEM_SPLIT, TFR_WT) against the oracle and - where the switch only moves work between
blocks or changes how bytes are stored - bit for bit against the default."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import RTOL, assert_close, make_oracle, rand_tables, TABLE_NAMES
from tfrecomm_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIDS = (L.MU, L.BU, L.BI, L.P, L.Q)
# D = 64: 16 lanes per entry, 4 entries per wave, 64 entries (16 waves) per piece, 16 pieces per 1024-entry tile
PIECE = 64


def _tile_keys(rs, runs, n, nkeys):
    """n keys whose sorted order is the given run lengths (then random short runs), shuffled"""
    runs = list(runs)
    while sum(runs) < n:
        runs.append(int(rs.choice([1, 1, 2, 3, 5, 9])))
    runs[-1] -= sum(runs) - n
    runs = [r for r in runs if r > 0]
    assert len(runs) <= nkeys
    keys = np.sort(rs.choice(nkeys, len(runs), replace=False))
    col = np.repeat(keys, runs).astype(np.int32)
    return col[rs.permutation(n)], max(runs)


def _batch(rs, U, I, B):
    """one batch of B entries (tiles of 1024, the last one short); returns u, i, r and the longest run"""
    structures = [
        # piece 0: runs of 1 and 2 waves and one of 13; piece 1: 15 waves + singles; piece 2: all 16 waves;
        # then a run across the piece boundary at 256 and a long one across several pieces
        [4, 8, 52, 60, 1, 1, 1, 1, PIECE, 2, 100, 13, 13, 300],
        [1024],                                          # one id fills the whole tile
        [5, 63, 61, 3, 129, 65, 7, 200, 127],            # 16 and 15 waves off the piece grid, runs across pieces
    ]
    u, i, longest = [], [], 1
    for t in range((B + 1023) // 1024):
        n = min(1024, B - 1024 * t)
        ri = structures[t % 3] if n == 1024 else [n // 2, 17, 64]
        ru = structures[(t + 1) % 3] if n == 1024 else [3, n // 3, 65]
        ci, li = _tile_keys(rs, ri, n, I)
        cu, lu = _tile_keys(rs, ru, n, U)
        u.append(cu)
        i.append(ci)
        longest = max(longest, li, lu)
    r = rs.randint(1, 6, B).astype(np.float32)
    return np.concatenate(u), np.concatenate(i), r, longest


@pytest.mark.parametrize("opt,mode", [("adam", "tf1"), ("sgd", "tf1")])
def test_constructed_runs_against_the_oracle(opt, mode):
    import tfrecomm_amd as T
    U, I, D, B = 3000, 2000, 64, 3 * 1024 + 500
    rs = np.random.RandomState(77)
    t = rand_tables(rs, U, I, D, scale=0.15)
    kw = dict(optimizer=opt, adam_mode=mode, loss="mse", lr=2e-3, reg=0.03)
    orc = make_oracle(U, I, D, t, **kw)
    longest = 1
    with T.SvdModel(U, I, D, **kw) as m:
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        for s in range(3):
            u, i, r, lg = _batch(rs, U, I, B)
            longest = max(longest, lg)
            logits, lossv, regv = m.train_step(u, i, r)
            wl, wloss, wreg = orc.train_step(u, i, r)
            tol = 2 * RTOL * (s + 1)
            assert_close(logits, wl, rtol=tol, what="step %d logits" % s)
            assert_close(lossv, wloss, rtol=tol, what="step %d loss" % s)
            assert_close(regv, wreg, rtol=tol, what="step %d reg" % s)
        got, want = m.tables(), orc.tables()
    base = 2e-4 if opt == "adam" else 4 * RTOL                # the sweep's tolerances (test_gpu_parity), by the longest run
    for tid in TIDS:
        assert_close(got[tid], want[tid], rtol=base * max(1.0, np.sqrt(longest / 64.0)), what="table %s" % TABLE_NAMES[tid])


def test_constructed_runs_published_and_self_sorted_are_identical():
    """the same batches through one multi-step call (every step after the first reads the sort the previous launch
    published), through single host-fed steps (every step sorts its own tiles), and once more: same losses and
    tables, bit for bit"""
    import tfrecomm_amd as T
    U, I, D, B, K = 3000, 2000, 64, 4 * 1024 + 300, 5
    rs = np.random.RandomState(5)
    t = rand_tables(rs, U, I, D, scale=0.15)
    bat = [_batch(rs, U, I, B) for _ in range(K)]
    su = np.concatenate([b[0] for b in bat])
    si = np.concatenate([b[1] for b in bat])
    sr = np.concatenate([b[2] for b in bat])
    ids = np.arange(K * B, dtype=np.int64).reshape(K, B)
    kw = dict(optimizer="adam", adam_mode="tf1", loss="mse")
    out = []
    for form in ("published", "self", "published"):
        with T.SvdModel(U, I, D, **kw) as m:
            m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
            if form == "published":
                m.upload_triples(su, si, sr)
                m.stage_ids(ids)
                loss = np.asarray(m.train_steps_staged(0, B, K, want_loss=True), np.float32)
            else:
                loss = np.array([m.train_step(su[ids[k]], si[ids[k]], sr[ids[k]])[1] for k in range(K)], np.float32)
            tabs = m.tables()
        out.append((loss, tabs))
    for loss, tabs in out[1:]:
        assert np.array_equal(loss, out[0][0])
        for tid in TIDS:
            assert np.array_equal(tabs[tid], out[0][1][tid]), TABLE_NAMES[tid]


_SWITCH_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import tfrecomm_amd as T
from tests.test_gpu_tile_pieces import _batch
U, I, D, B, K = 6040, 3952, 64, 10000, 3                    # the headline shape: 10 tiles, 20 look-ahead sort blocks
rs = np.random.RandomState(9)
t = dict(mu=np.float32(0.2), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
         P=rs.normal(0, .15, (U, D)).astype(np.float32), Q=rs.normal(0, .15, (I, D)).astype(np.float32))
bat = [_batch(rs, U, I, B) for _ in range(K)]
with T.SvdModel(U, I, D, optimizer="adam", adam_mode="tf1", loss="mse", lr=2e-3, reg=0.03) as m:
    m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
    m.upload_triples(np.concatenate([b[0] for b in bat]), np.concatenate([b[1] for b in bat]), np.concatenate([b[2] for b in bat]))
    m.stage_ids(np.arange(K * B, dtype=np.int64).reshape(K, B))
    loss = np.asarray(m.train_steps_staged(0, B, K, want_loss=True), np.float32)
    tabs = m.tables()
np.savez(%r, loss=loss, **{"t%%d" %% k: np.asarray(v) for k, v in tabs.items()})
"""


def _run_switched(tmp_path, name, env):
    out = str(tmp_path / (name + ".npz"))
    e = dict(os.environ, **env)
    p = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT % (ROOT, out)], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    z = np.load(out)
    return z["loss"], {tid: z["t%d" % tid] for tid in TIDS}, p.stderr.decode()


def test_every_switch_setting_gives_the_same_step(tmp_path):
    base_loss, base, _ = _run_switched(tmp_path, "default", {})
    for name, env, exact in (("wt0", {"TFR_WT": "0"}, True),                    # how bytes are stored: nothing else
                             ("wt_mix", {"TFR_WT": "5"}, True),
                             ("split", {"TFR_ITEM_SPLIT": "1"}, True),           # pieces do not depend on the block split
                             ("one_barrier", {"TFR_ONE_BARRIER": "1"}, False),   # another order of the cross-wave sums
                             ("all_switched", {"TFR_WT": "0", "TFR_ITEM_SPLIT": "1", "TFR_ONE_BARRIER": "1"}, False)):
        loss, tabs, _ = _run_switched(tmp_path, name, env)
        if exact:
            assert np.array_equal(loss, base_loss), name
            for tid in TIDS:
                assert np.array_equal(tabs[tid], base[tid]), (name, TABLE_NAMES[tid])
        else:
            assert_close(loss, base_loss, rtol=6 * RTOL, what=name + " loss")
            for tid in TIDS:
                assert_close(tabs[tid], base[tid], rtol=2e-4 * 4, what="%s table %s" % (name, TABLE_NAMES[tid]))
    # and the default against the float64 oracle, at the sweep's tolerances for the longest run (1024)
    rs = np.random.RandomState(9)
    U, I, D, B, K = 6040, 3952, 64, 10000, 3
    t = dict(mu=np.float32(0.2), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
             P=rs.normal(0, .15, (U, D)).astype(np.float32), Q=rs.normal(0, .15, (I, D)).astype(np.float32))
    bat = [_batch(rs, U, I, B) for _ in range(K)]
    orc = make_oracle(U, I, D, t, optimizer="adam", adam_mode="tf1", loss="mse", lr=2e-3, reg=0.03)
    for k in range(K):
        _, wloss, _ = orc.train_step(*bat[k][:3])
        assert_close(base_loss[k], wloss, rtol=2 * RTOL * (k + 1), what="step %d loss" % k)
    want = orc.tables()
    for tid in TIDS:
        assert_close(base[tid], want[tid], rtol=2e-4 * 4, what="table %s" % TABLE_NAMES[tid])


def test_item_side_takes_the_spare_cus(tmp_path):
    """TFR_ITEM_SPLIT=1 at the headline shape: the item side runs one piece per block, 20 look-ahead sort blocks + 79
    user-side blocks + 157 item-side blocks = 256, one per CU (TFR_TILE_DEBUG counts the blocks of every launch);
    by default both sides take two pieces per block: 178"""
    _, _, err = _run_switched(tmp_path, "debug_split", {"TFR_TILE_DEBUG": "1", "TFR_ITEM_SPLIT": "1"})
    assert "[k_tile_step] 256 blocks (20 look-ahead)" in err, err[-2000:]
    _, _, err = _run_switched(tmp_path, "debug", {"TFR_TILE_DEBUG": "1"})
    assert "[k_tile_step] 178 blocks (20 look-ahead)" in err, err[-2000:]
