"""The small-table sweep's three-round form (k_dense_tiles on full-width rows: every head piece and the first two k = 1
continuation pieces of a row in flight together) against its general form (TFR_SWEEP_ROUNDS=0), bit for bit, and
against the float64 oracle, on batches built around the rule that picks the continuation slots.

D = 64: 16 lanes per row, 64 entries per piece.  The order of distinct ids inside a tile's sorted list is the scan's,
so the runs are of lengths whose piece count does not depend on where they start: 65 entries always cover exactly two
pieces (one k = 1 continuation, none deeper), 129 or more at least three (deeper), 1024 a whole tile.

One child process per form runs every case once (the switch is read once per process); the tests compare what the
two left behind."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import RTOL, assert_close, make_oracle, TABLE_NAMES
from tfrecomm_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIDS = (L.MU, L.BU, L.BI, L.P, L.Q)
U, I, D, K = 300, 200, 64, 3
TILES = (3, 7, 10, 12, 16)                               # one per NT instantiation: 4, 8, 10, 12, 16
KW = dict(loss="mse", lr=2e-3, reg=0.03)
MODES = {"tf1": dict(optimizer="adam", adam_mode="tf1"), "lazy": dict(optimizer="adam", adam_mode="lazy"),
         "sgd": dict(optimizer="sgd", adam_mode="tf1")}
FROZEN_ITEM_SIDE = (1 << L.BI) | (1 << L.Q)


def batch_size(T):
    return T * 1024 - (24 if T == 10 else 0)             # ten tiles: a short last one


def _column(rs, nkeys, T, B, full_tile):
    """one id column of B entries.  ids 0..4: a run of 65 in exactly 0, 1, 2, 3 and all tiles, single entries in the
    other tiles; id 5: a run of 129 in tile 0 and of 65 in tile 2; id 6 fills tile `full_tile` (None: no such tile);
    every other entry in short random runs of the remaining ids"""
    want65 = (0, 1, 2, 3, T)
    free = [t for t in range(T) if t != full_tile]
    col = []
    for t in range(T):
        n = min(1024, B - 1024 * t)
        if t == full_tile:
            col.append(np.full(n, 6, np.int32))
            continue
        runs = {a: (65 if free.index(t) < want65[a] else 1) for a in range(5)}
        if t == 0:
            runs[5] = 129
        elif t == 2:
            runs[5] = 65
        rest = n - sum(runs.values())
        keys = 7 + rs.permutation(nkeys - 7)
        cnt = rs.multinomial(rest, np.full(keys.size, 1.0 / keys.size))
        ids = np.concatenate([np.repeat(np.array(list(runs), np.int32), list(runs.values())),
                              np.repeat(keys.astype(np.int32), cnt)])
        assert ids.size == n
        col.append(ids[rs.permutation(n)])
    return np.concatenate(col)


def slot_batches(T, seed=0):
    """K batches of T tiles; the middle one has a tile filled by one id on each side"""
    rs = np.random.RandomState(1000 * T + seed)
    B = batch_size(T)
    out = []
    for s in range(K):
        full = 1 if s == 1 else None
        out.append((_column(rs, U, T, B, full), _column(rs, I, T, B, full), rs.randint(1, 6, B).astype(np.float32)))
    return out


def tables_for(seed, d=D):
    rs = np.random.RandomState(seed)
    return dict(mu=np.float32(0.2), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
                P=rs.normal(0, .15, (U, d)).astype(np.float32), Q=rs.normal(0, .15, (I, d)).astype(np.float32))


def run_case(d, T, mode, form, frozen=0, void=False):
    """what one model leaves behind: losses, the five tables, the kernel plan.  void: the second batch carries an id
    out of range - the step must raise and leave every table as it was"""
    import tfrecomm_amd as TT
    t = tables_for(7, d)
    bat = slot_batches(T)
    B = batch_size(T)
    out = {}
    with TT.SvdModel(U, I, d, **dict(KW, **MODES[mode])) as m:
        m.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        if frozen:
            m.set_frozen(frozen)
        out["plan"] = np.array(m.kernel_plan(B)["apply"])
        if void:
            m.train_step(*bat[0])
            before = m.tables()
            u = bat[1][0].copy()
            u[B // 2] = U                                # one user id past the table
            try:
                m.train_step(u, bat[1][1], bat[1][2])
                raised = False
            except IndexError:
                raised = True
            after = m.tables()
            out["raised"] = np.array(raised)
            out["untouched"] = np.array(all(np.array_equal(before[k], after[k]) for k in TIDS))
            loss = np.array([m.train_step(*bat[2])[1]], np.float32)       # and still usable afterwards
        elif form == "staged":
            m.upload_triples(*(np.concatenate([b[c] for b in bat]) for c in range(3)))
            m.stage_ids(np.arange(K * B, dtype=np.int64).reshape(K, B))
            loss = np.asarray(m.train_steps_staged(0, B, K, want_loss=True), np.float32)
        else:
            loss = np.array([m.train_step(*b)[1] for b in bat], np.float32)
        out["loss"] = loss
        for tid, v in m.tables().items():
            out["t%d" % tid] = np.asarray(v)
    return out


def cases():
    """name -> arguments of run_case"""
    c = {}
    for T in TILES:
        for form in ("staged", "single"):
            c["slots-T%d-%s" % (T, form)] = dict(d=D, T=T, mode="tf1", form=form)
    for mode in ("lazy", "sgd"):
        c["mode-%s" % mode] = dict(d=D, T=10, mode=mode, form="staged")
    c["frozen"] = dict(d=D, T=10, mode="tf1", form="single", frozen=FROZEN_ITEM_SIDE)
    for d in (15, 60):
        c["general-D%d" % d] = dict(d=d, T=3, mode="tf1", form="staged")
    c["void"] = dict(d=D, T=10, mode="tf1", form="single", void=True)
    return c


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from tests import test_gpu_sweep_rounds as S
res = {}
for name, kw in S.cases().items():
    for k, v in S.run_case(**kw).items():
        res[name + "/" + k] = v
np.savez(%r, **res)
"""


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{switch setting: {case/key: array}} - the default (three rounds) and TFR_SWEEP_ROUNDS=0 (general form)"""
    got = {}
    for name, env in (("rounds", {}), ("general", {"TFR_SWEEP_ROUNDS": "0"})):
        out = str(tmp_path_factory.mktemp("sweep") / (name + ".npz"))
        e = dict(os.environ, **env)
        if not env:
            e.pop("TFR_SWEEP_ROUNDS", None)
        p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, out)], env=e, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        got[name] = dict(np.load(out))
    return got


def _identical(forms, case):
    a, b = forms["rounds"], forms["general"]
    keys = [k for k in a if k.startswith(case + "/")]
    assert keys and all(k in b for k in keys)
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def _against_oracle(forms, case, T, mode, frozen=0):
    t = tables_for(7)
    orc = make_oracle(U, I, D, t, frozen=frozen, **dict(KW, **MODES[mode]))
    loss = forms["rounds"][case + "/loss"]
    for s, b in enumerate(slot_batches(T)):
        _, wloss, _ = orc.train_step(*b)
        assert_close(loss[s], wloss, rtol=2 * RTOL * (s + 1), what="%s step %d loss" % (case, s))
    want = orc.tables()
    base = 2e-4 if mode != "sgd" else 4 * RTOL           # the sweep's tolerances (test_gpu_parity), by the longest run: 1024
    for tid in TIDS:
        assert_close(forms["rounds"]["%s/t%d" % (case, tid)], want[tid], rtol=base * max(1.0, np.sqrt(1024 / 64.0)),
                     what="%s table %s" % (case, TABLE_NAMES[tid]))


@pytest.mark.parametrize("T", TILES)
def test_slot_rule(forms, T):
    """rows with 0, 1, 2, 3 and T k = 1 continuations, a deeper run, a whole tile: both forms bit for bit, published
    sort and self-sorted single steps bit for bit, the default within the sweep's tolerances of the oracle"""
    for form in ("staged", "single"):
        _identical(forms, "slots-T%d-%s" % (T, form))
    a = forms["rounds"]
    for k in ["loss"] + ["t%d" % tid for tid in TIDS]:
        assert np.array_equal(a["slots-T%d-staged/%s" % (T, k)], a["slots-T%d-single/%s" % (T, k)]), k
    nt = 4 if T <= 4 else 8 if T <= 8 else 10 if T <= 10 else 12 if T <= 12 else 16
    assert str(a["slots-T%d-staged/plan" % T]) == "k_dense_tiles<16, 4, false, %d>" % nt
    _against_oracle(forms, "slots-T%d-staged" % T, T, "tf1")


@pytest.mark.parametrize("mode", ["tf1", "lazy", "sgd"])
def test_optimiser_modes(forms, mode):
    case = "slots-T10-staged" if mode == "tf1" else "mode-%s" % mode
    _identical(forms, case)
    _against_oracle(forms, case, 10, mode)


def test_frozen_sides(forms):
    _identical(forms, "frozen")
    t = tables_for(7)
    a = forms["rounds"]
    assert np.array_equal(a["frozen/t%d" % L.BI], t["bi"]) and np.array_equal(a["frozen/t%d" % L.Q], t["Q"])
    assert not np.array_equal(a["frozen/t%d" % L.P], t["P"]) and not np.array_equal(a["frozen/t%d" % L.BU], t["bu"])
    _against_oracle(forms, "frozen", 10, "tf1", frozen=FROZEN_ITEM_SIDE)


@pytest.mark.parametrize("d,vec", [(15, 1), (60, 4)])
def test_general_form_still_taken(forms, d, vec):
    """rows that do not fill their lane group stay on the general form: the switch changes nothing, the plan names the
    same kernel"""
    _identical(forms, "general-D%d" % d)
    for f in ("rounds", "general"):
        assert str(forms[f]["general-D%d/plan" % d]) == "k_dense_tiles<16, %d, false, 4>" % vec


def test_voided_step(forms):
    """an id out of range: the step raises and no table moves, in both forms (the error word stops the sweep before
    any address from the lookup tables is used)"""
    for f in ("rounds", "general"):
        assert bool(forms[f]["void/raised"]), f
        assert bool(forms[f]["void/untouched"]), f
    _identical(forms, "void")


@pytest.mark.parametrize("shape", [(6040, 3952, 64, 10000)] + [(U, I, D, batch_size(T)) for T in TILES])
def test_residency(shape):
    """the whole grid of the sweep is resident at once and nothing spills - what its timing rests on"""
    import torch
    users, items, d, B = shape
    blocks, scratch, grid = C.c_int32(), C.c_int64(), C.c_int64()
    L.check(L.load().tfr_sweep_residency(d, B, users, items, C.byref(blocks), C.byref(scratch), C.byref(grid)))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("shape %s: %d blocks per CU x %d CUs, grid %d, scratch %d" % (shape, blocks.value, cus, grid.value, scratch.value))
    assert blocks.value * cus >= grid.value
    assert scratch.value == 0
