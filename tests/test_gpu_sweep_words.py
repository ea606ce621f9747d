"""The three-round sweep (k_dense_tiles on full-width rows) fetches a row's 4-byte words - its table entries, the bias sums
of its pieces, its three bias words - in one request per round: lane t of the row's group loads what belongs to tile t
and the group hands the words round by cross-lane moves.  Here the default form is held bit for bit to the general form
(TFR_SWEEP_ROUNDS=0), all five tables with their Adam moments after three steps, on the shapes where lanes and tiles
can get out of step - which tests/test_gpu_sweep_rounds.py (D = 64 only) does not reach:

  * groups narrower than the tile count (D = 16: 4 lanes, D = 32: 8 lanes - entries and bias sums take several requests)
    and wider than it (D = 128, 256: groups of two and four 16-lane rows, lanes beyond the tile count idle);
  * 301 users and 203 items: the last wave of each side holds groups past the last row;
  * 1 and 9 tiles (the NT = 4 and NT = 10 instantiations then have lanes whose tile lies past the table's end), a short
    last tile (ten tiles are 10216 entries);
  * the batch builder of test_gpu_sweep_rounds at every width.  Its runs are made for D = 64 (64 entries per piece: rows
    with 0, 1, 2, 3 and T one-continuation runs, a run of three pieces, a tile filled by one id).  At D = 16 a piece
    holds 256 entries: a run of 65 or 129 has one continuation or none, by where it starts, and the filled tile has
    three.  At D = 128 and 256 a piece holds 32 and 16: every run of 65 is deeper than two pieces and goes through the
    hot-row loop, the single entries through the two slots;
  * runs cut to each width's own piece (_piece_column: a run of EPB + 1 entries is exactly two pieces wherever it starts,
    2 * EPB + 1 exactly three), so that rows with exactly 0, 1, 2 and 3 k = 1 continuations and a deeper run - both
    continuation slots, and both ways into the hot-row loop - are there by construction at D = 16, 32 and 128, at D = 16
    also in the NT = 4 instantiation;
  * reg_bias, the item side frozen, the biases alone frozen, lazy Adam and SGD; a voided step at D = 16;
  * the data-parallel sweep (WRITE = true) through tfr_dp_local_grads: the flat gradient buffer of every step.

One case per width is also held to the float64 oracle as test_gpu_sweep_rounds._against_oracle does.

One child process per form runs every case once (the switch is read once per process), as in test_gpu_sweep_rounds."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_gpu_sweep_rounds as S
from tests.util import RTOL, assert_close, make_oracle, TABLE_NAMES
from tfrecomm_amd import _lib as L

pytestmark = pytest.mark.gpu

U, I, K = 301, 203, 3
TIDS = S.TIDS
FROZEN_BIASES = (1 << L.BU) | (1 << L.BI)
WIDTHS = [(16, 3), (16, 10), (16, 16), (32, 10), (32, 16), (128, 10), (256, 10)]
TILE_COUNTS = [(64, 1), (64, 9), (16, 1), (16, 9)]
ORACLE = [(16, 10), (32, 10), (64, 9), (128, 10), (256, 10)]
PIECE_RUNS = [(16, 3), (16, 10), (32, 10), (128, 10)]             # runs cut to the width's piece: _piece_column
DP = [(16, 16), (64, 10)]


def batch_size(T):
    return 1000 if T == 1 else S.batch_size(T)           # one tile: a short one


def batches(T, seed=0):
    """K batches of T tiles from the builder of test_gpu_sweep_rounds, on this file's table sizes; the middle batch has
    a tile filled by one id on each side (where there is a second tile)"""
    rs = np.random.RandomState(1000 * T + seed)
    B = batch_size(T)
    out = []
    for s in range(K):
        full = 1 if (s == 1 and T > 1) else None
        out.append((S._column(rs, U, T, B, full), S._column(rs, I, T, B, full), rs.randint(1, 6, B).astype(np.float32)))
    return out


def _piece_column(rs, nkeys, T, B, epb):
    """one id column whose runs are cut to the width's piece of epb entries.  A run of epb + 1 covers exactly two pieces
    wherever it starts (one k = 1 continuation, none deeper), a run of 2 * epb + 1 exactly three (deeper).  ids 0..3: a run
    of epb + 1 in exactly 0, 1, 2 and 3 tiles (the first ones), single entries in the other tiles; id 4: a run of
    2 * epb + 1 in the last tile, single entries elsewhere; every other entry in short random runs of the remaining ids"""
    col = []
    for t in range(T):
        n = min(1024, B - 1024 * t)
        runs = {a: (epb + 1 if t < a else 1) for a in range(4)}
        runs[4] = 2 * epb + 1 if t == T - 1 else 1
        rest = n - sum(runs.values())
        assert rest >= 0
        keys = 5 + rs.permutation(nkeys - 5)
        cnt = rs.multinomial(rest, np.full(keys.size, 1.0 / keys.size))
        ids = np.concatenate([np.repeat(np.array(list(runs), np.int32), list(runs.values())),
                              np.repeat(keys.astype(np.int32), cnt)])
        assert ids.size == n
        col.append(ids[rs.permutation(n)])
    return np.concatenate(col)


def piece_batches(d, T, seed=1):
    """K batches of T >= 3 tiles with rows of exactly 0, 1, 2 and 3 k = 1 continuations and one deeper run on each side,
    at D = d: 1024 / (d / 4) entries per piece"""
    epb = 4096 // d
    rs = np.random.RandomState(1000 * T + d + seed)
    B = batch_size(T)
    return [(_piece_column(rs, U, T, B, epb), _piece_column(rs, I, T, B, epb), rs.randint(1, 6, B).astype(np.float32))
            for _ in range(K)]


def tables_for(seed, d):
    rs = np.random.RandomState(seed)
    return dict(mu=np.float32(0.2), bu=rs.normal(0, .5, U).astype(np.float32), bi=rs.normal(0, .5, I).astype(np.float32),
                P=rs.normal(0, .15, (U, d)).astype(np.float32), Q=rs.normal(0, .15, (I, d)).astype(np.float32))


def _leave(m, out, moments):
    for tid, v in m.tables().items():
        out["t%d" % tid] = np.asarray(v)
    if moments:
        for tid in TIDS:
            out["m%d" % tid] = np.asarray(m.get_table(tid | L.SLOT_M))
            out["v%d" % tid] = np.asarray(m.get_table(tid | L.SLOT_V))


def run_case(d, T, mode="tf1", form="staged", frozen=0, void=False, reg_bias=False, pieces=False):
    """what one model leaves behind after the K batches: losses, the five tables, their Adam moments, the kernel plan.
    void: the second batch carries an id out of range - the step must raise and leave every table as it was"""
    import tfrecomm_amd as TT
    t = tables_for(7, d)
    bat = piece_batches(d, T) if pieces else batches(T)
    B = batch_size(T)
    out = {}
    with TT.SvdModel(U, I, d, reg_bias=reg_bias, **dict(S.KW, **S.MODES[mode])) as m:
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
        _leave(m, out, mode != "sgd")
    return out


def run_dp(d, T):
    """one data-parallel replica: the flat gradient buffer tfr_dp_local_grads leaves for each of the K batches (applied
    in between), and the tables with their moments afterwards"""
    import torch
    from tfrecomm_amd import dataparallel
    t = tables_for(7, d)
    dev = torch.device("cuda", 0)
    out = {}
    rep = dataparallel.HipReplica(U, I, d, 0, **dict(S.KW, **S.MODES["tf1"]))
    try:
        rep.model.set_tables(t["mu"], t["bu"], t["bi"], t["P"], t["Q"])
        for s, b in enumerate(batches(T)):
            cols = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b]
            f = rep.local_grads(*cols)
            torch.cuda.synchronize()
            out["flat%d" % s] = f.cpu().numpy().copy()
            rep.apply(f)
            torch.cuda.synchronize()
            del cols
        _leave(rep.model, out, True)
    finally:
        rep.model.close()
    return out


def cases():
    """name -> (runner, arguments)"""
    c = {}
    for d, T in WIDTHS:
        c["width-D%d-T%d" % (d, T)] = (run_case, dict(d=d, T=T))
    for d, T in PIECE_RUNS:
        c["pieces-D%d-T%d" % (d, T)] = (run_case, dict(d=d, T=T, pieces=True))
    for d, T in TILE_COUNTS:
        c["tiles-D%d-T%d" % (d, T)] = (run_case, dict(d=d, T=T, form="single"))
    for d in (64, 16):
        c["reg_bias-D%d" % d] = (run_case, dict(d=d, T=10, reg_bias=True))
        c["frozen_biases-D%d" % d] = (run_case, dict(d=d, T=10, frozen=FROZEN_BIASES))
    c["frozen_items-D16"] = (run_case, dict(d=16, T=10, form="single", frozen=S.FROZEN_ITEM_SIDE))
    c["mode-lazy-D16"] = (run_case, dict(d=16, T=10, mode="lazy"))
    c["mode-sgd-D128"] = (run_case, dict(d=128, T=10, mode="sgd"))
    c["void-D16"] = (run_case, dict(d=16, T=10, form="single", void=True))
    for d, T in DP:
        c["dp-D%d-T%d" % (d, T)] = (run_dp, dict(d=d, T=T))
    return c


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
torch.cuda.init()                                        # torch's runtime before the library's (run_dp hands it torch tensors)
from tests import test_gpu_sweep_words as W
res = {}
for name, (run, kw) in W.cases().items():
    for k, v in run(**kw).items():
        res[name + "/" + k] = v
np.savez(%r, **res)
"""


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{switch setting: {case/key: array}} - the default (three rounds) and TFR_SWEEP_ROUNDS=0 (general form)"""
    got = {}
    for name, env in (("rounds", {}), ("general", {"TFR_SWEEP_ROUNDS": "0"})):
        out = str(tmp_path_factory.mktemp("words") / (name + ".npz"))
        e = dict(os.environ, **env)
        if not env:
            e.pop("TFR_SWEEP_ROUNDS", None)
        p = subprocess.run([sys.executable, "-c", _CHILD % (S.ROOT, out)], env=e, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        got[name] = dict(np.load(out))
    return got


def _identical(forms, case, moments=True):
    """every array the case left behind, bit for bit in both forms: the five tables (and their moments) among them"""
    a, b = forms["rounds"], forms["general"]
    keys = [k for k in a if k.startswith(case + "/")]
    want = ["t%d" % tid for tid in TIDS] + (["%s%d" % (s, tid) for tid in TIDS for s in "mv"] if moments else [])
    assert all(case + "/" + k in keys for k in want), keys
    assert all(k in b for k in keys)
    for k in keys:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _plan(forms, case, d, T):
    nt = 4 if T <= 4 else 8 if T <= 8 else 10 if T <= 10 else 12 if T <= 12 else 16
    assert str(forms["rounds"][case + "/plan"]) == "k_dense_tiles<%d, 4, false, %d>" % (d // 4, nt)


@pytest.mark.parametrize("d,T", WIDTHS)
def test_widths(forms, d, T):
    case = "width-D%d-T%d" % (d, T)
    _identical(forms, case)
    _plan(forms, case, d, T)


@pytest.mark.parametrize("d,T", PIECE_RUNS)
def test_piece_sized_runs(forms, d, T):
    """rows with exactly 0, 1, 2 and 3 k = 1 continuations and a deeper run at this width's piece size: the two
    continuation slots, the third continuation and the deeper run that send a row through the hot-row loop"""
    case = "pieces-D%d-T%d" % (d, T)
    _identical(forms, case)
    _plan(forms, case, d, T)


@pytest.mark.parametrize("d,T", TILE_COUNTS)
def test_tile_counts(forms, d, T):
    case = "tiles-D%d-T%d" % (d, T)
    _identical(forms, case)
    _plan(forms, case, d, T)


@pytest.mark.parametrize("case", ["reg_bias-D64", "reg_bias-D16", "mode-lazy-D16"])
def test_options(forms, case):
    _identical(forms, case)


def test_sgd(forms):
    _identical(forms, "mode-sgd-D128", moments=False)


@pytest.mark.parametrize("d", [64, 16])
def test_frozen_biases(forms, d):
    """the biases alone frozen: they stay, the factors move - and the three bias words' request reads no moment"""
    case = "frozen_biases-D%d" % d
    _identical(forms, case)
    t = tables_for(7, d)
    a = forms["rounds"]
    assert np.array_equal(a[case + "/t%d" % L.BU], t["bu"]) and np.array_equal(a[case + "/t%d" % L.BI], t["bi"])
    assert not np.array_equal(a[case + "/t%d" % L.P], t["P"]) and not np.array_equal(a[case + "/t%d" % L.Q], t["Q"])


def test_frozen_item_side(forms):
    case = "frozen_items-D16"
    _identical(forms, case)
    t = tables_for(7, 16)
    a = forms["rounds"]
    assert np.array_equal(a[case + "/t%d" % L.BI], t["bi"]) and np.array_equal(a[case + "/t%d" % L.Q], t["Q"])
    assert not np.array_equal(a[case + "/t%d" % L.P], t["P"]) and not np.array_equal(a[case + "/t%d" % L.BU], t["bu"])


def test_voided_step(forms):
    """an id out of range at D = 16: the step raises and no table moves, in both forms"""
    for f in ("rounds", "general"):
        assert bool(forms[f]["void-D16/raised"]), f
        assert bool(forms[f]["void-D16/untouched"]), f
    _identical(forms, "void-D16")


@pytest.mark.parametrize("d,T", DP)
def test_data_parallel_sweep(forms, d, T):
    """WRITE = true: the flat gradient buffer of every step, and the tables the applies leave, bit for bit"""
    case = "dp-D%d-T%d" % (d, T)
    assert all("%s/flat%d" % (case, s) in forms["rounds"] for s in range(K))
    assert all(np.any(forms["rounds"]["%s/flat%d" % (case, s)]) for s in range(K))
    _identical(forms, case)


@pytest.mark.parametrize("d,T", ORACLE)
def test_against_oracle(forms, d, T):
    """the default form within the sweep's tolerances of the float64 oracle (test_gpu_sweep_rounds._against_oracle)"""
    case = ("tiles-D%d-T%d" if (d, T) in TILE_COUNTS else "width-D%d-T%d") % (d, T)
    t = tables_for(7, d)
    orc = make_oracle(U, I, d, t, **dict(S.KW, **S.MODES["tf1"]))
    loss = forms["rounds"][case + "/loss"]
    for s, b in enumerate(batches(T)):
        _, wloss, _ = orc.train_step(*b)
        print("%s step %d loss %.9g oracle %.9g" % (case, s, loss[s], wloss))
        assert_close(loss[s], wloss, rtol=2 * RTOL * (s + 1), what="%s step %d loss" % (case, s))
    want = orc.tables()
    for tid in TIDS:
        assert_close(forms["rounds"]["%s/t%d" % (case, tid)], want[tid], rtol=2e-4 * max(1.0, np.sqrt(1024 / 64.0)),
                     what="%s table %s" % (case, TABLE_NAMES[tid]))
