"""The other side of every environment switch of DESIGN.md §23 that no other test sets, against the default side.

The table is tests/switch_cases.py: the settings, the workloads a setting touches and the relation the switched run must
keep to the default run - ``bits`` (every table, Adam slot, loss and logit bit for bit) or ``reference`` (each side's
host-fed steps held to tests/step_ref.py, each side's staged run bit for bit against its own host-fed run; no tolerance
between the sides).  The library keeps most switches in a ``static const``, so every setting runs in a fresh child
process (tests/switch_workloads.py) that writes one .npz; the default child is shared.  Every pair of runs also shows
that it took two forms (kernel_plan strings, a k_gather_triples count) where there is something to show.

Children run one after another.  A child that ends by a signal, by exit status 134 or 139, or at its timeout is
recorded, and every later test of this module then fails at once without starting another child."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import switch_cases as C
from tests.test_width_coverage import geometry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = "import sys; sys.path.insert(0, %r); from tests import switch_workloads as W; W.main(sys.argv[1], sys.argv[2:])" % ROOT
DEFAULT_CHILD_S = 3.9            # measured on an MI355X: the default child (every step workload, each step checked per row); the
                                 # longest child (33.5 M keys twice, 2.2 s of host argsort each) took 6.4 s, every other under 1.5 s
CHILD_TIMEOUT_S = 10 * DEFAULT_CHILD_S + 20      # a loaded machine, a cold start of the runtime
# a GPU fault the child survived long enough to report (HIP's error text): the device is not used again either
GPU_FAULT_WORDS = ("illegal memory access", "Memory access fault", "unspecified launch failure", "HSA_STATUS_ERROR")
SWITCHES = sorted({k for _, env, _ in C.CHILDREN for k in env})

_FAULT = []                      # the first child that ended by a signal, an abort or its timeout


class Run:
    def __init__(self, path):
        with np.load(path) as z:
            self.arrays = {k: z[k] for k in z.files if k != "meta"}
            self.meta = json.loads(bytes(z["meta"]).decode())

    def keys(self, prefix):
        return sorted(k for k in self.arrays if k.startswith(prefix + "/"))


def _child(tmp_path, name, env, workloads):
    if _FAULT:
        pytest.fail("not started: %s" % _FAULT[0])
    path = str(tmp_path / (name + ".npz"))
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, "-c", SCRIPT, path] + list(workloads), env=e, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _FAULT.append("the child %s %s did not end within %d s" % (name, env, CHILD_TIMEOUT_S))
        pytest.fail(_FAULT[0])
    err = p.stderr.decode(errors="replace")
    if p.returncode < 0 or p.returncode in (134, 139) or (p.returncode != 0 and any(w in err for w in GPU_FAULT_WORDS)):
        _FAULT.append("the child %s %s ended with status %d:\n%s" % (name, env, p.returncode, err[-2000:]))
        pytest.fail(_FAULT[0])
    assert p.returncode == 0 and b"CHILD OK" in p.stdout, "child %s %s: status %d\n%s" % (name, env, p.returncode, p.stderr.decode()[-3000:])
    run = Run(path)
    print("CHILD %s %s: %.1f s (%s)" % (name, env, time.time() - t0, run.meta["times"]))
    return run


@pytest.fixture(scope="module")
def default(tmp_path_factory):
    """the default side of every step workload, each host-fed step held to tests/step_ref.py, and which pass the sort takes"""
    return _child(tmp_path_factory.mktemp("switches"), "default", {},
                  ["check", "big_general", "big_stream", "big_long", "tiles", "sort_plans"])


# ----------------------------------------------------------------------------- what a workload's keys are
def _prefixes(workload):
    from tests.switch_workloads import big_key, tile_key
    if workload in ("big_general", "big_stream"):
        widths = C.BIG_GENERAL if workload == "big_general" else C.BIG_STREAM
        return [big_key(D, opt, C.BIG_B) for D in widths for opt in C.BIG_OPTS]
    if workload == "big_long":
        return [big_key(D, opt, C.BIG_LONG_B) for D, opt in C.BIG_LONG]
    if workload == "tiles":
        return [tile_key(D, B) for D, B in C.TILE_SHAPES]
    return []


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_bits(run, ref, prefix, what):
    keys = run.keys(prefix)
    assert keys and keys == ref.keys(prefix), (what, prefix)
    bad = [k for k in keys if not _same_bits(run.arrays[k], ref.arrays[k])]
    assert not bad, "%s: differs from the default run in\n  %s" % (what, "\n  ".join(bad))


def _assert_reference(run, prefix, what):
    """the statements of tests/step_ref.py hold for every host-fed step (the child lists the violated ones), and the staged
    run left the tables and slots of the host-fed run"""
    bad = [b for b in run.meta["bad"] if b.startswith(prefix + ",")]
    assert not bad, "%s:\n  %s" % (what, "\n  ".join(bad))
    host = [k for k in run.keys(prefix + "/host") if "/logits" not in k and "/loss" not in k]
    assert host, (what, prefix)
    diff = [k for k in host if not _same_bits(run.arrays[k], run.arrays[k.replace("/host/", "/staged/")])]
    assert not diff, "%s: staged against host-fed differs in\n  %s" % (what, "\n  ".join(diff))


# ----------------------------------------------------------------------------- the two forms
def tile_step_epg(ntiles, G, VEC, forced=0):
    """csrc/svd_kernels.hip tile_step_epg, restated"""
    def fits(e):
        static = 5 * 1024 * 4 + 2 * e * 16 * 4 + e * 16 * 4 + e * (2 * (1024 // G) + 1024) * 4 + 16 * 4
        return 2 * e * 16 * G * VEC * 4 <= 64 * 1024 and static + 64 * 1024 <= 160 * 1024
    if forced == 1 or (forced in (2, 4) and forced <= G and fits(forced)):
        return forced
    epg = 1
    while epg < 4 and epg < G and ntiles * (G // epg) * 2 > 256 and fits(2 * epg):
        epg *= 2
    return epg


def _assert_two_forms(entry, env, run, default):
    name, how = entry["name"], entry["plan"]
    plans, dplans = run.meta["plan"], default.meta["plan"]
    step_keys = [p for w in entry["workloads"] for p in _prefixes(w)]
    if how == "gather":
        for key in step_keys:
            assert default.meta["gather"][key] == 0 and run.meta["gather"][key] > 0, (key, default.meta["gather"][key], run.meta["gather"][key])
        return
    if how == "branch":            # the same kernels in another order, or nothing kernel_plan names: nothing to show
        return
    assert how == "differs"
    if name == "TFR_LEAN":         # the Adam item side alone has a !LEAN form (csrc/svd_kernels.h RED_PICKS)
        for key in step_keys:
            adam = "-adam_" in key
            assert (plans[key] != dplans[key]) == adam, (key, plans[key], dplans[key])
            assert ("true, false, false>" in plans[key]) == adam and "true, false, false>" not in dplans[key], (key, plans[key])
    elif name == "TFR_TILE_SPLIT":
        for key in step_keys:
            assert "forward=k_front<" in plans[key] and "k_tile_step" not in plans[key] and "k_tile_step" in dplans[key], (key, plans[key], dplans[key])
    elif name == "TFR_EPG":
        forced, differ = int(env["TFR_EPG"]), 0
        for D, B in C.TILE_SHAPES:
            key = "tiles/D%d-B%d" % (D, B)
            G, VEC = geometry(D)
            want = tile_step_epg(-(-B // 1024), G, VEC, forced)
            assert want == forced, "TFR_EPG=%d is not accepted at D %d" % (forced, D)
            assert "k_tile_step<%d, %d, %d>" % (G, VEC, want) in plans[key], (key, plans[key])
            assert "k_tile_step<%d, %d, %d>" % (G, VEC, tile_step_epg(-(-B // 1024), G, VEC)) in dplans[key], (key, dplans[key])
            differ += plans[key] != dplans[key]
        assert differ >= 1, "TFR_EPG=%d: no shape where the default takes another EPG" % forced
    else:                          # the two radix switches: which pass sorts, in the step and in sort_segments
        wide, narrow = "k_rsortw_hist/k_rsort_scan/k_rsortw_scatter", "k_rsort_rank/scan/scatter"
        mine, theirs = (wide, narrow) if name == "TFR_RSORT_WIDE_MIN" else (narrow, wide)
        sizes = C.SORT_WIDE_MIN_B if name == "TFR_RSORT_WIDE_MIN" else C.SORT_NARROW_B
        for key in step_keys + ["sort/B%d" % B for B in sizes]:
            assert mine in plans[key] and theirs in dplans[key], (key, plans[key], dplans[key])


# ----------------------------------------------------------------------------- the tests
def test_default_side_holds_the_reference(default):
    """what the ``reference`` relation asks of each side, for the default side; every ``bits`` child inherits it"""
    for w in ("big_general", "big_stream", "big_long", "tiles"):
        for prefix in _prefixes(w):
            _assert_reference(default, prefix, "default, %s" % prefix)
    assert all(g == 0 for g in default.meta["gather"].values()), default.meta["gather"]


def _check_sort(run, name, shapes):
    rows = run.meta["sort"][name]
    assert [(n, B) for n, B, _, _ in rows] == [(n, B) for n, sizes in shapes for B in sizes], rows
    bad = [r for r in rows if not (r[2] and r[3])]
    assert not bad, "%s: not np.argsort(kind='stable') at (n, B, positions, keys) %s" % (name, bad)


@pytest.mark.parametrize("cid,env,entry", C.CHILDREN, ids=[c[0] for c in C.CHILDREN])
def test_switched_side(cid, env, entry, default, tmp_path):
    run = _child(tmp_path, cid, env, (["check"] if entry["relation"] == C.REFERENCE else []) + list(entry["workloads"]))
    for w in entry["workloads"]:
        for prefix in _prefixes(w):
            if entry["relation"] == C.BITS:
                _assert_bits(run, default, prefix, "%s, %s" % (cid, prefix))
            else:
                _assert_reference(run, prefix, "%s, %s" % (cid, prefix))
        if w == "sort_wide_min":
            _check_sort(run, w, [(n, C.SORT_WIDE_MIN_B) for n in C.SORT_WIDE_MIN_N])
        elif w == "sort_narrow":
            _check_sort(run, w, [(C.SORT_NARROW_N, C.SORT_NARROW_B)])
        elif w == "draw":
            from tests.test_gpu_rng import DRAW_CASES
            rows = run.meta["draw"]
            assert [(h, c) for h, c, _, _, _ in rows] == [tuple(x) for x in DRAW_CASES]       # no entry dropped: the longest takes well under a second
            bad = [r for r in rows if not (r[2] and r[3])]
            assert not bad, "k_mt_draw alone: ids or final state differ from NumPy at (high, count, ids, state, s) %s" % bad
    _assert_two_forms(entry, env, run, default)


def test_narrow_scatter_either_side_of_its_lds_prefix(tmp_path):
    """TFR_RSORT_WIDE=0 at the two key counts around the 2048 scan-block totals k_rsort_scatter's LDS prefix holds (three
    passes): the last total is taken from the prefix / added behind it"""
    assert [C.scan_blocks(B) for B in C.SORT_NARROW_PREF_B] == [C.RSORT_PREF, C.RSORT_PREF + 1]
    run = _child(tmp_path, "narrow_pref", {"TFR_RSORT_WIDE": "0"}, ["sort_narrow_pref"])
    _check_sort(run, "sort_narrow_pref", [(C.SORT_NARROW_PREF_N, C.SORT_NARROW_PREF_B)])
    for B in C.SORT_NARROW_PREF_B:
        assert "k_rsort_rank/scan/scatter" in run.meta["plan"]["sort/B%d" % B]
