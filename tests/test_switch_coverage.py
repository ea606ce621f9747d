"""Every environment switch the library reads has a row in DESIGN.md §23 and an entry in tests/switch_cases.py - covered by a
test that sets it, or exempt with a reason - and the workloads of tests/test_gpu_switches.py are what they claim to be.
No GPU: source text, ``ast`` and the dispatch rules restated in tests/step_cases.py and tests/test_width_coverage.py."""
import ast
import os
import re
import shutil

import pytest

from tests import step_cases as S
from tests import switch_cases as C
from tests.test_width_coverage import geometry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tf-recomm_amd", "csrc")
READER = re.compile(r"\benv_(?:default_on|default_off|int|is_set)\(\s*\"([A-Za-z0-9_]+)\"")


def switches_read(csrc):
    """every name passed to one of the four readers of env_switch.h under ``csrc``"""
    names = set()
    for dirpath, _, files in os.walk(csrc):
        for f in files:
            if f.endswith((".hip", ".h", ".hpp", ".cpp", ".inc")):
                names |= set(READER.findall(open(os.path.join(dirpath, f), errors="replace").read()))
    return names


def design_rows():
    """{switch: last column} of the table of DESIGN.md §23"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("\n## 23. "):]
    sec = sec[:sec.index("\n## ", 1)]
    rows = {}
    for line in sec.splitlines():
        m = re.match(r"\| `(TFR_[A-Z0-9_]+)` \|", line)
        if m:
            rows[m.group(1)] = line.rstrip().rstrip("|").rsplit("|", 1)[1].strip()
    return rows


def check_table(read, rows, cases=C.BY_NAME, exempt=C.EXEMPT):
    """the violated statements, one line each"""
    bad = []
    for n in sorted(read - set(rows)):
        bad.append("%s is read under csrc/ and has no row in DESIGN.md §23" % n)
    for n in sorted(set(rows) - read):
        bad.append("%s has a row in DESIGN.md §23 and no reader under csrc/" % n)
    for n in sorted(read | set(rows)):
        if n in exempt:
            if len(exempt[n].split()) < 5:
                bad.append("%s is exempt without a reason" % n)
        elif n not in cases:
            bad.append("%s has no entry in tests/switch_cases.py" % n)
    for n in sorted((set(cases) | set(exempt)) - (read | set(rows))):
        bad.append("tests/switch_cases.py lists %s, which nothing reads" % n)
    return bad


def test_every_switch_read_has_a_row_and_an_entry():
    read, rows = switches_read(CSRC), design_rows()
    assert len(read) >= 28, sorted(read)                     # the collector still finds the readers
    bad = check_table(read, rows)
    assert not bad, "\n".join(bad)


def test_a_missing_entry_and_a_new_reader_are_noticed(tmp_path):
    """the guard guards: drop an entry, or add a reader to a scratch copy of a source file, and it says so"""
    read, rows = switches_read(CSRC), design_rows()
    for name in C.BY_NAME:
        less = {k: v for k, v in C.BY_NAME.items() if k != name}
        assert check_table(read, rows, cases=less) == ["%s has no entry in tests/switch_cases.py" % name]
    scratch = tmp_path / "csrc"
    scratch.mkdir()
    shutil.copy(os.path.join(CSRC, "sort.hip"), scratch / "sort.hip")
    shutil.copy(os.path.join(CSRC, "env_switch.h"), scratch / "env_switch.h")
    with open(scratch / "sort.hip", "a") as f:
        f.write('\nstatic const int fresh = (int)env_int("TFR_NEW", 0);\n')
    more = switches_read(str(scratch)) | read
    assert check_table(more, rows) == ["TFR_NEW is read under csrc/ and has no row in DESIGN.md §23", "TFR_NEW has no entry in tests/switch_cases.py"]


def test_design_names_the_test_that_holds_each_switch():
    rows = design_rows()
    for name, held in rows.items():
        if name in C.EXEMPT:
            assert held.startswith("exempt"), (name, held)
        elif C.BY_NAME[name]["held_by"] == C.NEW:
            assert "tests/test_gpu_switches.py" in held, (name, held)
        else:
            fname, test = C.BY_NAME[name]["held_by"]
            assert fname in held and test in held, (name, held)


def sets_variable(tree, var):
    """does the module set the environment variable ``var``: as a keyword (``dict(os.environ, VAR=...)``), as a key of a dict
    literal, by ``env[VAR] = ...`` or by ``setenv(VAR, ...)`` - VAR spelled out or a module-level name bound to it"""
    names = {t.id for n in tree.body if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant) and n.value.value == var
             for t in n.targets if isinstance(t, ast.Name)}

    def is_var(node):
        return (isinstance(node, ast.Constant) and node.value == var) or (isinstance(node, ast.Name) and node.id in names)

    for n in ast.walk(tree):
        if isinstance(n, ast.keyword) and n.arg == var:
            return True
        if isinstance(n, ast.Dict) and any(k is not None and is_var(k) for k in n.keys):
            return True
        if isinstance(n, ast.Subscript) and isinstance(n.ctx, ast.Store) and is_var(n.slice):
            return True
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "setenv" and n.args and is_var(n.args[0]):
            return True
    return False


HELD = [c for c in C.CASES if c["held_by"] != C.NEW]


@pytest.mark.parametrize("entry", HELD, ids=[c["name"] for c in HELD])
def test_the_named_test_sets_the_switch(entry):
    fname, test = entry["held_by"]
    tree = ast.parse(open(os.path.join(HERE, fname)).read())
    assert any(isinstance(n, ast.FunctionDef) and n.name == test for n in ast.walk(tree)), "%s has no %s" % (fname, test)
    assert sets_variable(tree, entry["name"]), "%s does not set %s" % (fname, entry["name"])
    assert len(entry["reason"].split()) >= 3


def test_the_new_entries_run_from_the_table():
    """tests/test_gpu_switches.py parametrises over switch_cases.CHILDREN - one child per setting of every ``new`` entry - and
    names no switch the table does not hold"""
    assert [(c["name"], env) for _, env, c in C.CHILDREN] == [(c["name"], env) for c in C.NEW_CASES for env in c["settings"]]
    assert len({cid for cid, _, _ in C.CHILDREN}) == len(C.CHILDREN)
    for c in C.NEW_CASES:
        assert c["settings"] and c["workloads"] and set(c["workloads"]) <= set(C.WORKLOADS), c["name"]
        assert c["relation"] in (C.BITS, C.REFERENCE) and c["plan"] in ("differs", "gather", "branch") and len(c["reason"].split()) >= 8, c["name"]
        assert all(c["name"] in env and set(env) <= set(C.BY_NAME) for env in c["settings"]), c["name"]
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_switches.py")).read())
    fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "test_switched_side"]
    assert len(fn) == 1
    over = [a for d in fn[0].decorator_list if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize" for a in d.args[1:]]
    assert len(over) == 1 and isinstance(over[0], ast.Attribute) and over[0].attr == "CHILDREN" and over[0].value.id == "C", \
        "test_switched_side does not parametrise over switch_cases.CHILDREN"
    named = {n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and re.fullmatch(r"TFR_[A-Z0-9_]+", n.value)}
    assert named <= {c["name"] for c in C.NEW_CASES}, "tests/test_gpu_switches.py names %s itself" % sorted(named - set(C.BY_NAME))
    for fname in ("test_gpu_switches.py", "switch_workloads.py"):          # and no list of settings of their own
        tree = ast.parse(open(os.path.join(HERE, fname)).read())
        lists = [n for n in ast.walk(tree) if isinstance(n, (ast.List, ast.Tuple)) and sum(isinstance(e, ast.Dict) for e in n.elts) > 1]
        assert not lists, "%s keeps a list of settings" % fname


def test_the_workloads_are_what_they_claim():
    # big: the fused big-table path (radix sort, k_seg_reduce with the forward inside, the look-ahead pipeline when staged)
    for B in (C.BIG_B, C.BIG_B - C.BIG_RAGGED, C.BIG_LONG_B, C.BIG_LONG_B - C.BIG_RAGGED):
        for opt, mode in C.BIG_OPTS:
            assert S.path_of(C.BIG_U, C.BIG_I, B, opt, mode) == "fused_big", (B, opt, mode)
    assert ("adam", "lazy") in C.BIG_OPTS and ("sgd", "tf1") in C.BIG_OPTS

    def full(D):
        g, vec = geometry(D)
        return D == g * vec
    # FAST (seg_reduce_pick: D == G * VEC) ignores nt, LEAN and stage_sum: the widths that run them are not full width
    assert C.BIG_GENERAL == (33, 100) and not any(full(D) for D in C.BIG_GENERAL)
    assert {geometry(D)[1] for D in C.BIG_GENERAL} == {1, 4}
    assert 64 in C.BIG_STREAM and full(64) and any(not full(D) for D in C.BIG_STREAM)
    assert C.BIG_B < 4096 and C.BIG_B % 1024 and C.BIG_LONG_B == 65536 + 5                 # a short only wide tile; the first wide size + 5
    assert {D for D, _ in C.BIG_LONG} >= {64} and {o for _, o in C.BIG_LONG} == set(C.BIG_OPTS)
    # tiles: k_tile_step's path, at a batch of at most 16 tiles
    for D, B in C.TILE_SHAPES:
        assert S.path_of(C.TILE_U, C.TILE_I, B, "adam", "tf1").startswith("tiles"), (D, B)
    assert set(C.TILE_SHAPES) >= {(64, 2049), (64, 10000), (15, 2049), (15, 10000), (128, 10000)}
    # every forced EPG is accepted somewhere and differs from the default's somewhere
    from tests.test_gpu_switches import tile_step_epg
    for forced in (1, 2, 4):
        took = [(tile_step_epg(-(-B // 1024), *geometry(D), forced), tile_step_epg(-(-B // 1024), *geometry(D))) for D, B in C.TILE_SHAPES]
        assert any(f == forced and f != d for f, d in took), (forced, took)
    assert tile_step_epg(10, *geometry(128)) == 4 and tile_step_epg(3, *geometry(64)) == 1 and tile_step_epg(10, *geometry(64)) == 2
    # sort: the edges the issue of record lists, and both sides of every count k_rsort_scatter branches on
    assert set(C.SORT_WIDE_MIN_B) >= {1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 12289}
    assert S.bits_for(C.SORT_WIDE_MIN_N[0]) == 15 and S.bits_for(C.SORT_WIDE_MIN_N[1]) == 25       # two and four 8-bit passes
    assert set(C.SORT_NARROW_B) >= {65536, 100_000, 300_001}
    assert [C.scan_blocks(B) for B in C.SORT_NARROW_B[-2:]] == [32, 33]                       # use_pref = nb > 32
    assert [C.scan_blocks(B) for B in C.SORT_NARROW_PREF_B] == [C.RSORT_PREF, C.RSORT_PREF + 1]
    assert 17 <= S.bits_for(C.SORT_NARROW_PREF_N) <= 24                                       # three passes
    for n in C.SORT_WIDE_MIN_N + (C.SORT_NARROW_N, C.SORT_NARROW_PREF_N):
        assert (1 << S.bits_for(n)) > S.CSORT_MAX_BINS                                        # the radix sort, not the counting sort
