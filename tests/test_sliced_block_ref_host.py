"""The host model of the scoring block (tests/sliced_block_ref.py) against the contract (tests/topk_ref.py,
tests/neighbours_ref.py) on every case of tests/sliced_cases.py, what the case list reaches of the block's paths, and that
the cases can fail: a wrong model is caught.  No device is needed; tests/test_gpu_sliced_block.py runs the same cases on one."""
import numpy as np
import pytest

from tests import sliced_block_ref as M
from tests import sliced_cases as C
from tests.topk_ref import topk_ref

CAPS = (256, 512)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def live_users(c):
    return sorted(set(c.rows().tolist()))


def test_the_plan_constants_are_the_headers():
    """the restated constants against csrc/topk.h, read as text: a change there must be made here too"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tf-recomm_amd", "csrc", "topk.h")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, name
        return m.group(1).strip()
    assert const("TOPK_KMAX") == "256" and const("TOPK_WAVES") == "4" and const("TOPK_SUB") == "32"
    assert const("TOPK_ROUND") == "TOPK_WAVES * TOPK_SUB" and const("TOPK_MAX_SLICES") == "256"
    assert const("TOPK_MERGE_KEYS") == "8192" and const("TOPK_CHUNK_MAX") == "65536"
    assert const("TOPK_PART_BYTES") == "(int64_t)128 << 20" and const("TOPK_TARGET_BLOCKS") == "1024"
    assert "k + TOPK_ROUND <= 256 ? 256 : 512" in src and "topk_cap(k) == 256 ? 32 : 16" in src


@pytest.mark.parametrize("c", C.CASES, ids=repr)
def test_case_claims_hold_in_the_restated_plan(c):
    p = c.plan()
    assert p["slices"] == c.slices, (p, c.slices)
    assert M.rounds_per_slice(p, 0, c.I) == c.claimed_rounds()
    assert p["chunk"] >= c.n_rows, "a case is one chunk"
    assert c.n_rows % p["upb"] != 0, "the last tile must be partial"
    rows = c.rows()
    tile0 = rows[:p["upb"]].tolist()
    assert len(set(tile0)) < len(tile0), "no user twice in the first tile"
    assert rows.min() >= 0 and rows.max() < C.NU
    if c.group == "tall":
        assert max(c.claimed_rounds()) >= 3 and c.n_rows >= 8192
    if c.group == "wide":
        assert c.slices == min(M.TOPK_MERGE_KEYS // c.k, M.TOPK_MAX_SLICES), "not the most slices k allows"
        assert max(c.claimed_rounds()) >= (3 if p["cap"] == 256 else 6)
        last = max(s for s, r in enumerate(c.claimed_rounds()) if r)
        _, s_lo, s_hi, r = M.slice_bounds(p, 0, c.I, last)
        assert 1 <= (s_hi - s_lo) - (r - 1) * M.TOPK_ROUND <= 3, "the last round must hold one to three candidates"
    if c.group == "merge" and c.n_rows == 3:
        assert M.slice_bounds(p, 0, c.I, 0)[0] in (128, 256)


@pytest.mark.parametrize("c", C.CASES, ids=repr)
def test_scores_are_exact(c):
    """every score of a case is the same number in float64: no rounding anywhere, so the device has one right answer"""
    t = c.tables()
    P, Q = t["P"].astype(np.float64), t["Q"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        S64 = P @ Q.T + float(t["mu"]) + t["bu"].astype(np.float64)[:, None] + t["bi"].astype(np.float64)[None, :]
    S = c.scores()
    ok = np.isnan(S64) | (S.astype(np.float64) == S64)
    assert ok.all()
    assert np.array_equal(np.isnan(S), np.isnan(S64))


@pytest.mark.parametrize("c", C.CASES, ids=repr)
def test_model_equals_the_contract(c):
    si, ss, _ = c.simulated()
    wi, ws = c.reference()
    assert np.array_equal(si, wi)
    assert np.array_equal(bits(ss), bits(ws))


@pytest.mark.parametrize("c", C.TALL + C.WIDE, ids=repr)
def test_model_equals_the_neighbour_contract(c):
    si, ss, ev = c.nb_simulated()
    wi, ws = c.nb_reference()
    assert np.array_equal(si, wi)
    assert np.array_equal(bits(ss), bits(ws))
    # the self mask bites late: some query would be its own neighbour, and its slice had compacted before its round came
    p, S = c.plan(), c.nb_scores()
    hit = []
    for u in range(C.NU):
        q = c.nb_at() + u
        free, _, _ = M.simulate(S[u], c.k, p, c.excl_of_user(u) if c.with_excl else None)
        per = M.slice_bounds(p, 0, c.I, 0)[0]
        if q in free and ev[u]["compactions_by_slice"][q // per] > 0:
            hit.append(u)
    assert hit, "no query would return itself after a compaction"


def test_signed_zeros_nan_and_infinities_in_the_model():
    """+0 orders before -0 (the key's order, and topk_ref's); NaN is never returned; the infinities order like numbers.
    No score the device computes can be -0 (its accumulators start at +0), so this is checked on the model alone."""
    rs = np.random.RandomState(5)
    for k, n_rows, I in ((10, 3, 700), (129, 3, 1300), (256, 40, 3000), (128, 3, 1500)):
        p = M.topk_plan(k, n_rows, I)
        for _ in range(4):
            s = rs.choice(np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 0.5], np.float32), I).astype(np.float32)
            x = np.unique(rs.randint(0, I, rs.randint(0, 50)))
            gi, gs, _ = M.simulate(s, k, p, x)
            wi, ws = topk_ref(s[None, :], k, [x])
            assert np.array_equal(gi, wi[0]) and np.array_equal(bits(gs), bits(ws[0]))
    s = np.array([-0.0, 0.0, -0.0, 0.0], np.float32)
    gi, gs, _ = M.simulate(s, 4, M.topk_plan(4, 1, 4))
    assert gi.tolist() == [1, 3, 0, 2] and bits(gs).tolist() == [0, 0, 0x80000000, 0x80000000]


def mixed_tile(c, ev):
    """a tile and slice in which one live queue compacts mid-stream and another does not"""
    upb, rows = c.plan()["upb"], c.rows()
    for t0 in range(0, min(rows.size, 4 * upb), upb):     # the row pattern repeats: the first tiles tell
        tile = rows[t0:t0 + upb]
        for s in range(c.slices):
            n = [ev[int(u)]["compactions_by_slice"][s] for u in tile]
            if max(n) > 0 and min(n) == 0:
                return True
    return False


def reached(c):
    """the events a case reaches, over the users its rows hold"""
    _, _, ev = c.simulated()
    got = set()
    for u in live_users(c):
        e = ev[u]
        if e["compactions"]:
            got.add("a mid-stream compaction")
        if e["appended_after_compaction"]:
            got.add("appends after a compaction")
        if e["threshold_rejected"]:
            got.add("threshold rejections")
        if e["empty_slices"]:
            got.add("an empty slice")
        if e["short_lists"]:
            got.add("a list shorter than k")
        for g, n in e["taken_by_head_group"].items():
            if n:
                got.add("a key taken from merge head group %d" % g)
        if e["most_from_one_list"] == c.k and c.slices > 1:
            got.add("a merge that takes all k from one list")
        if e["merge_ended_early"] and c.slices > 1:
            got.add("a merge that ends early")
    if mixed_tile(c, ev):
        got.add("a tile in which one queue compacts and another does not")
    return got


EVENTS = ["a mid-stream compaction", "appends after a compaction", "threshold rejections",
          "a tile in which one queue compacts and another does not", "an empty slice", "a list shorter than k",
          "a merge that takes all k from one list", "a merge that ends early"]
HEAD_GROUPS = ["a key taken from merge head group %d" % g for g in range(4)]


def test_the_cases_reach_every_path_of_the_block():
    """Every event at both queue capacities.  The merge's head groups 1 to 3 are lists 64 to 255, and a row has at most
    TOPK_MERGE_KEYS / k lists: 63 at k = 129, so only CAP 256 plans (k <= 128) can reach them; k_topk_merge itself takes no
    queue capacity."""
    assert M.TOPK_MERGE_KEYS // 129 < M.MERGE_LANES
    got = {cap: set() for cap in CAPS}
    for c in C.CASES:
        got[c.plan()["cap"]] |= reached(c)
    missing = ["%s at CAP %d" % (e, cap) for cap in CAPS for e in EVENTS if e not in got[cap]]
    missing += ["%s at CAP 256" % e for e in HEAD_GROUPS if e not in got[256]]
    missing += ["merge head group 0 at CAP 512"] if HEAD_GROUPS[0] not in got[512] else []
    assert not missing, "no case reaches: " + "; ".join(missing)
    # the CAP 512 queue first compacts after round 4: some case must append to it after that
    assert any(c.plan()["cap"] == 512 and max(c.claimed_rounds()) >= 6 and "appends after a compaction" in reached(c)
               for c in C.CASES)
    # a merge over exactly the 64 KB of LDS the plan allows
    assert any(c.plan()["lds_merge"] == 65536 for c in C.CASES)
    # the patterns: every one of them is some live row's, at both capacities
    for cap in CAPS:
        pats = {C.PATTERNS[c.user_feature(u)] for c in C.CASES if c.plan()["cap"] == cap for u in live_users(c)}
        assert pats >= set(C.PATTERNS[:8]), (cap, sorted(set(C.PATTERNS[:8]) - pats))
    assert {c.D % 4 == 0 for c in C.CASES} == {False, True}, "both load forms of the tile (V4 and not)"
    assert any(c.bi_mode == "specials" for c in C.CASES if c.plan()["cap"] == 256)
    assert any(c.bi_mode == "specials" for c in C.CASES if c.plan()["cap"] == 512)


def test_the_specials_are_where_the_cases_say():
    for c in C.CASES:
        if c.bi_mode != "specials":
            continue
        p, bi = c.plan(), c.tables()["bi"]
        per = M.slice_bounds(p, 0, c.I, 0)[0]
        assert np.isnan(bi[128:256]).all(), "a whole round of NaN"
        if p["slices"] > 1:
            assert np.isnan(bi[per:2 * per]).all(), "a whole slice of NaN"
        assert np.isposinf(bi).sum() >= 2 and np.isneginf(bi).sum() >= 2 and np.signbit(bi[bi == 0]).any()
        wi, ws = c.reference()
        u = [u for u in live_users(c) if len(c.excl_of_user(u)) == 0][0]
        assert np.isposinf(ws[u, 0]) and not np.isnan(ws).any()


def caught_by(mut, cases):
    for c in cases:
        p, S = c.plan(), c.scores()
        wi, ws = c.reference()
        for u in live_users(c):
            gi, gs, _ = M.simulate(S[u], c.k, p, c.excl_of_user(u) if c.with_excl else None, mut=mut)
            if not (np.array_equal(gi, wi[u]) and np.array_equal(bits(gs), bits(ws[u]))):
                return c.name, u
    return None


SMALL = [C.BY_NAME[n] for n in ("tall_k100_ragged", "tall_k129", "tall_k10_free", "merge_256", "merge_8_last_empty")]


@pytest.mark.parametrize("mut", ["threshold_one_high", "cut_one_short", "no_compaction", "merge_ignores_group_3"])
def test_a_wrong_model_is_caught(mut):
    """the cases can fail: a threshold raised to the (k - 1)-th key, a cut that keeps k - 1 keys, a queue that is never
    compacted (its appends past CAP are lost) and a merge that never looks at lists 192 to 255 each give a wrong answer on
    some case"""
    assert caught_by(mut, SMALL) is not None, mut


def test_the_threshold_test_cannot_tell_greater_from_greater_or_equal():
    """`key >= th` for `key > th` is no error, and no case can catch it: a threshold is a key of the queue, keys are
    distinct ((score, id) pairs, every id scored once per block), so no candidate's key ever equals it.  What the threshold
    test must not do is reject a key above the k-th, which is the cut's mutation above.  Pinned here, so that a change of the
    key that lets two candidates share one (dropping the id, say) shows up as this test failing."""
    assert caught_by("threshold_ge", SMALL) is None
    for c in SMALL:
        _, _, ev = c.simulated()
        p, S = c.plan(), c.scores()
        for u in live_users(c)[:8]:
            e = M.simulate(S[u], c.k, p, c.excl_of_user(u) if c.with_excl else None, mut="threshold_ge")[2]
            assert e["threshold_rejected"] == ev[u]["threshold_rejected"]
