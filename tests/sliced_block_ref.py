"""Host model of the shared scoring block (csrc/score_tile.h sliced_topk_block) and of the slice merge (csrc/topk.hip
k_topk_merge), in plain NumPy.

The contract (tests/topk_ref.py) says what the block must return.  This module restates how it gets there: the launch plan
(csrc/topk.h), the slice and round arithmetic, the per-query queue that takes up to 128 keys a round and is sorted and cut to
k only when it could not take another round, the running threshold, and the tournament over the slice lists.  Run on the
CPU, it tells for every test case which of those paths the device takes (the event record), so that the case list can be
held to reaching all of them (tests/test_sliced_block_ref_host.py) before the device is compared, bit for bit, with the
contract (tests/test_gpu_sliced_block.py).

The order in which the lanes of a round append their keys is not determined on the device.  Counts and results are: the
threshold only changes between the barriers that end a round, and a queue never overflows.  The model appends in candidate
order and asserts the no-overflow condition, so nothing here depends on the append order."""
import numpy as np

from tests.topk_ref import ordered_u32

# csrc/topk.h
TOPK_KMAX = 256
TOPK_WAVES = 4
TOPK_SUB = 32
TOPK_ROUND = TOPK_WAVES * TOPK_SUB
TOPK_MAX_SLICES = 256
TOPK_MERGE_KEYS = 8192
TOPK_CHUNK_MAX = 65536
TOPK_PART_BYTES = 128 << 20
TOPK_TARGET_BLOCKS = 1024
MERGE_LANES = 64                                           # csrc/topk.hip k_topk_merge: list s is head s // 64 of lane s % 64

MUTATIONS = ("threshold_ge", "threshold_one_high", "cut_one_short", "no_compaction", "merge_ignores_group_3")


def topk_cap(k):
    return 256 if k + TOPK_ROUND <= 256 else 512


def topk_upb(k):
    return 32 if topk_cap(k) == 256 else 16


def topk_slices_for(chunk, upb, k, items):
    smax = min(TOPK_MERGE_KEYS // k, TOPK_MAX_SLICES, -(-items // TOPK_ROUND))
    smax = max(smax, 1)
    tiles = -(-chunk // upb)
    s = -(-TOPK_TARGET_BLOCKS // tiles)
    return 1 if s < 1 else smax if s > smax else s


def topk_plan(k, n_rows, items):
    """csrc/topk.h topk_plan: dict(upb, cap, slices, chunk, lds_score, lds_merge), or None where the plan refuses"""
    if k < 1 or k > TOPK_KMAX or items < 1 or n_rows < 0:
        return None
    cap, upb = topk_cap(k), topk_upb(k)
    chunk = 1 if n_rows < 1 else min(n_rows, TOPK_CHUNK_MAX)
    chunk = -(-chunk // upb) * upb
    s = topk_slices_for(chunk, upb, k, items)
    while chunk > upb and chunk * s * k * 8 > TOPK_PART_BYTES:
        chunk = -(-(chunk // 2) // upb) * upb
        s = topk_slices_for(chunk, upb, k, items)
    return dict(upb=upb, cap=cap, slices=s, chunk=chunk, lds_score=upb * cap * 8 + upb * 8 + upb * 4, lds_merge=s * k * 8)


def slice_bounds(plan, cand_lo, cand_hi, s):
    """(per, s_lo, s_hi, rounds) of slice s over the candidates [cand_lo, cand_hi)"""
    n_cand = cand_hi - cand_lo
    per = -(-(-(-n_cand // plan["slices"])) // TOPK_ROUND) * TOPK_ROUND
    s_lo = cand_lo + s * per
    s_hi = min(s_lo + per, cand_hi)
    rounds = -(-(s_hi - s_lo) // TOPK_ROUND) if s_hi > s_lo else 0
    return per, s_lo, s_hi, rounds


def rounds_per_slice(plan, cand_lo, cand_hi):
    return [slice_bounds(plan, cand_lo, cand_hi, s)[3] for s in range(plan["slices"])]


def make_keys(scores, ids):
    """csrc/score_tile.h topk_key: (order-preserving uint32 of the score) << 32 | ~id"""
    o = ordered_u32(scores).astype(np.uint64)
    return (o << np.uint64(32)) | (~np.asarray(ids, np.int64).astype(np.uint32)).astype(np.uint64)


def key_ids(keys):
    return (~(keys & np.uint64(0xffffffff)).astype(np.uint32)).view(np.int32)


def key_scores(keys):
    o = (keys >> np.uint64(32)).astype(np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7fffffff), ~o).astype(np.uint32).view(np.float32)


def _compact(q, k, mut):
    """topk_compact: sort descending, keep the k best, the k-th key is the new threshold (0 while fewer than k are held)"""
    if mut == "cut_one_short" and k > 1:
        k = k - 1
    q = np.sort(q)[::-1]
    keep = min(q.size, k)
    q = q[:keep]
    if mut == "threshold_one_high" and keep == k and k > 1:
        return q, q[k - 2]
    return q, (q[k - 1] if keep == k else np.uint64(0))


def simulate_slice(score_row, k, plan, s, excluded, self_id, cand_lo, cand_hi, mut=None):
    """One block's work for one query: the sorted key list (at most k keys) it writes to part[row, s], and its events"""
    cap = plan["cap"]
    _, s_lo, s_hi, rounds = slice_bounds(plan, cand_lo, cand_hi, s)
    q = np.zeros(0, np.uint64)
    thr = np.uint64(0)
    ev = dict(compactions=0, appended_after=0, rejected=0, appends=[])
    for rd in range(rounds):
        base = s_lo + rd * TOPK_ROUND
        cand = np.arange(base, min(base + TOPK_ROUND, s_hi), dtype=np.int64)
        sc = score_row[cand]
        ok = np.ones(cand.size, bool)
        if self_id is not None:
            ok &= cand != self_id                          # eligible
        ok &= ~np.isnan(sc)                                # then NaN
        keys = make_keys(sc, cand)
        beats = keys >= thr if mut == "threshold_ge" else keys > thr
        ev["rejected"] += int(np.count_nonzero(ok & ~beats))
        ok &= beats                                        # then the threshold
        if excluded is not None and len(excluded):
            ok &= ~np.isin(cand, excluded)                 # then the exclusions
        new = keys[ok]
        ev["appends"].append(int(new.size))
        if ev["compactions"]:
            ev["appended_after"] += int(new.size)
        if mut == "no_compaction":
            new = new[:max(0, cap - q.size)]               # an append past the queue's CAP slots is lost to the queue
        q = np.concatenate([q, new])
        assert q.size <= cap, "a queue overflowed: cnt %d, CAP %d" % (q.size, cap)
        if q.size > cap - TOPK_ROUND and mut != "no_compaction":
            q, thr = _compact(q, k, mut)
            ev["compactions"] += 1
    if q.size:
        q, thr = _compact(q, k, mut)
    return q, ev


def merge(lists, k, mut=None):
    """k_topk_merge: the largest head over all lists, k times or until every list is exhausted.  Returns (keys taken, how many
    from each list, ended early)."""
    S = len(lists)
    part = np.zeros((S, k + 1), np.uint64)                 # key 0 marks the end of a list; column k is the `hd < k` guard
    for s, l in enumerate(lists):
        part[s, :l.size] = l
    if mut == "merge_ignores_group_3":
        part[3 * MERGE_LANES:] = 0
    hd = np.zeros(S, np.int64)
    taken = np.zeros(S, np.int64)
    out = []
    rows = np.arange(S)
    for _ in range(k):
        cur = part[rows, hd]
        s = int(np.argmax(cur))
        if cur[s] == 0:
            return np.array(out, np.uint64), taken, True
        out.append(cur[s])
        hd[s] += 1
        taken[s] += 1
    return np.array(out, np.uint64), taken, False


def simulate(score_row, k, plan, excluded=None, self_id=None, cand_lo=0, cand_hi=None, mut=None):
    """One query the way the device runs it.  score_row: f32 scores by candidate id (ids below cand_hi); excluded: sorted
    ids or None; self_id: the candidate a neighbour query may not return.  Returns (ids int32 [k], scores f32 [k], events)."""
    score_row = np.ascontiguousarray(score_row, np.float32)
    cand_hi = score_row.size if cand_hi is None else cand_hi
    S = plan["slices"]
    excluded = None if excluded is None else np.asarray(excluded, np.int64)
    lists, evs = [], []
    for s in range(S):
        l, e = simulate_slice(score_row, k, plan, s, excluded, self_id, cand_lo, cand_hi, mut)
        lists.append(l)
        evs.append(e)
    keys, taken, early = merge(lists, k, mut)
    ids = np.full(k, -1, np.int32)
    scores = np.full(k, -np.inf, np.float32)
    ids[:keys.size] = key_ids(keys)
    scores[:keys.size] = key_scores(keys)
    rounds = rounds_per_slice(plan, cand_lo, cand_hi)
    groups = sorted({s // MERGE_LANES for s in range(S)})
    events = dict(
        compactions=sum(e["compactions"] for e in evs),
        compactions_by_slice=[e["compactions"] for e in evs],
        appended_after_compaction=sum(e["appended_after"] for e in evs),
        threshold_rejected=sum(e["rejected"] for e in evs),
        empty_slices=sum(1 for r in rounds if r == 0),
        short_lists=sum(1 for r, l in zip(rounds, lists) if r > 0 and l.size < k),
        slices_by_head_group={g: sum(1 for s in range(S) if s // MERGE_LANES == g) for g in groups},
        taken_by_head_group={g: int(taken[g * MERGE_LANES:(g + 1) * MERGE_LANES].sum()) for g in groups},
        most_from_one_list=int(taken.max()) if S else 0,
        merge_ended_early=bool(early),
        appends_by_slice=[e["appends"] for e in evs],
    )
    return ids, scores, events
