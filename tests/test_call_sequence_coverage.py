"""Every entry point of the SVD handle has a place in the call-sequence suite (tests/handle_states.py,
tests/test_gpu_call_sequences.py), in the manner of tests/test_width_coverage.py: the header is the list.

A function of include/tfrecomm.h whose first parameter is ``tfr_model*`` must be
  - reached by a registered guest (the guest names it; that tfrecomm_amd/engine.py or the guest itself calls it is checked
    against the source text),
  - or used by a state builder or by the harness around the guest,
  - or listed in EXEMPT with the reason it has no place.
A new entry point fails here until it is placed.  Every guest runs in every state or carries a reason why not."""
import inspect
import os
import re

from tests import handle_states as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# used by the state builders, by capture / load, or by the tests of last_batch_auc and path_switch themselves
HARNESS = {
    "tfr_set_table": "load; set_tables in every builder",
    "tfr_get_table": "capture",
    "tfr_get_step": "capture",
    "tfr_set_step": "load",
    "tfr_set_frozen": "give",
    "tfr_set_hyper": "give",
    "tfr_upload_triples": "give",
    "tfr_upload_eval_triples": "give",
    "tfr_bpr_set_positives": "give",
    "tfr_bpr_set_sampler": "give",
    "tfr_stage_ids": "give; tile_lookahead's staged form",
    "tfr_rng_seed": "every builder",
    "tfr_rng_set_state": "load",
    "tfr_rng_get_state": "capture",
    "tfr_train_step": "two_table, path_switch, the last_batch_auc tests",
    "tfr_train_steps_drawn": "two_table_drawn, tile_lookahead; the training that follows a guest",
    "tfr_train_steps_staged": "tile_lookahead, grown; the training that follows a guest",
    "tfr_train_step_ids": "in_flight",
    "tfr_kernel_plan": "assert_path in every builder",
    "tfr_sync": "in_flight's training that follows; the device-pointer guests",
    "tfr_last_batch_auc": "test_gpu_call_sequences.py: its value tests, and after every guest",
    "tfr_bf16_snapshot": "the stale-snapshot guest: taken before the state is built",
}

EXEMPT = {
    "tfr_destroy": "ends the handle: nothing follows it (every case closes its handles)",
    "tfr_profile": "per-kernel timing switches the look-ahead paths off by design; not a state the library promises bit-equality under",
    "tfr_profile_read": "reads the timing counters of tfr_profile",
    "tfr_shard_route_ids": "store-id form of tfr_shard_route (the guest): same routing core, held per stage in test_gpu_shard_stages.py",
    "tfr_shard_bucket_ids": "pre-split routing needs a second rank's records; held per stage in test_gpu_shard_stages.py",
    "tfr_shard_route_recs": "as tfr_shard_bucket_ids",
}


def _header_entries():
    text = open(os.path.join(ROOT, "include", "tfrecomm.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tfr_\w+)\s*\(\s*tfr_model\s*\*\s*\w", text)))


def _guest_entries():
    out = {}
    for name, g in H.GUESTS.items():
        for e in g.entries:
            out.setdefault(e, []).append(name)
    return out


def test_the_header_lists_the_handle_s_entry_points():
    names = _header_entries()
    assert len(names) > 80 and "tfr_forward" in names and "tfr_bf16_neighbours_dev" in names and "tfr_create" not in names
    assert not [n for n in names if n.startswith(("tfr_fm_", "tfr_svdpp_", "tfr_als_", "tfr_ials_"))]


def test_every_entry_point_is_placed():
    guests = _guest_entries()
    placed = set(guests) | set(HARNESS) | set(EXEMPT)
    missing = [n for n in _header_entries() if n not in placed]
    assert not missing, "no guest, builder or exemption for: %s" % ", ".join(missing)
    gone = sorted(placed - set(_header_entries()))
    assert not gone, "placed but not in the header: %s" % ", ".join(gone)
    both = sorted(set(EXEMPT) & (set(guests) | set(HARNESS)))
    assert not both, "exempt and used: %s" % ", ".join(both)
    assert all(len(r) > 20 for r in EXEMPT.values())


def test_a_guest_calls_the_entry_points_it_names():
    """through the engine.py method that calls them (or the library handle directly): the name a guest registers is backed by
    the source of the guest and of the SvdModel methods it calls"""
    from tfrecomm_amd import engine
    methods = {n: inspect.getsource(f) for n, f in inspect.getmembers(engine.SvdModel, inspect.isfunction)}
    helpers = {n: inspect.getsource(f) for n, f in inspect.getmembers(H, inspect.isfunction)}

    def reach(src, seen):
        found = set(re.findall(r"\btfr_\w+", src))
        nxt = [("m", k) for k in re.findall(r"\bm\.(\w+)\(", src) if k in methods]
        for stem in re.findall(r"getattr\(m, \"(\w+)\"", src):          # getattr(m, "similar_items" + suffix): every such method
            nxt += [("m", k) for k in methods if k.startswith(stem)]
        nxt += [("h", k) for k in re.findall(r"\b(_\w+|capture)\(", src) if k in helpers]
        for kind, k in nxt:
            if (kind, k) not in seen:
                seen.add((kind, k))
                found |= reach((methods if kind == "m" else helpers)[k], seen)
        return found
    for name, g in sorted(H.GUESTS.items()):
        found = reach(inspect.getsource(g.fn), set())
        missing = [e for e in g.entries if e not in found]
        assert not missing, "guest %s names %s but its source does not reach them (it reaches %s)" % (name, missing, sorted(found))


def test_every_guest_runs_in_every_state_or_says_why_not():
    run, why = H.cases()
    ran = {(v["state"], g) for v, g in run}
    for g in H.GUESTS:
        for state in H.STATES:
            assert (state, g) in ran or len(why.get((state, g)) or "") > 20, "%s never runs in %s and gives no reason" % (g, state)
    assert not set(why) & ran
    assert not why, "every state has a variant for every guest today (an nll one, a dense and a touched-rows optimiser): %r" % why


def test_the_plan_reaches_what_it_was_written_for():
    by = {}
    for v in H.VARIANTS:
        by.setdefault(v["state"], []).append(v)
    assert {v["D"] for v in by["two_table"]} == {16, 33, 8} and any(v["item_abs"] for v in by["two_table"])
    assert {(v["opt"], v["mode"]) for v in by["two_table"]} == {H.LAZY, H.SGD}
    assert {v["way"] for v in by["tile_lookahead"]} == {"drawn9", "drawn3", "staged"}
    assert {v["B"] for v in by["tile_lookahead"]} == {700, 2500}
    assert {(v["opt"], v["mode"]) for v in by["tile_lookahead"]} == {H.TF1, H.LAZY}
    assert {v["n"] for v in by["grown"]} == {256, 3000} and {v["B"] for v in by["grown"]} == {700}
    for state, vs in by.items():
        assert {v["loss"] for v in vs} == {"mse", "nll"}, state          # eval_binary and auc run in the nll variant of each
    assert [b for b, _ in H.PATH_SWITCH_STEPS] == [700, 16385, 65537, 700, 65537, 16385]
