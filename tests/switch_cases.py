"""The environment switches of DESIGN.md §23 as plain data: for every switch the non-default settings that are run, the
workloads a setting touches, how the switched run must relate to the default one, the reason read off the code, and the
test that holds it.  tests/test_switch_coverage.py (no GPU) holds this table against csrc/ and DESIGN.md;
tests/test_gpu_switches.py runs the entries marked ``new``, each setting in a child process of its own (the library keeps
most switches in a ``static const``).

Relations:
  bits       both sides add the same values in the same order - every table, Adam slot, loss and logit of the switched run
             equals the default run's bit for bit;
  reference  the order of a sum differs - no tolerance between the two sides; each side's host-fed steps are held to
             tests/step_ref.py ``check_step`` at that module's limits, and each side's staged run equals its own
             host-fed run bit for bit.
The sort and draw workloads are index work: exact against NumPy on both sides (``bits``).

Nothing here is measured on the code under test: the relations come from reading the kernels, the shapes from the
dispatch rules restated in tests/step_cases.py and tests/test_width_coverage.py."""
import numpy as np

from tests.util import dup_heavy_ids, rand_tables

NEW = "new"
BITS, REFERENCE = "bits", "reference"

# ----------------------------------------------------------------------------- workloads
# big: the SVD_BIG shape of the suite (one side above CSORT_MAX_BINS rows: radix sort, fused k_seg_reduce, k_apply_rows),
# duplicate-heavy ids so that runs are cut at block boundaries.  Three full batches and a ragged one (B - 37): host-fed
# single steps, then the same batches staged - one train_steps_staged call of three steps (the look-ahead pipeline, both
# buffer sets) and the ragged batch restaged for a call of its own (a staged call has one batch size).
BIG_U, BIG_I, BIG_B, BIG_RAGGED = 16384 + 77, 300, 3000, 37
BIG_OPTS = (("adam", "lazy"), ("sgd", "tf1"))
BIG_GENERAL = (33, 100)        # not full width: seg_reduce_pick cannot give them the FAST form, which ignores nt, LEAN and stage_sum
BIG_STREAM = (64, 100)         # sort, gather and event order: a full-width row (the default's three-round form) and a general one
BIG_LONG_B = 65536 + 5         # the first batch size the default sorts in 4096-key tiles: the narrow pass above its usual range
BIG_LONG = ((64, ("adam", "lazy")), (33, ("sgd", "tf1")))

# tiles: tests/test_gpu_arg_preload.py's tables; TF1 Adam, host-fed and staged
TILE_U, TILE_I = 300, 200
TILE_SHAPES = ((64, 2049), (64, 10000), (15, 2049), (15, 10000), (128, 10000))      # (D, B)

# sort: sort_segments against np.argsort(kind="stable"), the hot-id and equal-block pattern of test_radix_sort_edges
SORT_WIDE_MIN_B = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 12289)   # one key, one wave, tile edges, short last tiles
SORT_WIDE_MIN_N = (20_000, 20_000_000)                                               # two and four passes
# k_rsort_scatter (csrc/sort.hip) takes the totals of the scan blocks in front of an entry from an LDS prefix of
# PREF = 2 * CSORT_TILE = 2048 of them once there are more than 32 (`use_pref = nb > 32`), nb = ceil(256 * ntiles / 4096),
# ntiles = ceil(B / 1024): 32 blocks up to B = 512 * 1024, 33 from one key more; 2048 up to B = 32768 * 1024 and 2049
# (one total added behind the prefix) from one key more.
RSORT_PREF, RSORT_CHUNK, RSORT_TILE = 2048, 4096, 1024
SORT_NARROW_B = (65536, 100_000, 300_001, 32 * 16 * RSORT_TILE, 32 * 16 * RSORT_TILE + 1)
SORT_NARROW_N = 20_000
SORT_NARROW_PREF_B = (RSORT_PREF * 16 * RSORT_TILE, RSORT_PREF * 16 * RSORT_TILE + 1)   # 33 554 432 and one more
SORT_NARROW_PREF_N = 300_000                                                            # 19 key bits: three passes


def scan_blocks(B):
    """nb of k_rsort_scatter for B keys (csrc/sort.hip)"""
    ntiles = -(-B // RSORT_TILE)
    return -(-256 * ntiles // RSORT_CHUNK)


def big_tables(D):
    return rand_tables(np.random.RandomState(300 + D), BIG_U, BIG_I, D, scale=0.3 / np.sqrt(max(D, 16) / 16))


def big_batches(B):
    """three batches of B and one of B - BIG_RAGGED"""
    rs = np.random.RandomState(B + 1)
    return [(dup_heavy_ids(rs, BIG_U, n), dup_heavy_ids(rs, BIG_I, n), rs.randint(1, 6, n).astype(np.float32))
            for n in (B, B, B, B - BIG_RAGGED)]


def sort_ids(n, B):
    rs = np.random.RandomState((n + B) % 100003)
    ids = rs.randint(0, n, B).astype(np.int32)
    if B > 1000:
        ids[rs.rand(B) < 0.33] = ids[0]
        ids[B // 2: B // 2 + 500] = n - 1
    return ids


# which workloads a child runs: name -> what tests/switch_workloads.py runs for it
WORKLOADS = ("big_general", "big_stream", "big_long", "tiles", "sort_wide_min", "sort_narrow", "draw")


def _entry(name, settings, workloads, relation, reason, held_by=NEW, plan=None):
    return dict(name=name, settings=tuple(settings), workloads=tuple(workloads), relation=relation, reason=reason,
                held_by=held_by, plan=plan)


def _held(name, fname, test, relation, reason):
    return _entry(name, (), (), relation, reason, held_by=(fname, test))


# ``plan``: how a pair of runs shows that it took two forms - "differs": the kernel_plan strings differ; "gather": a
# k_gather_triples count above zero in a single profiled step after the compared run; "branch": nothing beyond the
# non-default branch having been taken (the same kernels in another event order, or a kernel kernel_plan does not name).
CASES = (
    # ---- run by tests/test_gpu_switches.py
    _entry("TFR_LEAN", [{"TFR_LEAN": "0"}], ["big_general"], BITS,
           "k_seg_reduce: `w = (FWD && LEAN) ? load_frag(wsrc) : o` - the row kept in registers is the row re-read, nothing wrote it in between",
           plan="differs"),
    _entry("TFR_NT", [{"TFR_NT": "0"}, {"TFR_NT": "31"}, {"TFR_NT": "31", "TFR_DUALQ": "0"}, {"TFR_NT": "7", "TFR_DUALQ": "0"}],
           ["big_general"], BITS,
           "RedArgs::nt only picks load_frag_h / store_frag_h's cache policy; bits 8 and 16 (partner_by_pos, own_copy_out) exist with "
           "TFR_DUALQ=0 only, which test_two_table_form_is_bit_identical_to_the_copy_form holds bit-identical itself", plan="branch"),
    _entry("TFR_STAGE_SUM", [{"TFR_STAGE_SUM": "0"}], ["big_general"], REFERENCE,
           "k_seg_reduce: `a.stage_sum ? block_sum_pieces<G, 1> : block_sum_store<3, 16>` - the per-block {loss, reg, sum g} are added in "
           "another order, so loss, reg and bias_global differ in the last bits", plan="branch"),
    _entry("TFR_FUSE_GATHER", [{"TFR_FUSE_GATHER": "0"}], ["big_stream"], BITS,
           "front_and_sort: k_gather_triples writes the same (u, i, r) the first radix pass would gather itself; the sort reads them",
           plan="gather"),
    _entry("TFR_SORT_LATE", [{"TFR_SORT_LATE": "0"}], ["big_stream"], BITS,
           "staged_steps_lookahead: the same launches, the look-ahead chain ordered behind ev_first / ev_free instead of ev_mid", plan="branch"),
    _entry("TFR_NO_LOOKAHEAD", [{"TFR_NO_LOOKAHEAD": "1"}], ["big_stream"], BITS,
           "staged_steps: the same gather + sort + step launches, back to back on one stream", plan="branch"),
    _entry("TFR_RSORT_WIDE_MIN", [{"TFR_RSORT_WIDE_MIN": "1"}], ["big_stream", "sort_wide_min"], BITS,
           "a stable sort has one answer: k_rsortw_hist/scatter on a short only tile (with its own gather when staged) must give k_rsort_*'s order",
           plan="differs"),
    _entry("TFR_RSORT_WIDE", [{"TFR_RSORT_WIDE": "0"}], ["big_long", "sort_narrow"], BITS,
           "a stable sort has one answer: k_rsort_rank/scatter from 65536 keys up (with their gather when staged) must give k_rsortw_*'s order",
           plan="differs"),
    _entry("TFR_TILE_SPLIT", [{"TFR_TILE_SPLIT": "1"}], ["tiles"], REFERENCE,
           "k_seg_reduce in tile mode adds a run's entries one by one in sorted order, k_tile_step in wave-level doubling rounds; "
           "the forward's per-block sums come from k_front's blocks instead of one slot per piece", plan="differs"),
    _entry("TFR_EPG", [{"TFR_EPG": "1"}, {"TFR_EPG": "2"}, {"TFR_EPG": "4"}], ["tiles"], BITS,
           "k_tile_step<G, VEC, EPG>: a piece is 1024 / G entries whatever the block holds; block_sum_pieces adds each piece's values in "
           "its own fixed order and the sweep adds a row's pieces in piece order", plan="differs"),
    _entry("TFR_RNG_WIDE", [{"TFR_RNG_WIDE": "0"}], ["draw"], BITS,
           "ensure_rng leaves the wide scratch unset, launch_mt_draw then runs k_mt_draw alone: the same MT19937 stream, checked against NumPy",
           plan="branch"),
    # ---- held by tests that were there before this table
    _held("TFR_DUALQ", "test_gpu_parity.py", "test_two_table_form_is_bit_identical_to_the_copy_form", BITS,
          "the copy holds the pre-update item row the other table still holds"),
    _held("TFR_FAST", "test_gpu_parity.py", "test_three_round_load_form_is_bit_identical_to_the_general_form", BITS,
          "the three-round form loads earlier, adds in the same order"),
    _held("TFR_WT", "test_gpu_tile_pieces.py", "test_every_switch_setting_gives_the_same_step", BITS, "how bytes are stored, nothing else"),
    _held("TFR_ITEM_SPLIT", "test_gpu_tile_pieces.py", "test_every_switch_setting_gives_the_same_step", BITS,
          "pieces do not depend on the block split"),
    _held("TFR_ONE_BARRIER", "test_gpu_tile_pieces.py", "test_every_switch_setting_gives_the_same_step", REFERENCE,
          "another order of the cross-wave sums: held to the oracle"),
    _held("TFR_SWEEP_ROUNDS", "test_gpu_sweep_rounds.py", "test_optimiser_modes", BITS, "the same pieces added in piece order"),
    _held("TFR_RECS", "test_gpu_rng.py", "test_records_beside_the_drawn_ids_are_invisible", BITS, "the records are copies of the store rows"),
    _held("TFR_LDS_REDUCE", "test_gpu_forward_paths.py", "test_lds_group_sum_matches_the_float64_values_and_the_butterfly", REFERENCE,
          "lane order instead of the butterfly's"),
    _held("TFR_CHUNK_STEPS", "test_gpu_draw_chunks.py", "test_every_chunk_cap_gives_the_same_steps", BITS, "where the id stream is cut, not what it holds"),
    _held("TFR_FM_VARIANT", "test_gpu_fm.py", "test_fm_forward_load_forms_agree_and_hold_per_row", BITS, "cache policy of the V rows"),
    _held("TFR_FM_BF16_NTV", "test_gpu_fm_bf16.py", "test_forward_holds_per_row_on_round_tripped_rows_in_every_entry_and_load_form", BITS,
          "cache policy of the V rows"),
    _held("TFR_BF16_PNT", "test_gpu_forward_paths.py", "test_bf16_pnt_equals_the_plain_loads_bit_for_bit", BITS, "cache policy of the user rows"),
    _held("TFR_ALS_CHUNK", "test_gpu_als_step.py", "test_chunked_and_unchunked_loads_agree", REFERENCE, "chunk sums are added chunk by chunk"),
    _held("TFR_RNG_WIDE_TRIM", "test_gpu_rng.py", "test_wide_draw_that_comes_up_short_is_finished_by_the_sequential_kernel", BITS,
          "the sequential kernel continues the same stream"),
)

# diagnostic switches: they change what is printed or stamped, not what is computed
EXEMPT = {
    "TFR_CALL_TRACE": "prints host-side time marks of a multi-step call on stderr; no kernel or argument depends on it",
    "TFR_TILE_DEBUG": "per-block time stamps of k_tile_step on stderr; tests/test_gpu_tile_pieces.py test_item_side_takes_the_spare_cus "
                      "already runs it and reads its block counts",
    "TFR_RNG_DEBUG": "reserves two words for the generator's in-kernel clock; the ids do not depend on it",
}

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES) and not set(BY_NAME) & set(EXEMPT)
NEW_CASES = tuple(c for c in CASES if c["held_by"] == NEW)


def setting_id(env):
    return "-".join("%s=%s" % (k[4:], v) for k, v in sorted(env.items()))


# one child per setting: (id, env, entry)
CHILDREN = tuple((setting_id(env), env, c) for c in NEW_CASES for env in c["settings"])
