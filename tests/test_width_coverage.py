"""Every instantiation a supported row width can reach is run by the GPU tests (tests/widths.py).

Each kernel family picks a template instantiation from D.  The rules are restated here in a few lines each, next to the
source they restate; the tests enumerate what every supported D reaches and check that the family's width list reaches all
of it.  A new width-templated kernel, or a change to a dispatch rule, belongs here together with its width list."""
import pytest

from tests import widths as W


def supported(D):
    """a row width the models accept: geometry() rejects lanes > 64 (csrc/dispatch.h geometry)"""
    return 1 <= D <= 64 or (D % 4 == 0 and D <= 256)


SUPPORTED = [D for D in range(1, 257) if supported(D)]


def geometry(D):
    """(G, VEC) of the SVD step and forward and of the FM kernels (csrc/dispatch.h geometry and ROW_GEOMETRIES, fm_kernels.hip launch_fm)"""
    vec = 4 if D % 4 == 0 else 1
    lanes = -(-D // vec)
    g = 4
    while g < lanes:
        g *= 2
    return g, vec


def shard_class(D):
    """(G, VEC, full width): k_gather_packed<G, VEC> takes unguarded non-temporal 16-byte loads where D == G * VEC and
    guarded ones elsewhere (csrc/shard.hip); the sharded reduce takes its three-round load form at full width
    (csrc/svd_kernels.h seg_reduce_pick)"""
    g, vec = geometry(D)
    return g, vec, D == g * vec


def registers(D):
    """(NJ, last register full): NJ = ceil(D / 64) features per lane, f = lane + 64 j guarded by f < D
    (csrc/wave_rows.h with_nj: the one dispatcher of svdpp.hip, finetune.hip and bpr.hip)"""
    return -(-D // 64), D % 64 == 0


def tile(D):
    """(V4, where the last group ends): mfma_tile_dot walks DP4 = ceil(D / 4) float4s in groups of four and masks the last
    group; V4 = (D % 4 == 0) picks the vector loads (csrc/score_tile.h mfma_tile_dot, score_tile.h launch_score_kernel, rank.hip).
    The first group alone, or DP4 % 4 once past it.  tfr_topk_plan / tfr_rank_plan pick no template argument from D."""
    dp4 = -(-D // 4)
    return D % 4 == 0, "first group" if dp4 <= 4 else "DP4 %% 4 = %d" % (dp4 % 4)


TOPK_ROUND = 4 * 32                                        # csrc/topk.h TOPK_WAVES * TOPK_SUB


def topk_queue(k):
    """(users per block, queue size) of k_topk_score (csrc/topk.h topk_cap, topk_upb)"""
    return (32, 256) if k + TOPK_ROUND <= 256 else (16, 512)


ALS_MAXD = 32                                              # csrc/als_kernels.hip


def _check(name, rule, listed, reachable):
    bad = [D for D in listed if not supported(D)]
    assert not bad, "%s: unsupported widths %s" % (name, bad)
    covered = {rule(D) for D in listed}
    missing = sorted(set(reachable) - covered, key=str)
    assert not missing, "%s: no width reaches %s (widths %s)" % (name, ", ".join(map(str, missing)), list(listed))


def test_there_are_ten_row_geometries():
    assert len({geometry(D) for D in SUPPORTED}) == 10
    assert {registers(D) for D in SUPPORTED} == {(nj, full) for nj in (1, 2, 3, 4) for full in (False, True)}
    assert len({tile(D) for D in SUPPORTED}) == 10


@pytest.mark.parametrize("name", ["SVD_SMALL", "SVD_BIG", "FM", "DP"])
def test_every_row_geometry(name):
    _check(name, geometry, getattr(W, name), {geometry(D) for D in SUPPORTED})


def test_sharded_stages_reach_every_geometry_at_full_and_partial_width():
    reachable = {shard_class(D) for D in SUPPORTED}
    assert len(reachable) == 15 and not any(full for _, vec, full in reachable if vec == 1)
    _check("SHARD", shard_class, W.SHARD, reachable)


def test_fm_step_reaches_every_geometry_at_full_and_partial_width():
    """k_fm_forward<G, VEC, ...> branches on D == G * VEC (csrc/fm_kernels.hip `full`), and seg_reduce_pick (csrc/svd_kernels.h) gives the FM
    backward its three-round load form at full width only: the classes of ``shard_class``"""
    reachable = {shard_class(D) for D in SUPPORTED}
    assert len(reachable) == 15
    _check("FM_STEP", shard_class, W.FM_STEP, reachable)


def bf16_class(D):
    """(lanes per rating G, the group is wider than the row): k_forward_bf16<G, ...> is picked by G = the smallest power of
    two >= DP / 8, DP = 8 * ceil(D / 8) (csrc/bf16_rows.h bf16_geometry); where G * 8 > DP the lanes past DP / 8 have no
    fragment and Bf16Rows::load aims them at the row's first one (csrc/bf16_rows.hip)"""
    from tests import bf16_cases
    g = bf16_cases.lanes(D)
    return g, g * 8 > bf16_cases.row_stride(D)


def test_forward_pnt_reaches_every_geometry_at_full_and_partial_width():
    """launch_forward_mode picks k_forward<G, VEC, MODE, 4, PNT> by with_geometry (csrc/dispatch.h) and forward_pnt (csrc/svd_kernels.hip);
    load_frag<VEC, true> guards its non-temporal load by d0 < D, which is false for some lane only below full width"""
    reachable = {shard_class(D) for D in SUPPORTED}
    assert len(reachable) == 15
    _check("FORWARD_PNT", shard_class, W.FORWARD_PNT, reachable)


def test_bf16_pnt_reaches_every_lane_count_with_and_without_spare_lanes():
    reachable = {bf16_class(D) for D in SUPPORTED}
    assert {g for g, _ in reachable} == {1, 2, 4, 8, 16, 32} and len(reachable) == 10
    assert bf16_class(100) == (16, True)                    # the example of csrc/bf16_rows.hip: lanes 13..15
    _check("BF16_PNT", bf16_class, W.BF16_PNT, reachable)


def test_listed_pnt_widths_take_the_non_temporal_kernels_at_the_tests_table_size(monkeypatch):
    """tfr_forward_plan answers by the functions the launch calls (csrc/api.hip forward_plan): at the U the GPU tests build,
    every listed width reports PNT = true for INFER and EVAL, and one row fewer reports false; TRAIN never streams"""
    from tests import forward_cases as F
    monkeypatch.delenv("TFR_BF16_PNT", raising=False)         # the snapshot's A/B override would answer instead of the rule
    seen = set()
    for rows, listed in ((F.F32, W.FORWARD_PNT), (F.BF16, W.BF16_PNT)):
        for D in listed:
            U = F.pnt_rows(D, F.row_bytes(D, rows))
            for mode in (F.INFER, F.EVAL):
                name, args, _ = F.plan(D, U, mode, rows)
                assert args[-1] is True, (D, U, mode, rows, name, args)
                assert F.plan(D, U - 1, mode, rows)[1] == args[:-1] + (False,), (D, U - 1, mode, rows)
                seen.add((name, args))
        if rows == F.F32:
            assert all(F.plan(D, F.pnt_rows(D, 4 * D), F.TRAIN, rows)[1][-1] is False for D in listed)
    # every PNT instantiation the library compiles: ten geometries and six lane counts, INFER and EVAL
    assert len({a for n, a in seen if n == "k_forward"}) == 20 and len({a for n, a in seen if n == "k_forward_bf16"}) == 12


def test_the_gpu_tests_take_their_widths_from_these_lists():
    """a width list only guards what runs at it: the BPR, sharded, data-parallel and FM step GPU tests parametrise over these"""
    import ast
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for fname, name in (("test_gpu_bpr.py", "BPR"), ("shard_cases.py", "SHARD"), ("shard_cases.py", "DP"),
                        ("fm_cases.py", "FM_STEP"), ("test_gpu_fm.py", "FM_STEP"),
                        ("test_gpu_forward_paths.py", "FORWARD_PNT"), ("test_gpu_forward_paths.py", "BF16_PNT"),
                        ("test_forward_paths_host.py", "FORWARD_PNT"), ("test_forward_paths_host.py", "BF16_PNT")):
        tree = ast.parse(open(os.path.join(here, fname)).read())
        used = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "W"}
        assert name in used, "%s does not read widths.%s" % (fname, name)
    # test_gpu_fm_step.py runs the case list of fm_cases.py, whole
    tree = ast.parse(open(os.path.join(here, "test_gpu_fm_step.py")).read())
    used = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "C"}
    assert "CASES" in used, "test_gpu_fm_step.py does not run fm_cases.CASES"
    from tests import fm_cases
    assert {c["D"] for c in fm_cases.CASES if c["kind"] == "edges"} >= set(W.FM_STEP)
    from tests import test_gpu_bpr
    assert test_gpu_bpr.WIDTHS is W.BPR, "test_gpu_bpr.py keeps a private WIDTHS list"
    assert set(W.BPR) >= {1, 33, 64, 100, 128, 132, 192, 252, 256}, "BPR: the widths the BPR tests ran at must not shrink"


@pytest.mark.parametrize("name", ["SVDPP", "FINETUNE", "BPR"])
def test_every_register_count_full_and_partial(name):
    _check(name, registers, getattr(W, name), {registers(D) for D in SUPPORTED})


def test_streamed_fine_tuning_at_every_register_count():
    nj = lambda D: registers(D)[0]
    _check("FINETUNE_STREAMED", nj, W.FINETUNE_STREAMED, {nj(D) for D in SUPPORTED})


@pytest.mark.parametrize("name", ["TOPK", "RANK"])
def test_every_tile_load_and_last_group(name):
    _check(name, tile, getattr(W, name), {tile(D) for D in SUPPORTED})


def test_topk_k_reaches_both_queue_sizes():
    got = {topk_queue(k) for k in W.TOPK_KS}
    assert got == {topk_queue(k) for k in range(1, 257)}, got


def test_random_rank_and_fm_ranking_widths():
    v4 = lambda D: D % 4 == 0
    _check("RANK_RANDOM", v4, W.RANK_RANDOM, {False, True})
    _check("FM_TOPK", v4, W.FM_TOPK, {False, True})
    assert max(W.FM_TOPK) > 128, "FM_TOPK: no width above 128"


def test_als_reaches_both_ends_of_the_one_wave_cholesky():
    for name in ("ALS", "ALS_CHUNKED"):
        listed = getattr(W, name)
        assert all(1 <= d <= ALS_MAXD for d in listed), (name, listed)
    assert {1, ALS_MAXD} <= set(W.ALS), "ALS: d = 1 and d = %d not both listed" % ALS_MAXD
    assert ALS_MAXD in W.ALS_CHUNKED, "ALS_CHUNKED: no chunked long list at d = %d" % ALS_MAXD


def als_step_class(d):
    """(live A-entry slots, last slot exactly full, one staging pass, end of the range): k_als_fit and k_als_partial keep
    entry t = tid + 256 q of A in acc[q], so ceil(d * d / 256) slots are live and the last is full where d * d is a multiple
    of 256; als_accumulate stages a 32-rating tile with `for (t = tid; t < nk * d; t += 256)`, one pass while 32 d <= 256
    (csrc/als_kernels.hip).  A range of widths with the same slots and passes is run at its lowest and its highest d."""
    key = lambda x: (-(-x * x // 256), -(-32 * x // 256) == 1)
    first = d == 1 or key(d - 1) != key(d)
    last = d == ALS_MAXD or key(d + 1) != key(d)
    return key(d)[0], d * d % 256 == 0, key(d)[1], "lowest d" if first else "highest d" if last else "inside"


def test_als_step_reaches_both_ends_of_every_slot_count_and_staging_form():
    assert all(1 <= d <= ALS_MAXD for d in W.ALS_STEP), W.ALS_STEP
    reachable = {als_step_class(d) for d in range(1, ALS_MAXD + 1)}
    assert {c[0] for c in reachable} == {1, 2, 3, 4} and {c[:2] for c in reachable if c[1]} == {(1, True), (4, True)}
    wanted = {c for c in reachable if c[3] != "inside"}
    assert len(wanted) == 10
    covered = {als_step_class(d) for d in W.ALS_STEP}
    missing = sorted(wanted - covered)
    assert not missing, "ALS_STEP: no width reaches %s (widths %s)" % (", ".join(map(str, missing)), list(W.ALS_STEP))
    from tests import als_cases
    assert {c["d"] for c in als_cases.CASES if c["id"].startswith("tile_edges")} >= set(W.ALS_STEP)
