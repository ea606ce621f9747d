"""Every kernel of the interaction-list families is run by a GPU test and held to a restatement there (tests/list_paths.py).

The families of csrc/item_lists.h pick a template instantiation from K, loop over query chunks, and PureSVD branches on r.
The rules are restated here in a few lines each, next to the source they restate, and checked against the library's plan
functions where those expose them (the plans need no device).  The manifest is the list: every `kernel` line that
profiles/kernel_manifest.txt holds for itemknn.hip, userknn.hip, ease.hip, slim.hip and puresvd.hip must be reached by a class
that a list of tests/list_paths.py covers, or stand in EXEMPT with the test that holds it.  A new instantiation, or a change to
a dispatch rule, belongs here together with its list."""
import ast
import os
import re

import pytest

from tests import list_paths as LP

HERE = os.path.dirname(os.path.abspath(__file__))
MANIFEST = os.path.join(HERE, os.pardir, "profiles", "kernel_manifest.txt")
FILES = ("itemknn.hip", "userknn.hip", "ease.hip", "slim.hip", "puresvd.hip")

KMAX = 256                                                 # csrc/topk.h TOPK_KMAX
CHUNK_MAX = 65536                                          # csrc/itemknn.h KNN_CHUNK_MAX, csrc/ease.h EASE_CHUNK_MAX
PART_BYTES = 128 << 20                                     # csrc/topk.h TOPK_PART_BYTES
PSVD_MAX_R, PSVD_LDS_MAX = 128, 160 * 1024                 # csrc/puresvd.h


# ---- the dispatch rules, restated ------------------------------------------------------------------------------------------------
def knn_rounds(K):
    """64-lane rounds that cover one neighbour row (csrc/itemknn.h knn_rounds; KnnServe::launch and UknnServe::launch pick
    k_knn_score<R, MODE> and k_uknn_score<R, MODE> by it)"""
    return 1 if K <= 64 else 2 if K <= 128 else 4


def knn_fit_cap(K):
    """keys of a fit wave's queue: the kept K plus one 64-lane append, a power of two (csrc/itemknn.h knn_fit_cap)"""
    return 256 if K + 64 <= 256 else 512


def fit_lds(cap):
    """csrc/itemknn.h knn_fit_lds and knn_wfit_lds: 64 KiB of counters, four queues, four counts"""
    return 16384 * 4 + 4 * cap * 8 + 4 * 4


SERVING_MODES = {"recommend": (0,), "rank_items": (1, 2)}  # csrc/item_lists.h topk_run: launch<0>; rank_users: launch<1>, launch<2>


def score_class(K):
    """(R, the row fills its rounds): slot < K masks no lane of the last round where K == 64 R"""
    return knn_rounds(K), K == 64 * knn_rounds(K)


def fit_class(K):
    """(CAP, where K sits on that queue): "tightest" where K + 64 == CAP, so that an append fills the queue to its last slot
    before queue_compact (csrc/item_lists.h queue_offer: cnt > CAP - 64); "smallest" for the first K of a queue size"""
    cap = knn_fit_cap(K)
    at = "tightest" if K + 64 == cap else "smallest" if K == 1 or knn_fit_cap(K - 1) != cap else "inside"
    return cap, at


def psvd_rot_in_lds(r):
    """the rotations sit in LDS beside T where both fit (csrc/puresvd.h psvd_rot_in_lds; psvd_mat_lds has row stride r + 1)"""
    return 2 * r * (r + 1) * 8 + 4096 <= PSVD_LDS_MAX


def jacobi_lds(r):
    return (2 if psvd_rot_in_lds(r) else 1) * r * (r + 1) * 8 + 4096


def eig_class(r):
    """(rotations in LDS, r odd: index r sits out of every round, pairs per round) with the pairs capped at "several" """
    return psvd_rot_in_lds(r), r % 2 == 1, min((r + 1) // 2, 2) if r > 1 else 0


def spmm_kernels(widths, chunked):
    """k_psvd_spmm<EVEN, PART> (csrc/puresvd.hip launch_spmm): EVEN = (width % 2 == 0); the PART launch runs where a list is
    longer than the chunk, the row launch always"""
    return {("k_psvd_spmm", (int(w % 2 == 0), int(part))) for w in widths for part in ((0, 1) if chunked else (0,))}


def serving_chunk(n_rows, slices, k):
    """queries per chunk (csrc/itemknn.h knn_plan, csrc/ease.h ease_plan; uknn_plan and tfr_slim_plan go through them)"""
    chunk = 1 if n_rows < 1 else min(n_rows, CHUNK_MAX)
    return max(1, min(chunk, PART_BYTES // (slices * k * 8)))


# ---- the restatements against the library ----------------------------------------------------------------------------------------
def test_the_fit_cap_is_the_one_the_plans_report():
    from tfrecomm_amd import itemknn, rp3beta, userknn
    assert {fit_lds(256), fit_lds(512)} == {73744, 81936}
    for K in range(1, KMAX + 1):
        want = fit_lds(knn_fit_cap(K))
        got = (itemknn.plan(2304, K, 2304, 0)["lds"], rp3beta.weighted_plan(2304, K, 2304)["lds"], userknn.plan(2304, K, 2304, 0)["lds"],
               userknn.plan(2304, K, 10, 2)["lds"])
        assert got == (want,) * 4, (K, got, want)
    assert [knn_fit_cap(K) for K in (1, 192, 193, 256)] == [256, 256, 512, 512]
    assert [knn_rounds(K) for K in (1, 64, 65, 128, 129, 256)] == [1, 1, 2, 2, 4, 4]


def test_the_jacobi_form_is_the_one_the_plan_reports():
    from tfrecomm_amd import puresvd
    for r in range(1, PSVD_MAX_R + 1):
        assert puresvd.plan(10, 10, r, 0)["lds_bytes"] == jacobi_lds(r) <= PSVD_LDS_MAX, r
    assert [r for r in range(1, PSVD_MAX_R) if psvd_rot_in_lds(r) != psvd_rot_in_lds(r + 1)] == [99]


@pytest.mark.parametrize("family", LP.CHUNKED_FAMILIES)
def test_the_chunk_rule_is_the_one_the_plans_report(family):
    from tfrecomm_amd import ease, itemknn, slim, userknn
    plan = {"knn": itemknn.plan, "ease": ease.plan, "slim": slim.plan, "uknn": userknn.plan}[family]
    for n_items in (9, 1025, 8193, 16000):                 # SLIM's cap is 16384 items
        for k in (1, 10, 256):
            for n_rows in (0, 1, 3000, CHUNK_MAX, CHUNK_MAX + 2, 10 ** 7):
                p = plan(n_items, k, n_rows, 1)
                assert p["slices"] == -(-n_items // p["width"])
                assert p["chunk"] == serving_chunk(n_rows, p["slices"], k), (family, n_items, k, n_rows, p)
    # the chunked cases of tests/test_gpu_list_paths.py: the row cap on the tiny catalogue, the key bytes on the two-slice one
    assert all(plan(9, k, 10 ** 7, 1)["chunk"] == CHUNK_MAX for k in LP.CHUNKED_KS)
    if family == LP.CHUNKED_BY_BYTES[0]:
        p = plan(LP.CHUNKED_BY_BYTES[1], LP.CHUNKED_BY_BYTES[2], 10 ** 7, 1)
        assert p["slices"] == 2 and p["chunk"] == 32768
    if family == "uknn":
        assert all(userknn.plan(7, K, 10 ** 7, 2)["chunk"] == CHUNK_MAX for K in (3,) + LP.UKNN_LIST_KS)


# ---- the lists reach every class -------------------------------------------------------------------------------------------------
def _missing(name, rule, listed, wanted):
    missing = sorted(set(wanted) - {rule(v) for v in listed}, key=str)
    return ["%s: no value reaches %s (values %s)" % (name, c, list(listed)) for c in missing]


def test_the_score_ks_reach_every_round_count_full_and_one_over():
    reachable = {score_class(K) for K in range(1, KMAX + 1)}
    assert reachable == {(R, full) for R in (1, 2, 4) for full in (False, True)}
    missing = sorted(reachable - {score_class(K) for K in LP.KNN_SCORE_KS})
    assert not missing, "; ".join("KNN_SCORE_KS %s: no K runs k_knn_score<%d, MODE> and k_uknn_score<%d, MODE> with the row %s" % (
        list(LP.KNN_SCORE_KS), R, R, "full (K = %d)" % (64 * R) if full else "partly filled (K < %d)" % (64 * R)) for R, full in missing)
    # both sides of each change of R
    edges = {K for K in range(1, KMAX) if knn_rounds(K) != knn_rounds(K + 1)}
    assert all(K in LP.KNN_SCORE_KS and K + 1 in LP.KNN_SCORE_KS for K in edges), sorted(edges)
    assert {1, KMAX} <= set(LP.KNN_SCORE_KS)


@pytest.mark.parametrize("name", ["KNN_FIT_KS", "UKNN_LIST_KS"])
def test_the_fit_ks_reach_both_queue_edges(name):
    wanted = {fit_class(K) for K in range(2, KMAX + 1)} - {(256, "inside"), (512, "inside")}
    assert wanted == {(256, "tightest"), (512, "smallest")}
    bad = _missing(name, fit_class, getattr(LP, name), wanted)
    assert not bad, "; ".join(bad)


def test_the_eigen_sizes_reach_both_rotation_stores_odd_and_even():
    reachable = {eig_class(r) for r in range(1, PSVD_MAX_R + 1)}
    bad = _missing("PSVD_EIG_SIZES", eig_class, LP.PSVD_EIG_SIZES, reachable)
    assert not bad, "; ".join(bad)
    assert {1, 2, 3, 4, 99, 100, PSVD_MAX_R} <= set(LP.PSVD_EIG_SIZES)        # r = 1 .. 4, both sides of the LDS edge, the widest
    from tests import puresvd_cases
    assert puresvd_cases.EIG_SIZES is LP.PSVD_EIG_SIZES, "tests/puresvd_cases.py keeps a private EIG_SIZES"
    f, o = LP.PSVD_WIDE_FIT
    assert eig_class(f + o) == (False, True, 2) and f % 2 == 0 and f + o <= PSVD_MAX_R


def test_the_staircases_rise_under_every_fit_they_are_run_with():
    """every 64 columns a wave scans beat all it has kept: row 0's similarity is strictly higher on each step of the
    staircase than on the one before, for the metrics of test_fit_queue_edges_on_the_staircase"""
    import numpy as np
    from tests import itemknn_cases as IC
    from tests import itemknn_ref as R
    from tests import rp3_ref as R3
    indptr, items, nu, ni = IC.case("staircase")
    steps = ni // 64
    c = np.arange(1, steps + 1)                            # c(0, j) on step j // 64 = users 0 .. j // 64 = n_j (item 0 aside)
    assert nu == steps and np.bincount(items, minlength=ni)[64::64].tolist() == c[1:].tolist()
    for metric in ("cosine", "count"):
        s = R.similarity(c, np.full(steps, nu), c, metric, 0.0)
        assert (np.diff(s) > 0).all(), metric
    q, rs, cs, shift = R3.rp3_terms(indptr, items, nu, ni, 1.0, 0.6)
    s = ((np.cumsum(q.astype(np.float64)) * 2.0 ** -shift) * rs[0]) * cs[64 * np.arange(steps) + 1]
    assert (np.diff(s.astype(np.float32)) > 0).all()


# ---- the manifest is the list ----------------------------------------------------------------------------------------------------
def manifest_kernels(path=MANIFEST, files=FILES):
    """{(base name, template arguments)} of the `kernel` lines under the `== <file>` headers named: the base name is the
    lowercase k_... run of the mangled symbol, the arguments its Li<n>E / Lb<n>E groups"""
    out, inside = {}, None
    for line in open(path):
        if line.startswith("== "):
            inside = line[3:].split(":")[0].strip()
            continue
        if inside in files and line.startswith("kernel "):
            symbol = line.split()[1]
            base = re.search(r"k_[a-z0-9_]+", symbol)
            assert base, "no k_... name in %s" % symbol
            args = tuple(int(v) for v in re.findall(r"L[ib](\d+)E", symbol))
            out[(base.group(0), args)] = inside
    return out


def reached():
    """{kernel: the list of tests/list_paths.py whose test launches it and holds it to a restatement}"""
    out = {}
    for K in LP.KNN_SCORE_KS:
        for modes in SERVING_MODES.values():               # test_every_scoring_round_and_mode...: recommend and rank_items
            for mode in modes:
                out[("k_knn_score", (knn_rounds(K), mode))] = "KNN_SCORE_KS"
                out[("k_uknn_score", (knn_rounds(K), mode))] = "KNN_SCORE_KS"
    for K in LP.KNN_FIT_KS:                                # test_fit_queue_edges_on_the_staircase: tfr_knn_fit and the weighted fit
        out[("k_knn_cooc", (knn_fit_cap(K),))] = "KNN_FIT_KS"
        out[("k_knn_cooc_w", (knn_fit_cap(K),))] = "KNN_FIT_KS"
    for K in LP.UKNN_LIST_KS:
        out[("k_uknn_query_cooc", (knn_fit_cap(K),))] = "UKNN_LIST_KS"
    if "ease" in LP.CHUNKED_FAMILIES and "slim" in LP.CHUNKED_FAMILIES:       # SLIM serves through EASE's scoring launches
        out[("k_ease_score", (0,))] = "CHUNKED_FAMILIES"
    if LP.PSVD_EIG_SIZES:
        out[("k_psvd_jacobi", ())] = "PSVD_EIG_SIZES"
    f, o = LP.PSVD_WIDE_FIT                                # the fit multiplies at r and at `factors`; both sides hold a long list
    for kernel in spmm_kernels((f + o, f), chunked=True):
        out[kernel] = "PSVD_WIDE_FIT"
    return out


# kernels the lists above do not place: where each is held to a restatement already
EXEMPT = {
    ("k_ease_score", (1,)): "tests/test_gpu_ease.py test_rank_is_the_position_in_recommend and test_recommend_and_rank_at_the_slice_edges",
    ("k_ease_score", (2,)): "tests/test_gpu_ease.py test_rank_is_the_position_in_recommend and test_recommend_and_rank_at_the_slice_edges",
    ("k_ease_gram", ()): "tests/test_gpu_ease.py test_gram_bit_for_bit against tests/ease_ref.py gram",
    ("k_ease_diag", ()): "tests/test_gpu_ease.py test_inverse_exact_integers and test_inverse_within_the_error_constant",
    ("k_ease_gemm", ()): "tests/test_gpu_ease.py test_inverse_exact_integers; PureSVD's products in tests/test_gpu_puresvd.py",
    ("k_ease_copy", ()): "tests/test_gpu_ease.py test_inverse_exact_integers: a stage of the blocked inverse",
    ("k_ease_mirror", ()): "tests/test_gpu_ease.py test_inverse_exact_integers: the inverse is compared whole",
    ("k_ease_weights", ()): "tests/test_gpu_ease.py test_weights_bit_for_bit_from_the_device_inverse",
    ("k_slim_diag", ()): "tests/test_gpu_slim.py test_solve_bit_for_bit: the solver's diagonal, every case",
    ("k_slim_cd", ()): "tests/test_gpu_slim.py test_solve_bit_for_bit and test_solve_bit_for_bit_past_the_grid",
    ("k_psvd_chol", ()): "tests/test_gpu_puresvd.py test_orthonormalise_against_the_long_double_restatement, r 1 to 128",
    ("k_psvd_resid", ()): "tests/test_gpu_puresvd.py test_the_random_fit against tests/puresvd_ref.py residuals",
    ("k_psvd_export_f32", ()): "tests/test_gpu_puresvd.py test_fold_in_and_serving: the exported tables, byte for byte",
}


def placement_errors(kernels):
    """what is wrong with the placement of a manifest's kernels: [] or one line per kernel"""
    show = lambda k: "%s<%s>" % (k[0], ", ".join(map(str, k[1]))) if k[1] else k[0]
    placed = reached()
    bad = []
    for k in sorted(kernels):
        if k in placed and k in EXEMPT:
            bad.append("%s is both reached by %s and exempt" % (show(k), placed[k]))
        elif k not in placed and k not in EXEMPT:
            bad.append("%s (%s) is launched by no list of tests/list_paths.py and is not exempt" % (show(k), kernels[k]))
    for k in sorted(set(placed) | set(EXEMPT)):
        if k not in kernels:
            bad.append("%s is placed but is not in the manifest" % show(k))
    return bad


def test_every_kernel_of_the_list_families_is_placed():
    kernels = manifest_kernels()
    assert len(kernels) == 13 + 11 + 9 + 2 + 8, sorted(kernels)               # the counts of the five `==` headers
    bad = placement_errors(kernels)
    assert not bad, "\n".join(bad)
    assert all(len(reason) > 20 and "tests/test_gpu_" in reason for reason in EXEMPT.values())
    for name in set(reached().values()):
        assert LP.CASES[name]["how"] == "restatement", name


def test_a_made_up_kernel_and_a_missing_one_are_named(tmp_path):
    """the guard itself: a manifest with one kernel line more, and one with a line less, each fail and name the kernel"""
    text = open(MANIFEST).read()
    extra = tmp_path / "extra.txt"
    extra.write_text(text.replace("== userknn.hip:", "== userknn.hip:\nkernel _ZN12_GLOBAL__N_112k_uknn_scoreILi8ELi0EEEv13UknnScoreArgs vgpr=1", 1))
    bad = placement_errors(manifest_kernels(str(extra)))
    assert len(bad) == 1 and "k_uknn_score<8, 0> (userknn.hip) is launched by no list" in bad[0], bad
    fewer = tmp_path / "fewer.txt"
    fewer.write_text("".join(l for l in text.splitlines(True) if not (l.startswith("kernel ") and "k_knn_cooc_wILi512E" in l)))
    bad = placement_errors(manifest_kernels(str(fewer)))
    assert bad == ["k_knn_cooc_w<512> is placed but is not in the manifest"], bad


# ---- the GPU tests read the lists ------------------------------------------------------------------------------------------------
def _module(fname):
    return ast.parse(open(os.path.join(HERE, fname)).read())


def test_the_gpu_tests_take_their_values_from_these_lists():
    """a list only guards what runs at it"""
    for name, case in LP.CASES.items():
        assert hasattr(LP, name), name
        tree = _module(case["file"])
        funcs = {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
        assert case["test"] in funcs, "%s has no %s" % (case["file"], case["test"])
    assert {n for n in dir(LP) if n.isupper() and n != "CASES"} == set(LP.CASES), "a list of tests/list_paths.py without a case"
    reads = lambda fname, alias: {n.attr for n in ast.walk(_module(fname)) if isinstance(n, ast.Attribute)
                                  and isinstance(n.value, ast.Name) and n.value.id == alias}
    used = reads("test_gpu_list_paths.py", "LP")
    for name in ("KNN_SCORE_KS", "KNN_FIT_KS", "UKNN_LIST_KS", "CHUNKED_FAMILIES", "CHUNKED_KS", "CHUNKED_BY_BYTES"):
        assert name in used, "test_gpu_list_paths.py does not read list_paths.%s" % name
    assert {"PSVD_EIG_SIZES", "PSVD_WIDE_FIT"} <= reads("puresvd_cases.py", "LP")
    assert {"EIG_SIZES", "WIDE_FIT", "wide_case"} <= reads("test_gpu_puresvd.py", "PC")
    assert "\npytestmark = pytest.mark.gpu\n" in open(os.path.join(HERE, "test_gpu_list_paths.py")).read()
