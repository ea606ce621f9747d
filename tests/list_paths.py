"""The launch paths of the interaction-list models (csrc/item_lists.h: ItemKNN, RP3beta, EASE, SLIM, UserKNN, and PureSVD on
the same lists) the GPU tests run: neighbour-row widths K, serving chunks, eigen sizes.

Every scoring and fit kernel of the layer is templated on something K picks, every serving driver loops over query chunks,
and the PureSVD kernels branch on r (tests/test_list_path_coverage.py restates each rule, parses profiles/kernel_manifest.txt
and checks that the lists below reach every instantiation the library compiles).  Each list holds one value per class it
must reach, so that removing a value leaves a class untested and the guard names it.  Tests that ran at a hand-picked list
before keep that list; tests/test_gpu_list_paths.py runs these."""

# K of the neighbour lists the scoring kernels read, k_knn_score<R, MODE> and k_uknn_score<R, MODE>: both ends of each count
# of 64-lane rounds R = knn_rounds(K) (1 up to 64, 2 up to 128, 4 above), the row exactly full (K = 64 R, no lane masked by
# slot < K) and one slot into the next count.  recommend runs MODE 0 at each, rank_items MODE 1 and 2
KNN_SCORE_KS = (1, 64, 65, 128, 129, 256)
# K of the fits on the staircase, k_knn_cooc<CAP>, k_knn_cooc_w<CAP>: 192 is the tightest fit of the 256-key queue (K plus one
# 64-lane append is CAP exactly: queue_offer writes slot CAP - 1), 193 the smallest K on the 512-key queue
KNN_FIT_KS = (192, 193)
# K of UserKNN's neighbour search of query lists, k_uknn_query_cooc<CAP>: the same two edges
UKNN_LIST_KS = (192, 193)

# the eigen step, k_psvd_jacobi: r = 1, the first pair, the first odd r, two pairs per round, an odd width inside, both
# sides of the edge where the rotations leave LDS for global scratch (99 | 100), odd and even there, the widest odd r and
# the widest
PSVD_EIG_SIZES = (1, 2, 3, 4, 37, 99, 100, 101, 127, 128)
# (factors, oversample) of the wide PureSVD fit: r = 101 is odd with the rotations in global scratch, and k_psvd_spmm runs
# at r (odd) and at `factors` (even), as rows and as chunks of lists longer than PSVD_CHUNK
PSVD_WIDE_FIT = (8, 93)

# a second query chunk through every serving driver (tfr::topk_run behind topk and topk_lists, UknnServe::lists_prepare):
# (family, k).  n is plan(...)["chunk"] + 2 queries on a model of 7 users and 9 items
CHUNKED_FAMILIES = ("knn", "ease", "slim", "uknn")
CHUNKED_KS = (1, 10)
# and one case whose chunk is set by the 128 MiB of per-slice keys, not by the cap of 65536 rows: (family, items, k)
CHUNKED_BY_BYTES = ("ease", 1025, 256)

# How each list is held: the GPU test that runs it, and against what.  "restatement": the NumPy restatement of the operation
# (tests/*_ref.py), bit for bit unless the test's docstring states a bound.  Never "another handle".
CASES = {
    "KNN_SCORE_KS": dict(file="test_gpu_list_paths.py", test="test_every_scoring_round_and_mode_against_the_restatement", how="restatement"),
    "KNN_FIT_KS": dict(file="test_gpu_list_paths.py", test="test_fit_queue_edges_on_the_staircase", how="restatement"),
    "UKNN_LIST_KS": dict(file="test_gpu_list_paths.py", test="test_list_neighbours_queue_edges_on_the_transposed_staircase", how="restatement"),
    "CHUNKED_FAMILIES": dict(file="test_gpu_list_paths.py", test="test_a_second_query_chunk", how="restatement"),
    "CHUNKED_KS": dict(file="test_gpu_list_paths.py", test="test_a_second_query_chunk", how="restatement"),
    "CHUNKED_BY_BYTES": dict(file="test_gpu_list_paths.py", test="test_a_second_query_chunk_set_by_the_key_bytes", how="restatement"),
    "PSVD_EIG_SIZES": dict(file="test_gpu_puresvd.py", test="test_the_eigen_step", how="restatement"),
    "PSVD_WIDE_FIT": dict(file="test_gpu_puresvd.py", test="test_the_wide_fit_and_long_fold_ins", how="restatement"),
}
