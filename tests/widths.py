"""The row widths D the GPU tests run each kernel family at.

Every kernel is templated on something D picks (see tests/test_width_coverage.py, which restates each dispatch rule and
checks that each list below reaches every instantiation a supported D can reach).  Each list holds one width per
instantiation it must reach, so that removing a width leaves an instantiation untested and the guard names it.  Tests
that ran at a hand-picked list before keep that list and add these."""

# SVD forward and step, FM forward and training: geometry(D) -> (G, VEC), ten pairs
SVD_SMALL = (2, 5, 15, 16, 25, 28, 61, 64, 128, 200)       # small tables: k_tile_step
SVD_BIG = (3, 7, 9, 12, 31, 32, 33, 36, 100, 252)          # a side above CSORT_MAX_BINS rows: radix sort, k_seg_reduce, ...
FM = (2, 6, 13, 8, 25, 28, 61, 44, 100, 200)

# the row-sharded step's stages (tests/test_gpu_shard_stages.py): (G, VEC) crossed with full width D == G * VEC, which picks
# k_gather_packed's unguarded non-temporal loads and the reduce's three-round load form.  A VEC = 1 row is never full width
# (D == G would be a multiple of four), so there are fifteen classes
SHARD = (12, 16, 28, 32, 36, 64, 100, 128, 252, 256, 3, 7, 13, 31, 61)
# the data-parallel stages (tests/test_gpu_dp_stages.py), on the tile path and on the sort path: one width per (G, VEC)
DP = (8, 24, 48, 96, 200, 2, 6, 11, 25, 50)
# the FM step per row (tests/test_gpu_fm_step.py) and the FM forward's load forms: the same fifteen classes - k_fm_forward
# takes unguarded loads at full width, and the FM backward the reduce's three-round load form
FM_STEP = (12, 16, 28, 32, 36, 64, 100, 128, 252, 256, 3, 7, 13, 31, 61)
# the forward's non-temporal user-row loads (tests/test_gpu_forward_paths.py): k_forward<G, VEC, MODE, 4, true> on a user
# table above 256 MB, the same fifteen classes - load_frag<VEC, true> has lanes with d0 >= D at partial width only.
# k_forward_bf16<G, MODE, UNR, true>: the lanes per rating of the snapshot crossed with a group wider than the row
# (G * 8 > DP), whose spare lanes take the redirected load
FORWARD_PNT = (12, 16, 28, 32, 36, 64, 100, 128, 252, 256, 3, 7, 13, 31, 61)
BF16_PNT = (5, 13, 17, 31, 33, 61, 100, 128, 132, 256)

# SVD++ kernels and batched fine-tuning: NJ = ceil(D / 64) registers per lane, the last one full or partial
SVDPP = (33, 64, 100, 128, 132, 192, 252, 256)
FINETUNE = (20, 64, 68, 128, 132, 192, 252, 256)
BPR = (1, 33, 64, 100, 128, 132, 192, 252, 256)            # k_bpr_users / k_bpr_items (csrc/wave_rows.h with_nj, over csrc/dispatch.h with_one_of), and D = 1
FINETUNE_STREAMED = (20, 100, 132, 252)                    # one call stages some users and streams others, each NJ

# top-K and rank: V4 = (D % 4 == 0) crossed with where mfma_tile_dot's last group of four float4s ends
TOPK = (4, 5, 27, 33, 38, 63, 68, 104, 128, 252)
TOPK_KS = (1, 10, 100, 256)                                # both queue sizes (k + TOPK_ROUND <= 256, and above)
RANK = (3, 8, 17, 20, 28, 31, 32, 43, 54, 200)
RANK_RANDOM = (43, 200)                                    # rank == position in recommend, on random tables
FM_TOPK = (25, 200)                                        # FM get_ranking / rank_items: a V1 width, a width above 128

# ALS: one-wave Cholesky, lane r owns row r, 1 <= d <= ALS_MAXD
ALS = (1, 32)
ALS_CHUNKED = (32,)
# the ALS half-sweep per entity (tests/test_gpu_als_step.py): both ends of each count of live A-entry slots ceil(d*d / 256)
# (the last slot exactly full at d = 16 and d = 32), and both sides of the one-pass LDS staging of a 32-rating tile (d <= 8)
ALS_STEP = (1, 8, 9, 16, 17, 22, 23, 27, 28, 32)
