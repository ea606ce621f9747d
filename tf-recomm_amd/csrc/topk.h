// topk.h - top-K recommendation (tfr_topk*): launch plan, argument blocks and launchers shared by topk.hip and api.hip; the
// plan and the common argument block also serve neighbours.h, whose scoring block is the same one (score_tile.h).
//
// score(u, i) = ((dot + mu) + bu[u]) + bi[i], dot = f32 fmaf chain over f = 0..D-1 ascending from +0 of P[u,f] * Q'[i,f]
// (Q' = |Q| with item_abs).  Keys: (order-preserving uint32 of the score) << 32 | ~item, so one 64-bit compare orders by score
// descending, then item ascending; key 0 is below every real key and marks an empty slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

constexpr int TOPK_KMAX = 256;
constexpr int TOPK_WAVES = 4;                          // waves per scoring block
constexpr int TOPK_SUB = 32;                           // items per wave and round: the A block of one 32x32x2 MFMA
constexpr int TOPK_ROUND = TOPK_WAVES * TOPK_SUB;      // items per block and round = most one user's queue grows per round
constexpr int TOPK_MAX_SLICES = 256;
constexpr int64_t TOPK_MERGE_KEYS = 8192;              // slices * k of one row, held in the merge block's LDS
constexpr int64_t TOPK_CHUNK_MAX = 65536;              // users per chunk
constexpr int64_t TOPK_PART_BYTES = (int64_t)128 << 20;  // per-chunk (row, slice) key lists
constexpr int64_t TOPK_TARGET_BLOCKS = 1024;           // scoring blocks a chunk should fill (256 CUs, two blocks each, twice)

// per-user queue: the kept top k plus room for one round of appends, a power of two for the bitonic sort
constexpr int topk_cap(int k) { return k + TOPK_ROUND <= 256 ? 256 : 512; }
// users per scoring block: 32 = the B block of the MFMA; 16 (columns 16..31 repeat 0..15) keeps the queues at 64 KB for k > 128
constexpr int topk_upb(int k) { return topk_cap(k) == 256 ? 32 : 16; }
constexpr size_t topk_score_static_lds(int upb, int cap) {
    return (size_t)upb * cap * 8 /* queues */ + (size_t)upb * 8 /* thresholds */ + (size_t)upb * 4 /* counts */;
}
constexpr size_t topk_merge_lds(int slices, int k) { return (size_t)slices * k * 8; }

struct TopkPlan {
    int32_t upb, cap, slices;
    int64_t chunk;                                     // users per chunk (multiple of upb)
    size_t lds_score, lds_merge;                       // static LDS of the scoring block, dynamic LDS of the merge block
};

inline int64_t topk_slices_for(int64_t chunk, int upb, int k, int64_t items) {
    int64_t smax = TOPK_MERGE_KEYS / k;
    if (smax > TOPK_MAX_SLICES) smax = TOPK_MAX_SLICES;
    const int64_t by_items = (items + TOPK_ROUND - 1) / TOPK_ROUND;
    if (smax > by_items) smax = by_items;
    if (smax < 1) smax = 1;
    const int64_t tiles = (chunk + upb - 1) / upb;
    int64_t s = (TOPK_TARGET_BLOCKS + tiles - 1) / tiles;
    return s < 1 ? 1 : s > smax ? smax : s;
}

// false: k outside [1, 256] or items < 1 (the dim is checked by the caller)
inline bool topk_plan(int k, int64_t n_users, int64_t items, TopkPlan* p) {
    if (k < 1 || k > TOPK_KMAX || items < 1 || n_users < 0) return false;
    p->cap = topk_cap(k);
    p->upb = topk_upb(k);
    int64_t chunk = n_users < 1 ? 1 : n_users > TOPK_CHUNK_MAX ? TOPK_CHUNK_MAX : n_users;
    chunk = (chunk + p->upb - 1) / p->upb * p->upb;
    int64_t s = topk_slices_for(chunk, p->upb, k, items);
    while (chunk > p->upb && chunk * s * k * 8 > TOPK_PART_BYTES) {
        chunk = (chunk / 2 + p->upb - 1) / p->upb * p->upb;
        s = topk_slices_for(chunk, p->upb, k, items);
    }
    p->chunk = chunk;
    p->slices = (int32_t)s;
    p->lds_score = topk_score_static_lds(p->upb, p->cap);
    p->lds_merge = topk_merge_lds(p->slices, k);
    return true;
}

// what every scoring block (score_tile.h sliced_topk_block) is told, whatever it scores: filled once, by api.hip's driver
struct SlicedArgs {
    const int32_t* rows;                               // [n_rows] this chunk's query ids: users, or rows of the one table
    const int64_t* indptr; const int32_t* excl;        // exclusion CSR rows of this chunk (absolute offsets into excl), may be NULL
    const int32_t* excl_bad;                           // nonzero: the exclusion CSR failed its check, it is not read
    uint64_t* part;                                    // out [n_rows, slices, k] keys, descending
    int32_t* err;
    int64_t n_rows;
    int32_t D, k, slices, item_abs;
};

struct TopkArgs : SlicedArgs {
    const float* P; const float* bu;                   // user rows [U, D] and biases
    const float* Q; const float* bi;                   // item rows [n_items, D] and biases (already offset to the item range)
    const float* mu;
    int64_t U, n_items;
};

// the same scores from the bf16 snapshot (bf16_rows.h): P and Q are snapshot rows at a stride of DP elements, the biases and
// mu the snapshot's float32 copies of the same moment.  dot = the f32 sum of the exact products of the bf16 elements, 16
// features per v_mfma_f32_32x32x16_bf16, ascending from +0 (score_tile.h mfma_tile_dot_bf16).
struct Bf16TopkArgs : SlicedArgs {
    const uint16_t* P; const float* bu;
    const uint16_t* Q; const float* bi;
    const float* mu;
    int64_t U, n_items;
    int32_t DP;
};

struct TopkMergeArgs {
    const uint64_t* part;
    int32_t* items_out; float* scores_out;             // [n_rows, k]; scores may be NULL
    int64_t n_rows;
    int32_t k, slices;
};

void launch_topk_score(const TopkArgs& a, const TopkPlan& p, hipStream_t s);
void launch_bf16_topk_score(const Bf16TopkArgs& a, const TopkPlan& p, hipStream_t s);   // bf16_topk.hip
void launch_topk_merge(const TopkMergeArgs& a, hipStream_t s);
// the device entry's exclusion check: ids in [0, n_items) (else err |= 1) and rows non-decreasing (else err |= 16);
// either sets *bad, which makes the scoring kernel ignore the exclusions
void launch_topk_check_excl(const int64_t* indptr, const int32_t* excl, int64_t n_rows, int64_t n_items, int32_t* bad,
                            int32_t* err, hipStream_t s);

}  // namespace tfr
