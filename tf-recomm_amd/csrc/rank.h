// rank.h - ranking of held-out items over the whole catalogue (tfr_rank_items*): launch plan, argument block and launcher
// shared by rank.hip, bf16_rank.hip and api.hip.
//
// rank(t) = #{eligible items i with a non-NaN score and key(u, i) > key(u, t)}, keys as in topk.h.  A row's targets are cut
// into pieces of at most RANK_CAP; a piece is (user, targets, exclusions) and ranks independently of every other piece.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

constexpr int RANK_CAP = 128;                          // targets per piece: two per lane of the finishing scan
constexpr int RANK_PPB = 32;                           // pieces per counting block: the B block (columns) of the MFMA
constexpr int RANK_WAVES = 4;                          // waves per block (every kernel)
constexpr int RANK_SUB = 32;                           // items per wave and round: the A block of one 32x32x2 MFMA
constexpr int RANK_ROUND = RANK_WAVES * RANK_SUB;      // items per counting block and round
constexpr int RANK_MAX_SLICES = 1024;
constexpr int64_t RANK_CHUNK_MAX = 32768;              // pieces per chunk
constexpr int64_t RANK_TARGET_BLOCKS = 1536;           // counting blocks a chunk should fill (256 CUs, three blocks each, twice)
constexpr int64_t RANK_LDS_PER_CU = 160 * 1024;

constexpr size_t rank_targets_static_lds() {
    return (size_t)RANK_WAVES * (RANK_CAP * 8 /* keys */ + RANK_CAP * 4 /* bins */ + RANK_SUB * 4 /* scores */);
}
constexpr size_t rank_count_static_lds() {
    return (size_t)RANK_PPB * RANK_CAP * 8 /* sorted target keys */ + (size_t)RANK_PPB * RANK_CAP * 4 /* bins */;
}
static_assert(RANK_LDS_PER_CU / rank_count_static_lds() >= 3, "the counting block should leave room for three per CU");

// pieces of a request, at most: each row with targets gives ceil(n_t / RANK_CAP)
inline int64_t rank_pieces_bound(int64_t n_users, int64_t n_targets) {
    const int64_t b = n_users + n_targets / RANK_CAP;
    return n_targets < b ? n_targets : b;
}

struct RankPlan {
    int32_t ppb, cap, slices;
    int64_t chunk;                                     // pieces per chunk (multiple of ppb)
    size_t lds_targets, lds_count;                     // static LDS of the target and the counting block
};

inline bool rank_plan(int64_t n_pieces, int64_t items, RankPlan* p) {
    if (n_pieces < 0 || items < 1) return false;
    p->ppb = RANK_PPB;
    p->cap = RANK_CAP;
    int64_t chunk = n_pieces < 1 ? 1 : n_pieces > RANK_CHUNK_MAX ? RANK_CHUNK_MAX : n_pieces;
    chunk = (chunk + RANK_PPB - 1) / RANK_PPB * RANK_PPB;
    p->chunk = chunk;
    int64_t smax = (items + RANK_ROUND - 1) / RANK_ROUND;
    if (smax > RANK_MAX_SLICES) smax = RANK_MAX_SLICES;
    const int64_t tiles = chunk / RANK_PPB;
    int64_t s = (RANK_TARGET_BLOCKS + tiles - 1) / tiles;
    p->slices = (int32_t)(s < 1 ? 1 : s > smax ? smax : s);
    p->lds_targets = rank_targets_static_lds();
    p->lds_count = rank_count_static_lds();
    return true;
}

// one piece of a chunk; offsets index the chunk's staged target / exclusion items
struct RankPiece {
    int64_t tlo;                                       // targets tgt[tlo, tlo + nt): sorted, distinct
    int64_t xlo, xhi;                                  // exclusions excl[xlo, xhi): non-decreasing
    int32_t user, nt;
};

// what the three kernels are told whichever rows they score: filled once per chunk, by api.hip's rank_host
struct RankCommon {
    const RankPiece* pieces;                           // [n_pieces]
    const int32_t* tgt; const int32_t* excl;
    uint64_t* keys;                                    // [n_pieces, RANK_CAP] the piece's target keys, descending, 0 = unranked
    int32_t* order;                                    // [n_pieces, RANK_CAP] position in the piece of the target of each key
    int32_t* nr;                                       // [n_pieces] ranked targets
    int32_t* bins;                                     // [n_pieces, RANK_CAP] items whose key beats exactly p targets' keys
    int32_t* ranks;                                    // out, aligned with tgt
    int64_t n_pieces, n_items;
    int32_t D, slices, item_abs;
};

struct RankArgs : RankCommon {
    const float* P; const float* bu;                   // user rows [U, D] and biases
    const float* Q; const float* bi;                   // item rows [n_items, D] and biases (already offset to the item range)
    const float* mu;
};

// the same ranks from the bf16 snapshot (bf16_rows.h): P and Q are snapshot rows at a stride of DP elements, the biases and
// mu the snapshot's float32 copies; keys are those of Bf16TopkArgs (topk.h), so rank < K is the position in tfr_bf16_topk
struct Bf16RankArgs : RankCommon {
    const uint16_t* P; const float* bu;
    const uint16_t* Q; const float* bi;
    const float* mu;
    int32_t DP;
};

// k_rank_targets -> k_rank_count -> k_rank_finish on stream s
void launch_rank(const RankArgs& a, const RankPlan& p, hipStream_t s);
void launch_bf16_rank(const Bf16RankArgs& a, const RankPlan& p, hipStream_t s);     // bf16_rank.hip
// the last of the three, which reads bins and writes ranks only: one kernel for both (rank.hip)
void launch_rank_finish(const RankCommon& a, hipStream_t s);

}  // namespace tfr
