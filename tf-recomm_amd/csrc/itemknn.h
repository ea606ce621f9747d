// itemknn.h - item-based nearest neighbours (tfr_knn_*): the launch plans, the argument blocks of the two kernels
// and the handle.  itemknn.hip owns the kernels and the C-ABI entries; the CSR, the serving drivers and the device pieces it
// shares with EASE are item_lists.h's; the per-slice key lists are merged by topk.hip's launch_topk_merge (topk.h).
//
// Fit (which = 0): one block per (item, catalogue slice of KNN_W_FIT columns) counts co-occurrences in uint32 LDS counters
// and keeps the slice's K best keys.  Scoring (which = 1): one wave per (query, slice of KNN_W_SCORE columns) sums the
// query's neighbour lists into a float32 LDS accumulator of its own, four waves per block.  Weighted fit (which = 2 of the
// internal plan, tfr_knn_weighted_plan outside): the fit's block over KNN_W_WFIT columns of uint64 sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tfrecomm.h"
#include "devbuf.h"
#include "topk.h"
#include "score_tile.h"
#include "item_lists.h"

constexpr int KNN_KMAX = tfr::TOPK_KMAX;
constexpr int KNN_WAVES = 4;                             // waves per block of both kernels
constexpr int KNN_W_FIT = 16384;                         // counters per fit block: 64 KiB
constexpr int KNN_W_SCORE = 8192;                        // accumulator slots per scoring wave: 32 KiB
constexpr int KNN_SCORE_CAP = 512;                       // keys per scoring wave's queue
constexpr int KNN_FIT_AHEAD = 64;                        // users whose row bounds a fit wave loads and searches at once
constexpr int KNN_SCORE_AHEAD = 4;                       // list items whose neighbour rows a scoring wave loads ahead
constexpr int64_t KNN_CHUNK_MAX = 65536;                 // rows per chunk
constexpr int KNN_GRID_ROWS = 8192;                      // fit grid: rows past this are taken in strides

// per-wave queue of the fit: the kept K plus one 64-lane append, a power of two for the bitonic sort
constexpr int knn_fit_cap(int K) { return K + 64 <= 256 ? 256 : 512; }
constexpr size_t knn_fit_lds(int cap) { return (size_t)KNN_W_FIT * 4 + (size_t)KNN_WAVES * cap * 8 + KNN_WAVES * 4; }
constexpr size_t knn_score_lds() { return (size_t)KNN_WAVES * KNN_W_SCORE * 4 + (size_t)KNN_WAVES * KNN_SCORE_CAP * 8; }
// 64-lane rounds that cover one neighbour row
constexpr int knn_rounds(int K) { return K <= 64 ? 1 : K <= 128 ? 2 : 4; }

// The weighted fit (tfr_knn_fit_weighted): k_knn_cooc's block with uint64 sums of per-user weights in place of
// the uint32 counts.  KNN_W_WFIT columns of 8 bytes are the same 64 KiB as KNN_W_FIT of 4, so the LDS sizes, and with
// them the blocks per CU, are those of the unweighted fit.
constexpr int KNN_W_WFIT = 8192;
constexpr size_t knn_wfit_lds(int cap) { return (size_t)KNN_W_WFIT * 8 + (size_t)KNN_WAVES * cap * 8 + KNN_WAVES * 4; }
static_assert(knn_wfit_lds(256) == knn_fit_lds(256) && 2 * knn_wfit_lds(256) <= 163840, "two weighted fit blocks per CU at CAP 256");

struct KnnPlan {
    int32_t width, slices, cap, ahead;
    int64_t chunk;                                       // rows (fit: items, scoring: queries) per chunk
    size_t lds;                                          // static LDS of the block
};

// which: 0 the fit, 1 the scoring, 2 the weighted fit (tfr_knn_plan takes 0 and 1; tfr_knn_weighted_plan is 2)
// false: k outside [1, 256], no items, or more slices than the merge takes (slices <= 256 and slices * k <= 8192 keys)
inline bool knn_plan(int which, int64_t n_items, int k, int64_t n_rows, KnnPlan* p) {
    if (k < 1 || k > KNN_KMAX || n_items < 1 || n_items > 0x7fffffffLL || n_rows < 0 || which < 0 || which > 2) return false;
    p->width = which == 1 ? KNN_W_SCORE : which == 2 ? KNN_W_WFIT : KNN_W_FIT;
    const int64_t s = (n_items + p->width - 1) / p->width;
    if (s > tfr::TOPK_MAX_SLICES || s * k > tfr::TOPK_MERGE_KEYS) return false;
    p->slices = (int32_t)s;
    p->cap = which == 1 ? KNN_SCORE_CAP : knn_fit_cap(k);
    p->ahead = which == 1 ? KNN_SCORE_AHEAD : KNN_FIT_AHEAD;
    p->lds = which == 1 ? knn_score_lds() : which == 2 ? knn_wfit_lds(p->cap) : knn_fit_lds(p->cap);
    int64_t chunk = n_rows < 1 ? 1 : n_rows > KNN_CHUNK_MAX ? KNN_CHUNK_MAX : n_rows;
    const int64_t by_part = tfr::TOPK_PART_BYTES / (s * k * 8);
    if (chunk > by_part) chunk = by_part;
    p->chunk = chunk < 1 ? 1 : chunk;
    return true;
}

enum { KNN_COSINE = 0, KNN_JACCARD = 1, KNN_COUNT = 2 };

// float64 with IEEE operations from the three integers, rounded once to float32 (userknn.hip forms its similarities with it too)
__device__ __forceinline__ float knn_sim(int metric, uint32_t c, int64_t ni, int64_t nj, double shrink) {
    double s;
    if (metric == KNN_COSINE) s = (double)c / (sqrt((double)ni * (double)nj) + shrink);
    else if (metric == KNN_JACCARD) s = (double)c / ((double)(ni + nj - (int64_t)c) + shrink);
    else s = (double)c;
    return __double2float_rn(s);
}

struct KnnFitArgs {
    const int64_t* pu; const int32_t* items;             // the user rows, each strictly increasing
    const int64_t* pi; const int32_t* iu;                // the item lists (users ascending)
    uint64_t* part;                                      // out [n_rows, slices, K] keys, descending, 0 past the kept ones
    int64_t row_lo, n_rows, n_items;
    double shrink;
    int32_t K, slices, metric;
};

// k_knn_cooc<cap> over a grid of (rows, slices), for a caller outside itemknn.hip.  Nothing in the kernel ties "item" to the
// catalogue: with pi / iu the user rows, pu / items the item lists and n_items the user count it counts the items two users
// share - UserKNN's fit (userknn.hip).  cap is knn_fit_cap(K).
void knn_launch_cooc(const KnnFitArgs& a, int cap, dim3 grid, hipStream_t s);

struct KnnWFitArgs {
    const int64_t* pu; const int32_t* items;             // the user rows, each strictly increasing
    const int64_t* pi; const int32_t* iu;                // the item lists (users ascending)
    const unsigned long long* uw;                        // [n_users] fixed-point user weights
    const double* row_scale; const double* col_scale;    // [n_items] each
    uint64_t* part;                                      // out [n_rows, slices, K] keys, descending, 0 past the kept ones
    int64_t row_lo, n_rows, n_items;
    double unit;                                         // 2^-shift
    int32_t K, slices;
};

struct KnnScoreArgs {
    const int32_t* users;                                // NULL: query q is row q of (ptr, ids); else row users[q]
    const int64_t* ptr; const int32_t* ids;              // the query lists, each strictly increasing
    const int32_t* nb_items; const float* nb_scores;     // [n_items, K] neighbour lists, -1 past the kept ones
    const int64_t* xptr; const int32_t* xids;            // exclusion rows aligned with the queries; xptr may be NULL
    const int64_t* tptr; const int32_t* tids;            // target rows aligned with the queries (ranking)
    uint64_t* part;                                      // top-K: out [n, slices, k] keys of queries q_lo .. q_lo + n
    uint64_t* tkeys; int32_t* ranks;                     // ranking: per target its key (0 = unranked) and its rank
    int64_t q_lo, n, n_items;
    int32_t K, k, slices;
};

struct tfr_knn : tfr::ItemListModel {
    int32_t K = 0, metric = 0;
    double shrink = 0.0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    tfr::DevBuf<int32_t> nb_items;                       // [n_items, K]
    tfr::DevBuf<float> nb_scores;
    int64_t max_item_users = 0;                          // the longest loaded item list: bounds the weighted fit's sums
    tfr::DevBuf<unsigned long long> uw;                  // the weighted fit's staged inputs
    tfr::DevBuf<double> row_scale, col_scale;
};
