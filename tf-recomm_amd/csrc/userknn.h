// userknn.h - user-based nearest neighbours (tfr_uknn_*): the launch plan, the argument blocks of the two kernels
// and the handle.  userknn.hip owns the kernels and the C-ABI entries.  The CSR in both orientations, the serving drivers, the
// count loop, the key queue and the scoring tail are item_lists.h's; the fit is itemknn.hip's k_knn_cooc with the roles of
// users and items swapped (itemknn.h knn_launch_cooc), and the similarity is its knn_sim.
//
// Fit (which = 0): k_knn_cooc over (user, slice of KNN_W_FIT user columns).  Scoring (which = 1): one wave per (query, slice
// of KNN_W_SCORE item columns) adds the query's neighbours' item lists, in slot order, into a float32 LDS accumulator of its
// own.  Neighbour search of query lists (which = 2): the fit's block per (query list, slice of KNN_W_FIT user columns).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tfrecomm.h"
#include "devbuf.h"
#include "item_lists.h"
#include "itemknn.h"

constexpr int UKNN_SCORE_AHEAD = 64;                     // neighbour slots whose rows a scoring wave searches side by side

// which: 0 the fit, 1 the scoring, 2 the neighbour search of query lists; n_cols: the users (0, 2) or the items (1).
// The shapes are ItemKNN's fit and scoring blocks, so are the limits: false as knn_plan.
inline bool uknn_plan(int which, int64_t n_cols, int k, int64_t n_rows, KnnPlan* p) {
    if (which < 0 || which > 2) return false;
    if (!knn_plan(which == 1 ? 1 : 0, n_cols, k, n_rows, p)) return false;
    if (which == 1) p->ahead = UKNN_SCORE_AHEAD;
    return true;
}

struct UknnScoreArgs {
    const int32_t* users;                                // NULL: query q reads row q of the neighbour lists; else row users[q]
    const int64_t* ptr; const int32_t* ids;              // the query lists (what the serving drivers set; the kernel reads neither)
    const int32_t* nb_users; const float* nb_scores;     // [rows, K] neighbour lists, -1 in a slot that holds nobody
    const int64_t* pu; const int32_t* items;             // the resident user rows, each strictly increasing
    const int64_t* xptr; const int32_t* xids;            // exclusion rows aligned with the queries; xptr may be NULL
    const int64_t* tptr; const int32_t* tids;            // target rows aligned with the queries (ranking)
    uint64_t* part;                                      // top-K: out [n, slices, k] keys of queries q_lo .. q_lo + n
    uint64_t* tkeys; int32_t* ranks;                     // ranking: per target its key (0 = unranked) and its rank
    int64_t q_lo, n, n_items;
    int32_t K, k, slices;
};

// The fields count_row reads carry its names: it walks the "users" iu[p0, p1) of a row and, for each, the part of row
// pu / items inside the slice.  Here the row is a query list, its entries are items, and their rows are the item lists.
struct UknnQueryArgs {
    const int64_t* qptr; const int32_t* iu;              // the query lists: bounds and item ids
    const int64_t* pu; const int32_t* items;             // the model's item lists (users ascending): its pi and iu
    const int64_t* deg;                                  // the model's user row bounds: d_v = deg[v + 1] - deg[v]
    uint64_t* part;                                      // out [n_rows, slices, K] keys, descending, 0 past the kept ones
    int64_t row_lo, n_rows, n_users;
    double shrink;
    int32_t K, slices, metric;
};

struct tfr_uknn : tfr::ItemListModel {
    int32_t K = 0, metric = 0;
    double shrink = 0.0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    tfr::DevBuf<int32_t> nb_users;                       // [n_users, K]
    tfr::DevBuf<float> nb_scores;
    tfr::DevBuf<int32_t> q_nb_users;                     // [n, K]: the neighbours of one call's query lists
    tfr::DevBuf<float> q_nb_scores;
    bool serving_lists = false;                          // inside tfr_uknn_topk_lists: the scoring reads q_nb_*, row q
};
