// slim.h - SLIM (tfr_slim_*): the launch plan, the argument block of the solver kernel and the handle.  slim.hip
// owns the solver and the C-ABI entries; the Gram kernel and the three scoring launches are ease.hip's (ease.h
// ease_launch_gram / ease_launch_score, the scoring block stays EaseScoreArgs); the CSR, the serving drivers and the scoring
// tail are item_lists.h's.
//
// Fit: A = X^T X + beta I in float64 (k_ease_gram with lambda = beta), its diagonal (k_slim_diag), then k_slim_cd: one
// workgroup per item column runs cyclic coordinate descent on the column's elastic-net problem with the gradient residual q
// in LDS, and stores the column's non-zero weights into the dense float32 W.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tfrecomm.h"
#include "devbuf.h"
#include "item_lists.h"
#include "ease.h"

constexpr int64_t SLIM_MAX_ITEMS = 16384;                // q of one column: 128 KiB of the 160 KiB one workgroup may declare
constexpr int SLIM_T = 256;                              // threads per workgroup = coordinates one window examines at once
constexpr int SLIM_WAVES = SLIM_T / 64;
constexpr int SLIM_AHEAD = 4;                            // entries of a Gram row a thread loads before it applies them
constexpr int SLIM_HEAD = 128;                           // LDS bytes before q: the waves' exchange slots (two parities) and the maxima
constexpr int SLIM_CUS = 256;                            // compute units the grid is sized for
constexpr int SLIM_BLOCKS_PER_CU = 8;                    // 8 workgroups of 4 waves fill a CU's 32 wave slots
constexpr int64_t SLIM_LDS_PER_CU = 163840;
static_assert(2 * SLIM_WAVES * 8 + 2 * SLIM_WAVES * 4 + SLIM_WAVES * 8 <= SLIM_HEAD && SLIM_HEAD % 16 == 0, "the head holds the slots");
static_assert(SLIM_MAX_ITEMS <= EASE_MAX_ITEMS, "the scoring plan is EASE's");

constexpr size_t slim_cd_lds(int64_t n_items) { return (size_t)SLIM_HEAD + (((size_t)n_items * 8 + 15) & ~(size_t)15); }
static_assert(slim_cd_lds(SLIM_MAX_ITEMS) <= (size_t)SLIM_LDS_PER_CU, "the cap must fit one workgroup");

struct SlimPlan {
    int32_t window, grid, w_in_lds;                      // T; workgroups of k_slim_cd; 0: w lives in a global scratch row per workgroup
    size_t lds;                                          // dynamic LDS of one k_slim_cd workgroup
    int64_t f64_bytes, f32_bytes;                        // A, its diagonal and the scratch rows; W
};

// false: what a launch would refuse
inline bool slim_plan(int64_t n_items, SlimPlan* p) {
    if (n_items < 1 || n_items > SLIM_MAX_ITEMS) return false;
    p->window = SLIM_T;
    p->w_in_lds = 0;
    p->lds = slim_cd_lds(n_items);
    int64_t per_cu = SLIM_LDS_PER_CU / (int64_t)p->lds;
    per_cu = per_cu < 1 ? 1 : per_cu > SLIM_BLOCKS_PER_CU ? SLIM_BLOCKS_PER_CU : per_cu;
    const int64_t grid = per_cu * SLIM_CUS;
    p->grid = (int32_t)(n_items < grid ? n_items : grid);
    p->f64_bytes = (n_items * n_items + n_items + (int64_t)p->grid * n_items) * 8;
    p->f32_bytes = n_items * n_items * 4;
    return true;
}

struct SlimCdArgs {
    const double* A; const double* diag;                 // [n, n] symmetric: column j is row j; [n]
    double* w;                                           // scratch [grid, n]: the weights of the column a workgroup is solving
    float* W;                                            // out [n, n], zeroed before the launch: only non-zero weights are stored
    int32_t* sweeps; int32_t* updates; int32_t* converged;   // out [n] each
    int32_t* err;                                        // 0, or 1 + a column whose weights left the finite range
    int64_t n;
    double l1, tol;
    int32_t positive, max_iter;
};

struct tfr_slim : tfr::ItemListModel {
    double beta = 0.0;
    bool has_gram = false;                               // A and diag hold a Gram matrix (gram / set_gram; a solve keeps it)
    bool solved = false;                                 // W and the statistics are those of one tfr_slim_solve
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float gram_ms = 0.f;                                 // device time of the tfr_slim_gram that built A (0: a caller's)
    tfr::DevBuf<double> A, diag, w;                      // [n, n], [n], [grid, n]
    tfr::DevBuf<float> W;                                // [n, n]
    tfr::DevBuf<int32_t> sweeps, updates, converged;     // [n] each, of the last solve
    tfr::DevBuf<int32_t> err;
};
