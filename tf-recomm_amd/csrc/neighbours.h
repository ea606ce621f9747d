// neighbours.h - nearest neighbours in factor space (tfr_neighbours*): the argument block and launchers shared by
// neighbours.hip and api.hip; the launch plan is topk.h's.
//
// One table T [R, D] gives the query rows and the candidate rows.  dot(a, b) = the f32 fmaf chain over f = 0..D-1 ascending
// from +0 of T[a,f] * T[b,f] (the chain of topk.h, no bias terms); cosine(a, b) = (dot(a, b) * rn[a]) * rn[b] with
// rn[r] = 1 / sqrtf(ss[r]), ss[r] the same chain of T[r,f]^2, and rn = 0 where ss == 0.  Keys, queues, slices and the merge are
// those of topk.h; the ids in the keys are row ids of T, whatever the candidate range.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "topk.h"

namespace tfr {

constexpr int NB_RNORM_ROWS = 256;                     // rows per k_row_rnorm block: one lane per row, 64 rows per wave

// The scoring block is the top-K block (score_tile.h sliced_topk_block) with the query rows in the users' place and the
// candidate range in the items': TopkPlan / topk_plan give its queue capacity, rows per block, slices, chunking and LDS sizes.
struct NbArgs : SlicedArgs {
    const float* T;                                    // [R, D] query and candidate rows; excl holds row ids of T, sorted
    const float* rn;                                   // [R] inverse norms: cosine; NULL: dot
    int64_t R, lo, hi;                                 // candidates are rows [lo, hi)
};

void launch_nb_score(const NbArgs& a, const TopkPlan& p, hipStream_t s);
// rn[r] for r in [0, R): |T| and T have the same squares, so item_abs does not enter
void launch_row_rnorm(const float* T, int64_t R, int32_t D, float* rn, hipStream_t s);

}  // namespace tfr
