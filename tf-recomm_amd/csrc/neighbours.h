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

// The same on one table of the bf16 snapshot (bf16_rows.h; bf16_neighbours.hip): T holds snapshot rows at a
// stride of DP elements.  dot(a, b) = the f32 sum of the exact products of the bf16 elements, 16 features per
// v_mfma_f32_32x32x16_bf16, ascending from +0 (score_tile.h mfma_tile_dot_bf16; item_abs clears the sign bits of both
// operands); ss[r] = the f32 fmaf chain over f ascending from +0 of the widened elements squared (the squares are exact, pads
// add nothing), rn[r] = 1 / sqrtf(ss[r]), 0 where ss == 0; cosine(a, b) = (dot(a, b) * rn[a]) * rn[b].
struct Bf16NbArgs : SlicedArgs {
    const uint16_t* T;                                 // [R, DP] query and candidate rows; excl holds row ids of T, sorted
    const float* rn;                                   // [R] inverse norms: cosine; NULL: dot
    int64_t R, lo, hi;                                 // candidates are rows [lo, hi)
    int32_t DP;
};

void launch_bf16_nb_score(const Bf16NbArgs& a, const TopkPlan& p, hipStream_t s);
void launch_row_rnorm_bf16(const uint16_t* T, int64_t R, int32_t DP, float* rn, hipStream_t s);

}  // namespace tfr
