// bf16_rank.hip - rank held-out items from the bf16 snapshot (tfr_bf16_rank_items).
//
// k_rank_targets_bf16 / k_rank_count_bf16: the blocks of rank_body.h (the ones k_rank_targets / k_rank_count run: pieces,
//   sorted target keys, excluded items taken off, bins) with Bf16RankScorer: the tile's dot on snapshot rows
//   (v_mfma_f32_32x32x16_bf16, score_tile.h mfma_tile_dot_bf16) plus the snapshot's mu, bu and bi in Bf16TopkScorer's order,
//   so a pair gets the bits tfr_bf16_topk ranks it by.  Snapshot rows are always 16-byte aligned, so there is no V4 argument.
// The finishing scan works on bins only and is rank.hip's (launch_rank_finish).
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "rank.h"
#include "rank_body.h"

namespace tfr {

// score(u, i) = ((dot + mu) + bu[u]) + bi[i]: A rows are the items', the B row the user's, both of the snapshot
struct Bf16RankScorer {
    const Bf16RankArgs& a;
    const uint16_t* brow;
    float mu, ub;
    __device__ __forceinline__ Bf16RankScorer(const Bf16RankArgs& a_, int32_t user)
        : a(a_), brow(a_.P + (int64_t)user * a_.DP), mu(*a_.mu), ub(a_.bu[user]) {}
    __device__ __forceinline__ f32x16 tile(int64_t row, int h) const {
        return mfma_tile_dot_bf16(a.Q + row * a.DP, brow, a.DP, a.item_abs, h);
    }
    __device__ __forceinline__ float score(float dot, int64_t item) const { return ((dot + mu) + ub) + a.bi[item]; }
};

__global__ __launch_bounds__(256) void k_rank_targets_bf16(Bf16RankArgs a) {
    warm_args(a);
    rank_targets_block<Bf16RankScorer>(a);
}

__global__ __launch_bounds__(256) void k_rank_count_bf16(Bf16RankArgs a) {
    warm_args(a);
    rank_count_block<Bf16RankScorer>(a);
}

void launch_bf16_rank(const Bf16RankArgs& a, const RankPlan& p, hipStream_t s) {
    if (a.n_pieces < 1) return;
    const unsigned per_wave = (unsigned)((a.n_pieces + RANK_WAVES - 1) / RANK_WAVES);
    hipLaunchKernelGGL(k_rank_targets_bf16, dim3(per_wave), dim3(256), 0, s, a);
    const dim3 g((unsigned)((a.n_pieces + p.ppb - 1) / p.ppb), (unsigned)p.slices);
    hipLaunchKernelGGL(k_rank_count_bf16, g, dim3(256), 0, s, a);
    launch_rank_finish(a, s);
}

}  // namespace tfr
