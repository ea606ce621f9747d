// bf16_topk.hip - top-K recommendation from the bf16 snapshot (tfr_bf16_topk*).
//
// k_topk_score_bf16: the scoring block of score_tile.h (sliced_topk_block, the one k_topk_score runs: queues, thresholds,
//   exclusions, part[row, slice] out) with Bf16TopkScorer: the tile's dot on snapshot rows (v_mfma_f32_32x32x16_bf16, 16
//   features per instruction, ascending from a zero accumulator) plus the snapshot's mu, bu and bi in TopkScorer's order.
// Snapshot rows are always 16-byte aligned, so there is no V4 argument: two instantiations, one per queue size.  The merge
// and the exclusion check are topk.hip's, which work on keys and ids only.
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "topk.h"

namespace tfr {

// score(u, i) = ((dot + mu) + bu[u]) + bi[i]: A rows are the items', the B row the user's, both of the snapshot
struct Bf16TopkScorer {
    const Bf16TopkArgs& a;
    const uint16_t* brow;
    float mu, ub;
    __device__ __forceinline__ Bf16TopkScorer(const Bf16TopkArgs& a_, int32_t user)
        : a(a_), brow(a_.P + (int64_t)(user < 0 ? 0 : user) * a_.DP), mu(*a_.mu), ub(user >= 0 ? a_.bu[user] : 0.f) {}
    template <bool>
    __device__ __forceinline__ f32x16 tile(int64_t item, int h) const {
        return mfma_tile_dot_bf16(a.Q + item * a.DP, brow, a.DP, a.item_abs, h);
    }
    __device__ __forceinline__ bool eligible(int64_t) const { return true; }
    __device__ __forceinline__ float score(float dot, int64_t item) const { return ((dot + mu) + ub) + a.bi[item]; }
};

template <int UPB, int CAP>
__global__ __launch_bounds__(256) void k_topk_score_bf16(Bf16TopkArgs a) {
    warm_args(a);
    sliced_topk_block<UPB, CAP, true, Bf16TopkScorer>(a, a.U, 0, a.n_items);
}

void launch_bf16_topk_score(const Bf16TopkArgs& a, const TopkPlan& p, hipStream_t s) {
    const dim3 g((unsigned)((a.n_rows + p.upb - 1) / p.upb), (unsigned)p.slices);
    void (*const kern)(Bf16TopkArgs) = p.cap == 256 ? k_topk_score_bf16<32, 256> : k_topk_score_bf16<16, 512>;
    hipLaunchKernelGGL(kern, g, dim3(256), 0, s, a);
}

}  // namespace tfr
