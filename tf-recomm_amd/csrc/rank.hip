// rank.hip - rank held-out items over the whole catalogue on gfx950.
//
// Every key is scored by the MFMA tile of topk.hip (score_tile.h), so a target, an excluded item and a counted item get the
// same bits for the same pair, and the same bits tfr_topk ranks by.
// k_rank_targets: one wave per piece.  Scores the piece's targets, marks a NaN or excluded target unranked (key 0), sorts
//   the keys descending (bitonic, LDS), records the position of each sorted key's target, and starts the piece's bins at
//   minus the excluded items: every distinct excluded item with a non-NaN score is binned as k_rank_count bins it, and taken
//   off.  Writes -1 to the piece's ranks (the unranked stay so).
// k_rank_count: a block owns 32 pieces (the B columns of v_mfma_f32_32x32x2_f32) and one item slice.  A pair whose key
//   beats the piece's lowest ranked target adds 1 to bin p = #{targets with key >= it} (binary search of the sorted keys in
//   LDS, LDS integer atomic).  The block adds its bins to the piece's with global integer atomics.
// k_rank_finish: one wave per piece: rank of sorted target j = bins[0] + ... + bins[j], scattered to the target's position.
// The bodies of the first two live in rank_body.h, generic over a scorer; here they run with RankScorer on the float32 tables,
// in bf16_rank.hip on the bf16 snapshot.  k_rank_finish reads bins only and serves both (launch_rank_finish).
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "rank.h"
#include "rank_body.h"

namespace tfr {

// score(u, i) = ((dot + mu) + bu[u]) + bi[i] on the float32 tables: the scorer of rank_body.h's blocks
template <bool V4>
struct RankScorer {
    const RankArgs& a;
    const float* prow;
    float mu, ub;
    __device__ __forceinline__ RankScorer(const RankArgs& a_, int32_t user)
        : a(a_), prow(a_.P + (int64_t)user * a_.D), mu(*a_.mu), ub(a_.bu[user]) {}
    __device__ __forceinline__ f32x16 tile(int64_t row, int h) const {
        return mfma_tile_dot<V4>(a.Q + row * a.D, prow, a.D, a.item_abs, h);
    }
    __device__ __forceinline__ float score(float dot, int64_t item) const { return ((dot + mu) + ub) + a.bi[item]; }
};

template <bool V4>
__global__ __launch_bounds__(256) void k_rank_targets(RankArgs a) {
    warm_args(a);
    rank_targets_block<RankScorer<V4>>(a);
}

template <bool V4>
__global__ __launch_bounds__(256) void k_rank_count(RankArgs a) {
    warm_args(a);
    rank_count_block<RankScorer<V4>>(a);
}

__global__ __launch_bounds__(256) void k_rank_finish(RankCommon a) {
    static_assert(RANK_CAP == 128, "a lane scans two bins");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pc = (int64_t)blockIdx.x * RANK_WAVES + wave;
    if (pc >= a.n_pieces) return;
    const int nr = a.nr[pc];
    const int32_t* b = a.bins + pc * RANK_CAP;
    const int j0 = 2 * lane, j1 = 2 * lane + 1;
    const int32_t v0 = j0 < nr ? b[j0] : 0, v1 = j1 < nr ? b[j1] : 0;
    int32_t s = v0 + v1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t o = __shfl_up(s, off);
        if (lane >= off) s += o;
    }
    const int32_t r0 = s - v1, r1 = s;                 // inclusive sums through bins j0 and j1
    const int32_t* go = a.order + pc * RANK_CAP;
    int32_t* out = a.ranks + a.pieces[pc].tlo;
    if (j0 < nr) out[go[j0]] = r0;
    if (j1 < nr) out[go[j1]] = r1;
}

template <bool V4>
static void launch_rank_v(const RankArgs& a, const RankPlan& p, hipStream_t s) {
    const unsigned per_wave = (unsigned)((a.n_pieces + RANK_WAVES - 1) / RANK_WAVES);
    hipLaunchKernelGGL((k_rank_targets<V4>), dim3(per_wave), dim3(256), 0, s, a);
    const dim3 g((unsigned)((a.n_pieces + p.ppb - 1) / p.ppb), (unsigned)p.slices);
    hipLaunchKernelGGL((k_rank_count<V4>), g, dim3(256), 0, s, a);
    launch_rank_finish(a, s);
}

void launch_rank_finish(const RankCommon& a, hipStream_t s) {
    const unsigned per_wave = (unsigned)((a.n_pieces + RANK_WAVES - 1) / RANK_WAVES);
    hipLaunchKernelGGL(k_rank_finish, dim3(per_wave), dim3(256), 0, s, a);
}

void launch_rank(const RankArgs& a, const RankPlan& p, hipStream_t s) {
    if (a.n_pieces < 1) return;
    if ((a.D & 3) == 0) launch_rank_v<true>(a, p, s);
    else launch_rank_v<false>(a, p, s);
}

}  // namespace tfr
