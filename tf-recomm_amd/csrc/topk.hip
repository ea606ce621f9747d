// topk.hip - top-K recommendation on gfx950 (forward.py:47-61 get_ranking, als3.py:110-113 predict-then-rank).
//
// k_topk_score: the scoring block of score_tile.h (sliced_topk_block: a tile of users against a slice of the items, per-user
//   LDS queues, part[row, slice] out) with TopkScorer: the tile's dot (v_mfma_f32_32x32x2_f32, k ascending from a zero
//   accumulator, bit for bit the fmaf chain of the contract) plus mu, bu and bi in that order.
// k_topk_merge: one wave per row merges the slices' sorted lists (tournament over the list heads in LDS) into the output.
// k_topk_check_excl: the device entry's range / order check of the exclusion CSR.
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "topk.h"

namespace tfr {

// score(u, i) = ((dot + mu) + bu[u]) + bi[i]: A rows are the items', the B row the user's
struct TopkScorer {
    static constexpr bool ABS_B = false;
    const TopkArgs& a;
    const float* brow;
    float mu, ub;
    __device__ __forceinline__ TopkScorer(const TopkArgs& a_, int32_t user)
        : a(a_), brow(a_.P + (int64_t)(user < 0 ? 0 : user) * a_.D), mu(*a_.mu), ub(user >= 0 ? a_.bu[user] : 0.f) {}
    __device__ __forceinline__ const float* arow(int64_t item) const { return a.Q + item * a.D; }
    template <bool V4>
    __device__ __forceinline__ f32x16 tile(int64_t item, int h) const {
        return mfma_tile_dot<V4, ABS_B>(arow(item), brow, a.D, a.item_abs, h);
    }
    __device__ __forceinline__ bool eligible(int64_t) const { return true; }
    __device__ __forceinline__ float score(float dot, int64_t item) const { return ((dot + mu) + ub) + a.bi[item]; }
};

template <int UPB, int CAP, bool V4>
__global__ __launch_bounds__(256) void k_topk_score(TopkArgs a) {
    warm_args(a);
    sliced_topk_block<UPB, CAP, V4, TopkScorer>(a, a.U, 0, a.n_items);
}

__global__ __launch_bounds__(64) void k_topk_merge(TopkMergeArgs a) {
    extern __shared__ uint64_t keys[];
    warm_args(a);
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int k = a.k, S = a.slices;
    const uint64_t* src = a.part + (size_t)row * S * k;
    for (int t = lane; t < S * k; t += 64) keys[t] = src[t];
    __syncthreads();
    // lane holds the heads of lists lane, lane + 64, lane + 128, lane + 192
    int hd[4];
    uint64_t cur[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        const int s = lane + 64 * z;
        hd[z] = 0;
        cur[z] = s < S ? keys[s * k] : 0;
    }
    int32_t* io = a.items_out + (size_t)row * k;
    float* so = a.scores_out ? a.scores_out + (size_t)row * k : nullptr;
    int q = 0;
    for (; q < k; ++q) {
        uint64_t best = cur[0];
        int bz = 0;
#pragma unroll
        for (int z = 1; z < 4; ++z) if (cur[z] > best) { best = cur[z]; bz = z; }
        uint64_t m = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(m, off);
            m = o > m ? o : m;
        }
        if (m == 0) break;                             // every list is exhausted
        if (best == m) {                               // keys are distinct: exactly one lane
            io[q] = (int32_t)~(uint32_t)m;
            if (so) so[q] = topk_key_score(m);
#pragma unroll
            for (int z = 0; z < 4; ++z)
                if (z == bz) {
                    ++hd[z];
                    cur[z] = hd[z] < k ? keys[(lane + 64 * z) * k + hd[z]] : 0;
                }
        }
    }
    for (int t = q + lane; t < k; t += 64) {
        io[t] = -1;
        if (so) so[t] = -INFINITY;
    }
}

__global__ __launch_bounds__(256) void k_topk_check_excl(const int64_t* indptr, const int32_t* x, int64_t n_rows,
                                                         int64_t n_items, int32_t* bad, int32_t* err) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_rows; row += (int64_t)gridDim.x * 4) {
        const int64_t lo = indptr[row], hi = indptr[row + 1];
        int32_t f = 0;
        if (lo < 0 || hi < lo) {
            f = 16;                                    // the items of a malformed row are not read
        } else {
            for (int64_t t = lo + lane; t < hi; t += 64) {
                const int32_t v = x[t];
                if (v < 0 || (int64_t)v >= n_items) f |= 1;
                if (t > lo && x[t - 1] > v) f |= 16;
            }
        }
        if (f) { atomicOr(bad, 1); atomicOr(err, f); }
    }
}

void launch_topk_score(const TopkArgs& a, const TopkPlan& p, hipStream_t s) {
    launch_score_kernel(k_topk_score<32, 256, true>, k_topk_score<32, 256, false>, k_topk_score<16, 512, true>,
                        k_topk_score<16, 512, false>, a, p, s);
}

void launch_topk_merge(const TopkMergeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)a.n_rows), dim3(64), topk_merge_lds(a.slices, a.k), s, a);
}

void launch_topk_check_excl(const int64_t* indptr, const int32_t* excl, int64_t n_rows, int64_t n_items, int32_t* bad,
                            int32_t* err, hipStream_t s) {
    int64_t nb = (n_rows + 3) / 4;
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_topk_check_excl, dim3((unsigned)nb), dim3(256), 0, s, indptr, excl, n_rows, n_items, bad, err);
}

}  // namespace tfr
