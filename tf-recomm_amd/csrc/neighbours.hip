// neighbours.hip - nearest neighbours in factor space on gfx950: "what is like item i", "who is like user u".
//
// k_row_rnorm: a wave owns 64 rows, one lane each; the lane runs the f32 fmaf chain of its row's squares in f order and
//   writes rn = 1 / sqrtf(ss), 0 for a zero row.  Runs once per (table, step counter, table generation); api.hip keeps the rule.
// k_nb_score: the scoring block of score_tile.h (sliced_topk_block, the one k_topk_score runs) with NbScorer: both MFMA
//   operands from the one table, a tile of query rows (the B block) against a slice of the candidate range (the A block).  The
//   accumulator is the dot; the cosine form scales it by rn[query] and then rn[candidate]; the query row itself, excluded
//   rows and NaN scores make no key.  The per-slice lists are merged by topk.hip's launch_topk_merge.
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "neighbours.h"

namespace tfr {

template <bool V4>
__global__ __launch_bounds__(NB_RNORM_ROWS) void k_row_rnorm(const float* T, int64_t R, int32_t D, float* rn) {
    const int64_t row = (int64_t)blockIdx.x * NB_RNORM_ROWS + threadIdx.x;
    if (row >= R) return;
    const float* x = T + row * D;
    float ss = 0.f;
    if (V4) {
        for (int f = 0; f < D; f += 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + f);
            ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
        }
    } else {
        for (int f = 0; f < D; ++f) ss = fmaf(x[f], x[f], ss);
    }
    rn[row] = ss == 0.f ? 0.f : 1.0f / sqrtf(ss);
}

// dot, or (dot * rn[query]) * rn[candidate] with rn given; both MFMA operands are rows of T, the query itself is no candidate
struct NbScorer {
    static constexpr bool ABS_B = true;
    const NbArgs& a;
    const float* brow;
    int32_t qid;
    bool cosine;
    float rq;
    __device__ __forceinline__ NbScorer(const NbArgs& a_, int32_t q)
        : a(a_), brow(a_.T + (int64_t)(q < 0 ? 0 : q) * a_.D), qid(q), cosine(a_.rn != nullptr),
          rq(cosine && q >= 0 ? a_.rn[q] : 0.f) {}
    __device__ __forceinline__ const float* arow(int64_t cand) const { return a.T + cand * a.D; }
    template <bool V4>
    __device__ __forceinline__ f32x16 tile(int64_t cand, int h) const {
        return mfma_tile_dot<V4, ABS_B>(arow(cand), brow, a.D, a.item_abs, h);
    }
    __device__ __forceinline__ bool eligible(int64_t cand) const { return cand != qid; }
    __device__ __forceinline__ float score(float dot, int64_t cand) const { return cosine ? (dot * rq) * a.rn[cand] : dot; }
};

template <int UPB, int CAP, bool V4>
__global__ __launch_bounds__(256) void k_nb_score(NbArgs a) {
    warm_args(a);
    sliced_topk_block<UPB, CAP, V4, NbScorer>(a, a.R, a.lo, a.hi);
}

void launch_nb_score(const NbArgs& a, const TopkPlan& p, hipStream_t s) {
    launch_score_kernel(k_nb_score<32, 256, true>, k_nb_score<32, 256, false>, k_nb_score<16, 512, true>,
                        k_nb_score<16, 512, false>, a, p, s);
}

void launch_row_rnorm(const float* T, int64_t R, int32_t D, float* rn, hipStream_t s) {
    const dim3 g((unsigned)((R + NB_RNORM_ROWS - 1) / NB_RNORM_ROWS));
    if ((D & 3) == 0) hipLaunchKernelGGL(k_row_rnorm<true>, g, dim3(NB_RNORM_ROWS), 0, s, T, R, D, rn);
    else hipLaunchKernelGGL(k_row_rnorm<false>, g, dim3(NB_RNORM_ROWS), 0, s, T, R, D, rn);
}

}  // namespace tfr
