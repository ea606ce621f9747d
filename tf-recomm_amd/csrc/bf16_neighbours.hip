// bf16_neighbours.hip - nearest neighbours in factor space from the bf16 snapshot (tfr_bf16_neighbours*).
//
// k_row_rnorm_bf16: a wave owns 64 snapshot rows, one lane each; the lane reads its row in 16-byte loads, widens every
//   element (bits << 16) and runs the f32 fmaf chain of the squares in f order; rn = 1 / sqrtf(ss), 0 for a zero row.  The
//   square of a widened bf16 value is exact in float32 and a pad adds fma(0, 0, ss) = ss, so ss is plain float32 arithmetic.
// k_nb_score_bf16: the scoring block of score_tile.h (sliced_topk_block, the one k_nb_score runs) with Bf16NbScorer: both
//   MFMA operands are rows of the one snapshot table (mfma_tile_dot_bf16<ABS_B>: item_abs clears the sign bits of both), the
//   cosine form scales the dot by rn[query] and then rn[candidate]; the query row itself, excluded rows and NaN scores make
//   no key.  Snapshot rows are always 16-byte aligned: no V4 argument.  The merge is topk.hip's launch_topk_merge.
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "neighbours.h"

namespace tfr {

__global__ __launch_bounds__(NB_RNORM_ROWS) void k_row_rnorm_bf16(const uint16_t* T, int64_t R, int32_t DP, float* rn) {
    const int64_t row = (int64_t)blockIdx.x * NB_RNORM_ROWS + threadIdx.x;
    if (row >= R) return;
    const u32x4* x = reinterpret_cast<const u32x4*>(T + row * DP);
    const int NF = DP >> 3;
    float ss = 0.f;
    for (int f = 0; f < NF; ++f) {
        const u32x4 v = x[f];
#pragma unroll
        for (int w = 0; w < 4; ++w) {                  // a word holds elements 2w (low half) and 2w + 1 of the fragment
            const float lo = __uint_as_float(v[w] << 16), hi = __uint_as_float(v[w] & 0xffff0000u);
            ss = fmaf(lo, lo, ss);
            ss = fmaf(hi, hi, ss);
        }
    }
    rn[row] = ss == 0.f ? 0.f : 1.0f / sqrtf(ss);
}

// dot, or (dot * rn[query]) * rn[candidate] with rn given; both MFMA operands are rows of T, the query itself is no candidate
struct Bf16NbScorer {
    const Bf16NbArgs& a;
    const uint16_t* brow;
    int32_t qid;
    bool cosine;
    float rq;
    __device__ __forceinline__ Bf16NbScorer(const Bf16NbArgs& a_, int32_t q)
        : a(a_), brow(a_.T + (int64_t)(q < 0 ? 0 : q) * a_.DP), qid(q), cosine(a_.rn != nullptr),
          rq(cosine && q >= 0 ? a_.rn[q] : 0.f) {}
    template <bool>
    __device__ __forceinline__ f32x16 tile(int64_t cand, int h) const {
        return mfma_tile_dot_bf16<true>(a.T + cand * a.DP, brow, a.DP, a.item_abs, h);
    }
    __device__ __forceinline__ bool eligible(int64_t cand) const { return cand != qid; }
    __device__ __forceinline__ float score(float dot, int64_t cand) const { return cosine ? (dot * rq) * a.rn[cand] : dot; }
};

template <int UPB, int CAP>
__global__ __launch_bounds__(256) void k_nb_score_bf16(Bf16NbArgs a) {
    warm_args(a);
    sliced_topk_block<UPB, CAP, true, Bf16NbScorer>(a, a.R, a.lo, a.hi);
}

void launch_bf16_nb_score(const Bf16NbArgs& a, const TopkPlan& p, hipStream_t s) {
    const dim3 g((unsigned)((a.n_rows + p.upb - 1) / p.upb), (unsigned)p.slices);
    void (*const kern)(Bf16NbArgs) = p.cap == 256 ? k_nb_score_bf16<32, 256> : k_nb_score_bf16<16, 512>;
    hipLaunchKernelGGL(kern, g, dim3(256), 0, s, a);
}

void launch_row_rnorm_bf16(const uint16_t* T, int64_t R, int32_t DP, float* rn, hipStream_t s) {
    const dim3 g((unsigned)((R + NB_RNORM_ROWS - 1) / NB_RNORM_ROWS));
    hipLaunchKernelGGL(k_row_rnorm_bf16, g, dim3(NB_RNORM_ROWS), 0, s, T, R, DP, rn);
}

}  // namespace tfr
