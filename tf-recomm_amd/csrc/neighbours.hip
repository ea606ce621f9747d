// neighbours.hip - nearest neighbours in factor space on gfx950: "what is like item i", "who is like user u".
//
// k_row_rnorm: a wave owns 64 rows, one lane each; the lane runs the f32 fmaf chain of its row's squares in f order and
//   writes rn = 1 / sqrtf(ss), 0 for a zero row.  Runs once per (table, step counter, table generation); api.hip keeps the rule.
// k_nb_score: k_topk_score with both MFMA operands from the one table.  A block owns a tile of query rows (the B block) and a
//   slice of the candidate range (the A block, 32 rows per wave and round).  The accumulator is the dot; the cosine form
//   scales it by rn[query] and then rn[candidate]; the query row itself, excluded rows and NaN scores make no key.  Queues,
//   thresholds, the per-slice lists and their merge (launch_topk_merge) are those of topk.hip.
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

template <int UPB, int CAP, bool V4>
__global__ __launch_bounds__(256) void k_nb_score(NbArgs a) {
    __shared__ uint64_t queue[UPB * CAP];
    __shared__ uint64_t thr[UPB];
    __shared__ int32_t cnt[UPB];
    static_assert(sizeof(queue) + sizeof(thr) + sizeof(cnt) == topk_score_static_lds(UPB, CAP),
                  "tfr_neighbours_plan reports a different LDS size than the kernel declares");
    static_assert(CAP - TOPK_ROUND >= (CAP == 256 ? 128 : TOPK_KMAX), "a queue must hold k plus one round of appends");
    warm_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int j = c & (UPB - 1);                       // query of this lane's accumulator column
    const bool own_col = c < UPB;                      // UPB 16: columns 16..31 repeat 0..15 and select nothing
    const int64_t row = (int64_t)blockIdx.x * UPB + j;
    const int slice = blockIdx.y;
    const int k = a.k;

    int32_t qid = -1;
    if (row < a.n_rows) {
        qid = a.rows[row];
        if (qid < 0 || (int64_t)qid >= a.R) {
            if (own_col && h == 0) atomicOr(a.err, 1);
            qid = -1;
        }
    }
    const bool live = own_col && qid >= 0;
    int64_t xlo = 0, xhi = 0;
    if (live && a.indptr && *a.excl_bad == 0) { xlo = a.indptr[row]; xhi = a.indptr[row + 1]; }
    const float* brow = a.T + (int64_t)(qid < 0 ? 0 : qid) * a.D;
    const bool cosine = a.rn != nullptr;
    const float rq = cosine && qid >= 0 ? a.rn[qid] : 0.f;
    for (int t = threadIdx.x; t < UPB; t += 256) { cnt[t] = 0; thr[t] = 0; }
    __syncthreads();

    const int64_t n_cand = a.hi - a.lo;
    const int64_t per = ((n_cand + a.slices - 1) / a.slices + TOPK_ROUND - 1) / TOPK_ROUND * TOPK_ROUND;
    const int64_t s_lo = a.lo + (int64_t)slice * per;
    const int64_t s_hi = s_lo + per < a.hi ? s_lo + per : a.hi;
    const int64_t rounds = s_hi > s_lo ? (s_hi - s_lo + TOPK_ROUND - 1) / TOPK_ROUND : 0;

    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t base = s_lo + rd * TOPK_ROUND + wave * TOPK_SUB;
        int64_t my_cand = base + c;                    // A row = candidate; past the slice: a row inside it, result dropped
        if (my_cand >= s_hi) my_cand = s_hi - 1;
        const float* arow = a.T + my_cand * a.D;
        const f32x16 acc = mfma_tile_dot<V4, true>(arow, brow, a.D, a.item_abs, h);
        // C[candidate row][query column]: this lane holds query j, candidates base + (r&3) + 8(r>>2) + 4h
        const uint64_t th = thr[j];
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t cand = base + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (cand < s_hi && cand != qid) {
                    float s = acc[r];
                    if (cosine) s = (s * rq) * a.rn[cand];
                    if (!__builtin_isnan(s)) {
                        const uint64_t key = topk_key(s, cand);
                        if (key > th && !(xhi > xlo && topk_excluded(a.excl, xlo, xhi, (int32_t)cand))) {
                            const int pos = atomicAdd(&cnt[j], 1);
                            queue[j * CAP + pos] = key;
                        }
                    }
                }
            }
        }
        __syncthreads();
        for (int u = wave; u < UPB; u += TOPK_WAVES)
            if (cnt[u] > CAP - TOPK_ROUND) topk_compact<CAP>(queue + u * CAP, cnt + u, thr + u, k, lane);
        __syncthreads();
    }
    for (int u = wave; u < UPB; u += TOPK_WAVES) {
        const int64_t rw = (int64_t)blockIdx.x * UPB + u;
        if (rw >= a.n_rows) continue;
        if (cnt[u] > 0) topk_compact<CAP>(queue + u * CAP, cnt + u, thr + u, k, lane);
        const int n = cnt[u];
        uint64_t* dst = a.part + ((size_t)rw * a.slices + slice) * k;
        for (int q = lane; q < k; q += 64) dst[q] = q < n ? queue[u * CAP + q] : 0;
    }
}

template <int UPB, int CAP>
static void launch_nb_v(const NbArgs& a, dim3 g, hipStream_t s) {
    if ((a.D & 3) == 0) hipLaunchKernelGGL((k_nb_score<UPB, CAP, true>), g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_nb_score<UPB, CAP, false>), g, dim3(256), 0, s, a);
}

void launch_nb_score(const NbArgs& a, const NbPlan& p, hipStream_t s) {
    const dim3 g((unsigned)((a.n_rows + p.upb - 1) / p.upb), (unsigned)p.slices);
    if (p.cap == 256) launch_nb_v<32, 256>(a, g, s);
    else launch_nb_v<16, 512>(a, g, s);
}

void launch_row_rnorm(const float* T, int64_t R, int32_t D, float* rn, hipStream_t s) {
    const dim3 g((unsigned)((R + NB_RNORM_ROWS - 1) / NB_RNORM_ROWS));
    if ((D & 3) == 0) hipLaunchKernelGGL(k_row_rnorm<true>, g, dim3(NB_RNORM_ROWS), 0, s, T, R, D, rn);
    else hipLaunchKernelGGL(k_row_rnorm<false>, g, dim3(NB_RNORM_ROWS), 0, s, T, R, D, rn);
}

}  // namespace tfr
