// warp.hip - the violator search of a WARP step on gfx950 (wave64).  DESIGN §30.
//
// One wave per triple (u, i).  Lane t forms candidate c_t (the draw k_bpr_sample makes at attempt t) and searches row u of
// the positives for it; one ballot gives the set of non-positive candidates.  The wave then walks that set in order,
// WARP_GROUP candidates per round: their rows are loaded together (independent loads), dotted with P[u] held in registers
// (features across the lanes as in k_bpr_users, f = lane + 64 j), and compared in order; the search stops at the first
// x = (d_i + bi[i]) - (d_c + bi[c]) < margin.  x is bpr_x on dots formed as k_bpr_users forms them, so the user run that
// follows sees the bits the search compared.  Every branch is wave-uniform (the ballot, and butterfly sums that leave the
// same bits in every lane).  No LDS, no atomic, no block barrier; lane 0 writes the triple's outputs.
#include <hip/hip_runtime.h>
#include "warp.h"
#include "wave_rows.h"

namespace tfr {

static_assert(BPR_WAVES == ROW_WAVES, "wave_slot and wave_grid count ROW_WAVES waves per block");
static_assert(BPR_MAX_ATTEMPTS <= 64, "one lane per candidate");

// w of a triple whose violator was the N-th non-positive candidate (N >= 1): the restatement in include/tfrecomm.h
__device__ __forceinline__ float warp_weight(int64_t I, int32_t N) {
    const int32_t r = (int32_t)((I - 1) / N);
    return logf((float)(r > 1 ? r : 1));
}

template <int NJ>
__global__ void __launch_bounds__(64 * BPR_WAVES) k_warp_sample(WarpSampleArgs a) {
    const int64_t b = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    if (b >= a.B) return;
    int32_t u = -1, i = 0;
    if (a.ids) {
        const int64_t e = a.ids[b];
        if (e >= 0 && e < a.pos.nnz) {                             // (always: the draw is randint(0, nnz))
            u = a.pos.rowof[e];
            i = a.pos.idx[e];
        }
    } else {
        u = a.u_in[b];
        i = a.i_in[b];
    }
    int32_t j = -1, N = 0;
    float w = 0.f;
    if (a.neg_in) {
        j = a.neg_in[b];                                           // as given: the sort checks it
        N = 1;
        w = warp_weight(a.I, 1);
    } else if (u >= 0 && u < a.U && i >= 0 && i < a.I) {           // (a bad id voids the step in the sort: no row is read)
        int32_t c = 0;
        bool open = false;                                         // c_t is not a positive of u
        if (lane < a.attempts) {
            const uint64_t r = bpr_mix(a.key ^ (((uint64_t)b << 6) | (uint64_t)lane));
            c = (int32_t)(((r >> 32) * (uint64_t)a.I) >> 32);
            const int64_t hi0 = a.pos.ip[u + 1];
            int64_t lo = a.pos.ip[u], hi = hi0;                    // first entry of the row >= c
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.pos.idx[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            open = lo == hi0 || a.pos.idx[lo] != c;
        }
        unsigned long long todo = __ballot(open);
        if (todo) {
            const int64_t urow = (int64_t)u * D, irow = (int64_t)i * D;
            float pu[NJ], di = 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const int f = lane + 64 * k;
                pu[k] = f < D ? a.P[urow + f] : 0.f;
            }
            each_feature<NJ>(lane, D, [&](int k, int f) {
                const float x1 = a.Q[irow + f];
                di = fmaf(pu[k], a.item_abs ? fabsf(x1) : x1, di);
            });
            di = wave_sum_all(di);
            const float bii = a.bi[i];
            while (todo && j < 0) {
                int32_t cs[WARP_GROUP];
                float dc[WARP_GROUP], bc[WARP_GROUP];
#pragma unroll
                for (int g = 0; g < WARP_GROUP; ++g) {             // the next WARP_GROUP open candidates, in order
                    cs[g] = -1;
                    if (todo) {
                        const int t = __ffsll((long long)todo) - 1;
                        todo &= todo - 1;
                        cs[g] = __shfl(c, t, 64);
                    }
                }
#pragma unroll
                for (int g = 0; g < WARP_GROUP; ++g) {             // their rows: loads that do not wait for one another
                    dc[g] = 0.f;
                    bc[g] = 0.f;
                    if (cs[g] < 0) continue;
                    const int64_t crow = (int64_t)cs[g] * D;
                    each_feature<NJ>(lane, D, [&](int k, int f) {
                        const float x2 = a.Q[crow + f];
                        dc[g] = fmaf(pu[k], a.item_abs ? fabsf(x2) : x2, dc[g]);
                    });
                    bc[g] = a.bi[cs[g]];
                }
#pragma unroll
                for (int g = 0; g < WARP_GROUP; ++g) dc[g] = wave_sum_all(dc[g]);
#pragma unroll
                for (int g = 0; g < WARP_GROUP; ++g) {
                    if (cs[g] < 0 || j >= 0) continue;
                    ++N;
                    if (bpr_x(di, bii, dc[g], bc[g]) < a.margin) j = cs[g];
                }
            }
        }
        if (j < 0) N = 0;                                          // no violator: skipped
        else w = warp_weight(a.I, N);
    }
    if (lane != 0) return;
    if (a.neg) a.neg[b] = j;
    if (a.trials) a.trials[b] = N;
    if (a.wgt) a.wgt[b] = w;
    if (a.neg_copy) a.neg_copy[b] = j;
    if (a.trials_copy) a.trials_copy[b] = N;
    if (a.pos_out) a.pos_out[b] = i;
    if (a.ou) {
        a.ou[2 * b] = u;
        a.ou[2 * b + 1] = u;
        a.oi[2 * b] = i;
        a.oi[2 * b + 1] = (j < 0 && !a.neg_in) ? i : j;            // a skipped triple sorts with its positive
    }
}

void launch_warp_sample(const WarpSampleArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    with_nj(a.D, [&](auto nj) { hipLaunchKernelGGL(k_warp_sample<decltype(nj)::value>, wave_grid(a.B), wave_block(), 0, s, a); });
}

}  // namespace tfr
