// bpr.hip - the BPR step kernels on gfx950 (wave64): the negative sampler, the user runs and the item runs.  DESIGN §15.
//
// The sampler gives one thread to a triple.  The other two kernels give one wave to a run of a sorted 2B-key column;
// features lie across the lanes, NJ = ceil(D / 64) per lane (f = lane + 64 j).  No kernel has a block barrier or an atomic:
// a row is written by the one wave that owns it, and every sum runs in a fixed order:
//   user run   its triples in batch order (the stable sort keeps 2b, 2b+1 adjacent): s_i, s_j, x, g, the data and
//              regulariser terms, dP; the pre-step P row goes to pold before the row is updated
//   item run   its occurrences in occurrence order: +g_b P[u_b] for 2b, -g_b P[u_b] for 2b+1, P read from pold
// The user runs read Q before the item runs write it (kernel boundary); the item runs read P from pold, which holds it as
// it was before the user runs wrote it.  Both sides therefore see the tables as they were before the step.
#include <hip/hip_runtime.h>
#include "bpr.h"
#include "wave_rows.h"

namespace tfr {

static_assert(BPR_WAVES == ROW_WAVES, "wave_slot and wave_grid count ROW_WAVES waves per block");

// lazy Adam (touched rows) in the SVD step's operation order (adam_sparse), or SGD, on one value
__device__ __forceinline__ void bpr_update(float* w, float* m, float* v, int64_t x, float g, const BprArgs& a) {
    update_at(w, m, v, x, g, a.opt == 0, AdamC{a.alpha, a.b1, a.b2, a.eps, a.omb1, a.omb2}, a.lr);
}

__global__ void __launch_bounds__(256) k_bpr_sample(BprSampleArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
        if (a.i_in) i = a.i_in[b];
    }
    int32_t j = -1;
    if (a.neg_in) {
        j = a.neg_in[b];                                           // as given: the sort checks it
    } else if (u >= 0 && u < a.U) {                                // (a bad user voids the step in the sort)
        const int64_t lo0 = a.pos.ip[u], hi0 = a.pos.ip[u + 1];
        for (int t = 0; t < a.attempts; ++t) {
            const uint64_t r = bpr_mix(a.key ^ (((uint64_t)b << 6) | (uint64_t)t));
            const int32_t c = (int32_t)(((r >> 32) * (uint64_t)a.I) >> 32);
            int64_t lo = lo0, hi = hi0;                            // first entry of the row >= c
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.pos.idx[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo == hi0 || a.pos.idx[lo] != c) {
                j = c;
                break;
            }
        }
    }
    if (a.neg) a.neg[b] = j;
    if (a.neg_copy) a.neg_copy[b] = j;
    if (a.pos_out) a.pos_out[b] = i;
    if (a.ou) {
        a.ou[2 * b] = u;
        a.ou[2 * b + 1] = u;
        a.oi[2 * b] = i;
        a.oi[2 * b + 1] = (j < 0 && !a.neg_in) ? i : j;            // a skipped triple sorts with its positive
    }
}

// HINGE: the weighted hinge of a WARP step (warp.h) in place of the logistic g and the softplus term
template <int NJ, bool HINGE>
__global__ void __launch_bounds__(64 * BPR_WAVES) k_bpr_users(BprArgs a) {
    const int64_t w = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    if (w >= a.B || *a.err) return;
    const int64_t p = 2 * w, n = 2 * a.B;                          // a run holds whole triples: it starts at an even position
    const int32_t u = a.ks_u[p];
    if (p > 0 && a.ks_u[p - 1] == u) {                             // not a run head: an empty partial for the finish
        if (lane < 4) a.scal[w * 4 + lane] = 0.f;
        return;
    }
    const int64_t q = sorted_run_end(a.ks_u, p, n, lane);
    const int64_t urow = (int64_t)u * D;
    float pu[NJ], dp[NJ], psq = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int f = lane + 64 * j;
        pu[j] = f < D ? a.P[urow + f] : 0.f;
        dp[j] = 0.f;
        if (f < D) a.pold[w * D + f] = pu[j];
        psq = fmaf(pu[j], pu[j], psq);
    }
    psq = wave_sum_all(psq);
    const float lam = a.lam;
    float loss = 0.f, reg = 0.f;
    int32_t cnt = 0;
    for (int64_t e = p; e < q; e += 2) {
        const int32_t b = a.ps_u[e] >> 1;
        if (lane == 0) a.head[b] = (int32_t)w;
        const int32_t jn = a.neg[b];
        if (jn < 0) continue;                                      // skipped: absent from the batch
        const int32_t ip = a.pos[b];
        const int64_t irow = (int64_t)ip * D, jrow = (int64_t)jn * D;
        float qi[NJ] = {}, qj[NJ] = {}, di = 0.f, dj = 0.f, qisq = 0.f, qjsq = 0.f;
        each_feature<NJ>(lane, D, [&](int j, int f) {
            const float x1 = a.Q[irow + f], x2 = a.Q[jrow + f];
            qi[j] = a.item_abs ? fabsf(x1) : x1;
            qj[j] = a.item_abs ? fabsf(x2) : x2;
            di = fmaf(pu[j], qi[j], di);
            dj = fmaf(pu[j], qj[j], dj);
            qisq = fmaf(x1, x1, qisq);
            qjsq = fmaf(x2, x2, qjsq);
        });
        di = wave_sum_all(di);
        dj = wave_sum_all(dj);
        qisq = wave_sum_all(qisq);
        qjsq = wave_sum_all(qjsq);
        const float bii = a.bi[ip], bij = a.bi[jn];
        const float x = bpr_x(di, bii, dj, bij);
        const float wb = HINGE ? a.wgt[b] : 0.f;                   // (HINGE is a template argument: one side is compiled)
        const float g = HINGE ? (x < a.margin ? -wb : 0.f)
                              : -1.f / (1.f + expf(x));           // -sigmoid(-x)
        loss += HINGE ? wb * fmaxf(a.margin - x, 0.f)
                      : fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))); // softplus(-x)
        float rk = (0.5f * psq + 0.5f * qisq) + 0.5f * qjsq;
        if (a.reg_bias) rk += 0.5f * (bii * bii) + 0.5f * (bij * bij);
        reg += rk;
#pragma unroll
        for (int j = 0; j < NJ; ++j) dp[j] += fmaf(g, qi[j] - qj[j], lam * pu[j]);
        if (lane == 0) a.g[b] = g;
        ++cnt;
    }
    if (lane == 0) {
        a.scal[w * 4 + 0] = loss;
        a.scal[w * 4 + 1] = reg;
        a.scal[w * 4 + 2] = 0.f;
        a.scal[w * 4 + 3] = 0.f;
    }
    if (cnt == 0 || ((a.frozen >> 3) & 1)) return;                 // every triple skipped: the row and its slots stay
    each_feature<NJ>(lane, D, [&](int j, int f) { bpr_update(a.P, a.Pm, a.Pv, urow + f, dp[j], a); });
}

template <int NJ>
__global__ void __launch_bounds__(64 * BPR_WAVES) k_bpr_items(BprArgs a) {
    const int64_t p = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    const int64_t n = 2 * a.B;
    if (p >= n || *a.err) return;
    const int32_t it = a.ks_i[p];
    if (p > 0 && a.ks_i[p - 1] == it) return;
    const int64_t q = sorted_run_end(a.ks_i, p, n, lane);
    const int64_t irow = (int64_t)it * D;
    const float lam = a.lam, bi = a.bi[it];
    float qr[NJ], sg[NJ], dq[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int f = lane + 64 * j;
        qr[j] = f < D ? a.Q[irow + f] : 0.f;
        sg[j] = a.item_abs ? (qr[j] > 0.f ? 1.f : qr[j] < 0.f ? -1.f : 0.f) : 1.f;
        dq[j] = 0.f;
    }
    float dbi = 0.f;
    int32_t cnt = 0;
    for (int64_t e = p; e < q; ++e) {
        const int32_t k = a.ps_i[e];
        const int32_t b = k >> 1;
        if (a.neg[b] < 0) continue;                                // skipped: absent from the batch
        const float gb = a.g[b];
        const float g = (k & 1) ? -gb : gb;
        const float* pr = a.pold + (int64_t)a.head[b] * D;
        each_feature<NJ>(lane, D, [&](int j, int f) { dq[j] += (g * pr[f]) * sg[j] + lam * qr[j]; });
        dbi += a.reg_bias ? g + lam * bi : g;
        ++cnt;
    }
    if (cnt == 0) return;                                          // only skipped triples: no touch
    if (!((a.frozen >> 4) & 1)) each_feature<NJ>(lane, D, [&](int j, int f) { bpr_update(a.Q, a.Qm, a.Qv, irow + f, dq[j], a); });
    if (!((a.frozen >> 2) & 1) && lane == 0) bpr_update(a.bi, a.bim, a.biv, it, dbi, a);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_bpr_sample(const BprSampleArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(k_bpr_sample, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, s, a);
}

void launch_bpr_users(const BprArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    with_nj(a.D, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        if (a.wgt) hipLaunchKernelGGL((k_bpr_users<NJ, true>), wave_grid(a.B), wave_block(), 0, s, a);
        else hipLaunchKernelGGL((k_bpr_users<NJ, false>), wave_grid(a.B), wave_block(), 0, s, a);
    });
}

void launch_bpr_items(const BprArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    with_nj(a.D, [&](auto nj) { hipLaunchKernelGGL(k_bpr_items<decltype(nj)::value>, wave_grid(2 * a.B), wave_block(), 0, s, a); });
}

}  // namespace tfr
