// finetune.hip - batched per-user fine-tuning on gfx950 (tfr_finetune_users): the rounds of adaptive_test.py:87-116 and
// non_adaptive_test.py:56-87 for every user of a schedule in one launch.
//
// With mu and the item tables frozen and an optimiser that touches only the rows it is given (SGD, lazy Adam), one user's
// steps read and write only that user's row, bias and slots: the users are independent chains.  k_finetune gives each
// user one wave (FT_WAVES independent waves per block, no block barrier) and runs its rounds in order:
//   ask logit   ((dot(p, q'[ask]) + mu) + bu) + bi[ask] with the parameters of the moment (q' = |q| with item_abs)
//   nsteps x    logit phase (lane = row of the prefix, 64 rows per pass): the f32 fmaf chain over f ascending from +0, the
//               forward's order of the bias adds, dlogit = logit - r (mse) or sigmoid(logit) - r (nll);
//               gradient phase (lane = feature): g_f = sum over the prefix rows, in row order, of fmaf(dlogit_k, q'_kf,
//               lam * p_f) - the regulariser over the gathered rows, one lam * p per occurrence, as the step sums them -
//               and the bias likewise (+ lam * bu per occurrence with reg_bias);
//               then SGD (w - lr * g) or lazy Adam with lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) from the beta powers
//               the host replayed to the round's sequential position, advanced here step by step.
// Every sum has a fixed order and nothing is shared between waves, so a user's results do not depend on which other users
// share the launch, or on the order the host gives the users (descending work, so the long chains start first).
#include <hip/hip_runtime.h>
#include "finetune.h"
#include "wave_rows.h"

namespace tfr {

static_assert(FT_WAVES == ROW_WAVES, "wave_slot and wave_grid count ROW_WAVES waves per block");

__device__ __forceinline__ float ft_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }

// the item row value a lane reads: staged in LDS (|q| already taken) or from the table
template <bool STAGED>
__device__ __forceinline__ float ft_q(const float* q_s, int S, const float* Q, const int32_t* it, int64_t k, int f, int D,
                                      int item_abs) {
    if constexpr (STAGED) {
        return q_s[k * S + f];
    } else {
        const float q = Q[(int64_t)it[k] * D + f];
        return item_abs ? fabsf(q) : q;
    }
}

template <int NJ, bool STAGED>
__device__ void ft_user(const FtArgs& a, float* w, int32_t uix, int lane) {
    const int D = a.D, S = ft_stride(D), dp = ft_dpad(D);
    const int64_t user = a.users[uix];
    const int64_t r0 = a.row_ptr[uix], n = a.row_ptr[uix + 1] - r0;
    const int64_t k0 = a.round_ptr[uix], k1 = a.round_ptr[uix + 1];
    if (k0 == k1) return;                              // no rounds: the user's rows stay as they are
    const int32_t* it = a.items + r0;
    const float* rt = a.rates + r0;
    float* p_s = w;
    float* aq_s = p_s + dp;
    float* dl_s = aq_s + dp;
    float* ls_s = dl_s + 64;
    float* bi_s = ls_s + 64;
    float* r_s = bi_s + a.rows_staged;
    float* q_s = r_s + a.rows_staged;
    if constexpr (STAGED) {
        for (int64_t e = lane; e < n * D; e += 64) {
            const int64_t k = e / D;
            const int f = (int)(e - k * D);
            const float q = a.Q[(int64_t)it[k] * D + f];
            q_s[k * S + f] = a.item_abs ? fabsf(q) : q;
        }
        for (int64_t k = lane; k < n; k += 64) { bi_s[k] = a.bi[it[k]]; r_s[k] = rt[k]; }
    }
    float p[NJ], m[NJ], v[NJ];
    const int64_t prow = user * D;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {                     // (clears the registers past D as it loads: not each_feature's shape)
        const int f = lane + 64 * j;
        p[j] = m[j] = v[j] = 0.f;
        if (f < D) {
            p[j] = a.P[prow + f];
            if (a.adam) { m[j] = a.Pm[prow + f]; v[j] = a.Pv[prow + f]; }
        }
    }
    float bu = a.bu[user], bm = 0.f, bv = 0.f;
    if (a.adam) { bm = a.bum[user]; bv = a.buv[user]; }
    const float mu = a.mu[0], lam = a.lam, lr = a.lr;
    const float omb1 = 1.f - a.b1, omb2 = 1.f - a.b2;
    for (int64_t kr = k0; kr < k1; ++kr) {
        const int64_t L = a.prefix[kr];
        const int32_t ask = a.ask[kr];
        each_feature<NJ>(lane, D, [&](int j, int f) {
            p_s[f] = p[j];
            const float q = a.Q[(int64_t)ask * D + f];
            aq_s[f] = a.item_abs ? fabsf(q) : q;
        });
        wave_lds_sync();
        {
            float s = 0.f;
            for (int f = 0; f < D; ++f) s = fmaf(p_s[f], aq_s[f], s);
            const float logit = ((s + mu) + bu) + a.bi[ask];
            if (lane == 0) a.ask_out[kr] = logit;
        }
        float b1p = 0.f, b2p = 0.f;
        if (a.adam) { b1p = a.bpow[2 * kr]; b2p = a.bpow[2 * kr + 1]; }
        for (int32_t st = 0; st < a.nsteps; ++st) {
            const bool last = st + 1 == a.nsteps;
            const bool want_loss = last && a.loss_out;
            const bool want_final = last && a.final_out && kr + 1 == k1;
            float g[NJ], lp[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) { g[j] = 0.f; lp[j] = lam * p[j]; }
            const float lbu = lam * bu;
            float gb = 0.f, lsum = 0.f;
            for (int64_t c0 = 0; c0 < L; c0 += 64) {
                // logit phase: lane = row c0 + lane of the prefix
                const int64_t k = c0 + lane;
                float dl = 0.f, l = 0.f;
                if (k < L) {
                    float s = 0.f;
                    if constexpr (STAGED) {
                        const float* qk = q_s + k * S;
#pragma unroll 4
                        for (int f = 0; f < D; ++f) s = fmaf(p_s[f], qk[f], s);
                    } else {
                        const float* qk = a.Q + (int64_t)it[k] * D;
#pragma unroll 4
                        for (int f = 0; f < D; ++f) s = fmaf(p_s[f], a.item_abs ? fabsf(qk[f]) : qk[f], s);
                    }
                    const float bik = STAGED ? bi_s[k] : a.bi[it[k]];
                    const float rk = STAGED ? r_s[k] : rt[k];
                    const float logit = ((s + mu) + bu) + bik;
                    if (a.loss == 0) {                         // l2_loss(logit - rate)
                        dl = logit - rk;
                        l = 0.5f * dl * dl;
                    } else {                                   // sigmoid cross-entropy
                        dl = ft_sigmoid(logit) - rk;
                        l = fmaxf(logit, 0.f) - logit * rk + log1pf(__expf(-fabsf(logit)));
                    }
                    if (want_final) a.final_out[r0 + k] = logit;
                }
                dl_s[lane] = dl;
                if (want_loss) ls_s[lane] = l;
                wave_lds_sync();
                // gradient phase: lane = feature, rows in order
                const int cnt = (int)(L - c0 < 64 ? L - c0 : 64);
                for (int kk = 0; kk < cnt; ++kk) {
                    const float d = dl_s[kk];
                    each_feature<NJ>(lane, D, [&](int j, int f) {
                        g[j] += fmaf(d, ft_q<STAGED>(q_s, S, a.Q, it, c0 + kk, f, D, a.item_abs), lp[j]);
                    });
                    gb += a.reg_bias ? d + lbu : d;
                }
                if (want_loss)
                    for (int kk = 0; kk < cnt; ++kk) lsum += ls_s[kk];
                wave_lds_sync();                               // dl_s / ls_s are rewritten by the next pass
            }
            if (a.adam) {
                const AdamC c = {lr * sqrtf(1.f - b2p) / (1.f - b1p), a.b1, a.b2, a.eps, omb1, omb2};
                if (!a.frozen_rows) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) adam_sparse(p[j], m[j], v[j], g[j], c);
                }
                if (!a.frozen_bias) adam_sparse(bu, bm, bv, gb, c);
                b1p *= a.b1;
                b2p *= a.b2;
            } else {
                if (!a.frozen_rows) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) sgd_step(p[j], g[j], lr);
                }
                if (!a.frozen_bias) sgd_step(bu, gb, lr);
            }
            if (want_loss && lane == 0) a.loss_out[kr] = lsum;
            each_feature<NJ>(lane, D, [&](int j, int f) { p_s[f] = p[j]; });
            wave_lds_sync();
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int f = lane + 64 * j;
        if (f < D && !a.frozen_rows) {
            a.P[prow + f] = p[j];
            if (a.adam) { a.Pm[prow + f] = m[j]; a.Pv[prow + f] = v[j]; }
        }
    }
    if (lane == 0 && !a.frozen_bias) {
        a.bu[user] = bu;
        if (a.adam) { a.bum[user] = bm; a.buv[user] = bv; }
    }
}

template <int NJ>
__global__ __launch_bounds__(FT_WAVES * 64) void k_finetune(FtArgs a) {
    extern __shared__ float ft_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t slot = wave_slot();
    if (slot >= a.n_users) return;                     // whole waves only: no block barrier follows
    const int32_t uix = a.order[slot];
    float* w = ft_lds + (size_t)wave * a.wave_floats;
    if (a.row_ptr[uix + 1] - a.row_ptr[uix] <= a.rows_staged)
        ft_user<NJ, true>(a, w, uix, lane);
    else
        ft_user<NJ, false>(a, w, uix, lane);
}

void launch_finetune(const FtArgs& a, const FtPlan& p, hipStream_t s) {
    if (a.n_users < 1) return;
    with_nj(a.D, [&](auto nj) { hipLaunchKernelGGL(k_finetune<decltype(nj)::value>, wave_grid(a.n_users), wave_block(), p.lds_bytes, s, a); });
}

}  // namespace tfr
