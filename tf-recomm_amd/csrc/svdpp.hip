// svdpp.hip - the SVD++ kernels on gfx950 (wave64): implicit sums, forward, both sides of the step and the Y update.
// DESIGN §14.
//
// One wave owns one unit of work (a piece of N, a user run, an item run, a piece of NT, a Y row); features lie across the
// lanes, NJ = ceil(D / 64) per lane (f = lane + 64 j).  No kernel has a block barrier or an atomic: a row is written by the
// one wave that owns it, and every sum runs in a fixed order:
//   piece of N      sum of Y[j] over its entries, ascending j (the rows of N are strictly increasing)
//   user run        z_u = s_u * (pieces of N(u) added in piece order); then its batch entries in the stable sort's order
//                   (batch order): logit, g, W_u = s_u * sum g_k Q'[i_k], the P / user_bias gradient and their update
//   item run        the Q / item_bias gradient over its entries in batch order, from peff of the pre-update tables
//   piece of NT     sum over its users, ascending, of the active ones' W_u + lam c_u Y[j]
//   Y row           the pieces of its NT column in piece order (pieces without an active user skipped), then the update
// Phase handoffs (peff / W / g -> item and Y kernels, partials -> their owners) are kernel boundaries on the stream.
#include <hip/hip_runtime.h>
#include "svdpp.h"
#include "wave_rows.h"

namespace tfr {

static_assert(PP_WAVES == ROW_WAVES, "wave_slot and wave_grid count ROW_WAVES waves per block");

__device__ __forceinline__ void pp_piece_range(const PpCsr& c, int64_t w, int32_t row, int64_t* lo, int64_t* hi) {
    const int64_t l = c.ip[row] + (w - c.pbeg[row]) * (int64_t)PP_PIECE;
    const int64_t end = c.ip[row + 1];
    *lo = l;
    *hi = l + PP_PIECE < end ? l + PP_PIECE : end;
}

// lazy Adam (touched rows) or SGD on one value.  The one form left unpinned: which product the compiler fuses is its choice
// here, unlike adam_sparse (svd_kernels.h).  Pinning it changes bits, so it waits for a pull request of its own.
__device__ __forceinline__ void pp_update(float* w, float* m, float* v, int64_t x, float g, const PpArgs& a) {
    if (a.opt == 0) {
        const float mm = m[x] * a.b1 + g * (1.f - a.b1);
        const float vv = v[x] * a.b2 + (g * g) * (1.f - a.b2);
        m[x] = mm;
        v[x] = vv;
        w[x] -= (a.alpha * mm) / (sqrtf(vv) + a.eps);
    } else {
        w[x] -= a.lr * g;
    }
}

__global__ void __launch_bounds__(256) k_pp_mark(PpActive a, const int32_t* err) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n || *err) return;
    const int32_t u = a.ks[e];
    if (e == 0 || a.ks[e - 1] != u) {
        a.stamp[u] = a.cur;
        a.run_of[u] = (int32_t)e;
    }
}

template <int NJ>
__global__ void __launch_bounds__(64 * PP_WAVES) k_pp_ypart(PpArgs a) {
    const int64_t w = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    if (w >= a.N.n_pieces || *a.err) return;
    const int32_t u = a.N.prow[w];
    if (a.act.stamp[u] != a.act.cur) return;
    int64_t lo, hi;
    pp_piece_range(a.N, w, u, &lo, &hi);
    float acc[NJ] = {}, sq = 0.f;
    const int32_t jl = lo + lane < hi ? a.N.idx[lo + lane] : 0;    // a piece is at most 64 x 2 entries: two id loads
    const int32_t jl2 = lo + 64 + lane < hi ? a.N.idx[lo + 64 + lane] : 0;
    const int n = (int)(hi - lo);
    for (int t = 0; t < n; ++t) {
        const int32_t item = t < 64 ? __shfl(jl, t, 64) : __shfl(jl2, t - 64, 64);
        const float* y = a.Y + (int64_t)item * D;
        each_feature<NJ>(lane, D, [&](int j, int f) {
            const float x = y[f];
            acc[j] += x;
            sq = fmaf(x, x, sq);
        });
    }
    each_feature<NJ>(lane, D, [&](int j, int f) { a.part[w * D + f] = acc[j]; });
    sq = wave_sum_all(sq);
    if (lane == 0) a.part_sq[w] = sq;
}
static_assert(PP_PIECE <= 128, "k_pp_ypart stages a piece's ids in two loads per lane");

template <int NJ, int MODE>
__global__ void __launch_bounds__(64 * PP_WAVES) k_pp_users(PpArgs a) {
    const int64_t p = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    const int64_t n = a.act.n;
    if (p >= n || *a.err) return;
    const int32_t u = a.act.ks[p];
    if (p > 0 && a.act.ks[p - 1] == u) {                       // not a run head: an empty partial for the finish
        if (MODE == PP_USERS_TRAIN && lane < 4) a.scal[p * 4 + lane] = 0.f;
        return;
    }
    const int64_t q = sorted_run_end(a.act.ks, p, n, lane);
    const int64_t nu = a.N.ip[u + 1] - a.N.ip[u];
    const float s = nu > 0 ? 1.f / sqrtf((float)nu) : 0.f;
    float z[NJ] = {}, pe[NJ] = {}, pu[NJ] = {};
    float ysq = 0.f;
    for (int32_t pc = a.N.pbeg[u]; pc < a.N.pbeg[u + 1]; ++pc) {
        each_feature<NJ>(lane, D, [&](int j, int f) { z[j] += a.part[(int64_t)pc * D + f]; });
        ysq += a.part_sq[pc];
    }
    const int64_t urow = (int64_t)u * D;
    float psq = 0.f;
    each_feature<NJ>(lane, D, [&](int j, int f) {
        pu[j] = a.P[urow + f];
        pe[j] = pu[j] + s * z[j];
        a.peff[urow + f] = pe[j];
        psq = fmaf(pu[j], pu[j], psq);
    });
    if (MODE == PP_USERS_PEFF) return;
    psq = wave_sum_all(psq);
    const float mu = a.mu[0], bu = a.bu[u], lam = a.lam;
    float wacc[NJ] = {}, dp[NJ] = {};
    float loss = 0.f, reg = 0.f, sumg = 0.f, dbu = 0.f;
    for (int64_t e = p; e < q; ++e) {
        const int32_t k = a.act.ps[e];
        const int32_t i = a.it[k];
        const int64_t irow = (int64_t)i * D;
        float qt[NJ] = {}, dot = 0.f, qsq = 0.f;
        each_feature<NJ>(lane, D, [&](int j, int f) {
            const float qq = a.Q[irow + f];
            qt[j] = a.item_abs ? fabsf(qq) : qq;
            dot = fmaf(pe[j], qt[j], dot);
            qsq = fmaf(qq, qq, qsq);
        });
        dot = wave_sum_all(dot);
        const float bi = a.bi[i];
        const float x = ((dot + mu) + bu) + bi;
        if (MODE == PP_USERS_FORWARD) {
            if (lane == 0) a.logits[k] = x;
            continue;
        }
        qsq = wave_sum_all(qsq);
        const float rt = a.r[k];
        float g;
        if (a.loss == 0) {
            const float d = x - rt;
            g = d;
            loss += 0.5f * (d * d);
        } else {
            g = 1.f / (1.f + expf(-x)) - rt;
            loss += fmaxf(x, 0.f) - x * rt + log1pf(expf(-fabsf(x)));
        }
        if (lane == 0) {
            if (a.logits) a.logits[k] = x;
            a.g[k] = g;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            wacc[j] = fmaf(g, qt[j], wacc[j]);
            dp[j] += fmaf(g, qt[j], lam * pu[j]);
        }
        float rk = 0.5f * psq + 0.5f * qsq;
        if (a.reg_bias) {
            rk += 0.5f * (bu * bu) + 0.5f * (bi * bi);
            dbu += g + lam * bu;
        } else {
            dbu += g;
        }
        reg += rk + 0.5f * ysq;
        sumg += g;
    }
    if (MODE == PP_USERS_FORWARD) return;
    each_feature<NJ>(lane, D, [&](int j, int f) { a.W[p * D + f] = s * wacc[j]; });
    if (lane == 0) {
        a.cnt[p] = (int32_t)(q - p);
        a.scal[p * 4 + 0] = loss;
        a.scal[p * 4 + 1] = reg;
        a.scal[p * 4 + 2] = sumg;
        a.scal[p * 4 + 3] = 0.f;
    }
    if (!((a.frozen >> 3) & 1)) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {                               // (pp_update sites keep the plain loop: see pp_update)
            const int f = lane + 64 * j;
            if (f < D) pp_update(a.P, a.Pm, a.Pv, urow + f, dp[j], a);
        }
    }
    if (!((a.frozen >> 1) & 1) && lane == 0) pp_update(a.bu, a.bum, a.buv, u, dbu, a);
}

template <int NJ>
__global__ void __launch_bounds__(64 * PP_WAVES) k_pp_items(PpArgs a) {
    const int64_t p = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    if (p >= a.B || *a.err) return;
    const int32_t i = a.ks_i[p];
    if (p > 0 && a.ks_i[p - 1] == i) return;
    const int64_t q = sorted_run_end(a.ks_i, p, a.B, lane);
    const int64_t irow = (int64_t)i * D;
    const float lam = a.lam, bi = a.bi[i];
    float qr[NJ], sg[NJ], dq[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int f = lane + 64 * j;
        qr[j] = f < D ? a.Q[irow + f] : 0.f;
        sg[j] = a.item_abs ? (qr[j] > 0.f ? 1.f : qr[j] < 0.f ? -1.f : 0.f) : 1.f;
        dq[j] = 0.f;
    }
    float dbi = 0.f;
    for (int64_t e = p; e < q; ++e) {
        const int32_t k = a.ps_i[e];
        const float g = a.g[k];
        const int64_t urow = (int64_t)a.u[k] * D;
        each_feature<NJ>(lane, D, [&](int j, int f) { dq[j] += (g * a.peff[urow + f]) * sg[j] + lam * qr[j]; });
        dbi += a.reg_bias ? g + lam * bi : g;
    }
    if (!((a.frozen >> 4) & 1)) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {                               // (pp_update sites keep the plain loop: see pp_update)
            const int f = lane + 64 * j;
            if (f < D) pp_update(a.Q, a.Qm, a.Qv, irow + f, dq[j], a);
        }
    }
    if (!((a.frozen >> 2) & 1) && lane == 0) pp_update(a.bi, a.bim, a.biv, i, dbi, a);
}

template <int NJ>
__global__ void __launch_bounds__(64 * PP_WAVES) k_pp_ygrad(PpArgs a) {
    const int64_t w = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    if (w >= a.NT.n_pieces || *a.err) return;
    const int32_t item = a.NT.prow[w];
    int64_t lo, hi;
    pp_piece_range(a.NT, w, item, &lo, &hi);
    const int64_t yrow = (int64_t)item * D;
    float y[NJ] = {}, acc[NJ] = {};
    each_feature<NJ>(lane, D, [&](int j, int f) { y[j] = a.Y[yrow + f]; });
    int32_t c = 0;
    for (int64_t base = lo; base < hi; base += 64) {
        const int64_t e = base + lane;
        int32_t run = -1;
        if (e < hi) {
            const int32_t uu = a.NT.idx[e];
            if (a.act.stamp[uu] == a.act.cur) run = a.act.run_of[uu];
        }
        unsigned long long mask = __ballot(run >= 0);
        while (mask) {                                              // ascending lanes = ascending users
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int32_t r = __shfl(run, b, 64);
            const int32_t cr = a.cnt[r];
            const float lc = a.lam * (float)cr;
            each_feature<NJ>(lane, D, [&](int j, int f) { acc[j] += a.W[(int64_t)r * D + f] + lc * y[j]; });
            c += cr;
        }
    }
    each_feature<NJ>(lane, D, [&](int j, int f) { a.gpart[w * D + f] = acc[j]; });
    if (lane == 0) a.gcnt[w] = c;
}

template <int NJ>
__global__ void __launch_bounds__(64 * PP_WAVES) k_pp_yapply(PpArgs a) {
    const int64_t j0 = wave_slot();
    const int lane = threadIdx.x & 63, D = a.D;
    if (j0 >= a.I || *a.err) return;
    float gy[NJ] = {};
    int32_t c = 0;
    for (int32_t pc = a.NT.pbeg[j0]; pc < a.NT.pbeg[j0 + 1]; ++pc) {
        const int32_t cc = a.gcnt[pc];
        if (cc == 0) continue;
        each_feature<NJ>(lane, D, [&](int j, int f) { gy[j] += a.gpart[(int64_t)pc * D + f]; });
        c += cc;
    }
    if (c == 0) return;                                             // untouched row: lazy Adam leaves its slots alone
    const int64_t yrow = j0 * D;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {                               // (pp_update sites keep the plain loop: see pp_update)
        const int f = lane + 64 * j;
        if (f < D) pp_update(a.Y, a.Ym, a.Yv, yrow + f, gy[j], a);
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_pp_mark(const PpActive& a, const int32_t* err, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_pp_mark, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a, err);
}

void launch_pp_ypart(const PpArgs& a, hipStream_t s) {
    if (a.N.n_pieces <= 0) return;
    with_nj(a.D, [&](auto nj) { hipLaunchKernelGGL(k_pp_ypart<decltype(nj)::value>, wave_grid(a.N.n_pieces), wave_block(), 0, s, a); });
}

template <int MODE>
static void launch_users_mode(const PpArgs& a, hipStream_t s) {
    with_nj(a.D, [&](auto nj) { hipLaunchKernelGGL((k_pp_users<decltype(nj)::value, MODE>), wave_grid(a.act.n), wave_block(), 0, s, a); });
}

void launch_pp_users(const PpArgs& a, int mode, hipStream_t s) {
    if (a.act.n <= 0) return;
    if (mode == PP_USERS_PEFF) launch_users_mode<PP_USERS_PEFF>(a, s);
    else if (mode == PP_USERS_FORWARD) launch_users_mode<PP_USERS_FORWARD>(a, s);
    else launch_users_mode<PP_USERS_TRAIN>(a, s);
}

void launch_pp_items(const PpArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    with_nj(a.D, [&](auto nj) { hipLaunchKernelGGL(k_pp_items<decltype(nj)::value>, wave_grid(a.B), wave_block(), 0, s, a); });
}

void launch_pp_y(const PpArgs& a, hipStream_t s) {
    if (((a.frozen >> 5) & 1) || a.NT.n_pieces <= 0) return;   // Y frozen: neither its gradient nor its update
    with_nj(a.D, [&](auto nj) {
        hipLaunchKernelGGL(k_pp_ygrad<decltype(nj)::value>, wave_grid(a.NT.n_pieces), wave_block(), 0, s, a);
        if (a.I > 0) hipLaunchKernelGGL(k_pp_yapply<decltype(nj)::value>, wave_grid(a.I), wave_block(), 0, s, a);
    });
}

}  // namespace tfr
