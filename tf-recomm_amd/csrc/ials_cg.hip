// ials_cg.hip - the conjugate-gradient half-sweep of the implicit ALS (include/tfrecomm.h states the solver), float64,
// 1 <= d <= 256.  No per-row matrix is formed: per row and per step the solver multiplies by G = Y^T Y and walks the row's
// list once.  G comes from the one Gram of both paths (ials.hip) and is bitwise symmetric.
//   k_ials_cg_fit<NC>   one 256-thread block per entity, grid-stride, empty entities included (they get exactly 0).
//       x, r, p, Ap live in LDS.  A pass over a vector v (x for the first residual, p in a step) gives every wave the list
//       entries k = wave, wave + 4, ... and the rows c' = wave, wave + 4, ... of G: lane l holds the components l + 64 j,
//       j < NC = ceil(d / 64), of the gathered row y_k and of its two running sums; y_k . v is the lane's own NC products
//       (j ascending) and then a butterfly over the wave (xor 32, 16, .. 1: every lane ends with the same bits); the
//       axpys stay in registers.  The four waves' partial vectors are added in wave order by thread c = component c.
//       r . r and p . Ap: thread c's product, a butterfly per wave, the four waves' sums added in wave order.
//   k_ials_loss_users_wide   the per-user part of the loss with x[256] staged: thread c < d the head term
//       x_c ((G x)_c + lambda x_c), wave w the list entries w, w + 4, ... (lane 0 adds their terms in that order after its
//       own head term), then the halving tree over the 256 threads.
// No atomics, no inter-block waits, no sum whose order depends on the grid; every loop is bounded by cg_steps, d or the
// list length.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include "ials_model.h"

namespace {

constexpr int CG_AHEAD = 4;                  // list entries a wave gathers ahead in the fit kernel's pass

// the sum over the wave, in every lane: xor 32, 16, 8, 4, 2, 1
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a . b over the block's components: thread c's product (0 past d), a butterfly per wave, the waves' sums in wave order.
// Two barriers; every thread returns the same bits.
__device__ __forceinline__ double block_dot(const double* a, const double* b, int d, double* wred) {
    const int tid = threadIdx.x;
    const double s = wave_sum(tid < d ? a[tid] * b[tid] : 0.0);
    __syncthreads();                                               // wred's last readers are done
    if ((tid & 63) == 0) wred[tid >> 6] = s;
    __syncthreads();
    return ((wred[0] + wred[1]) + wred[2]) + wred[3];
}

// One pass over v (in LDS).  FIRST: lst = sum_k (c_k - w_k (y_k . v)) y_k; otherwise lst = sum_k w_k (y_k . v) y_k;
// gv = G v.  Wave w takes k = lo + w, lo + w + 4, ... and the rows c' = w, w + 4, ... of G; its two partial vectors go to
// pl[w] and pg[w].  The caller's barrier makes them visible.
template <int NC, bool FIRST>
__device__ __forceinline__ void cg_pass(const IalsArgs& a, int64_t lo, int64_t hi, const double* v, double (*pl)[IALS_CG_MAXD],
                                        double (*pg)[IALS_CG_MAXD]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = a.d;
    double vr[NC], al[NC], ag[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = lane + 64 * j;
        vr[j] = (c < d) ? v[c] : 0.0;
        al[j] = 0.0;
        ag[j] = 0.0;
    }
    int64_t k = lo + wave;
    for (; k + 4 * (CG_AHEAD - 1) < hi; k += 4 * CG_AHEAD) {       // CG_AHEAD entries' gathers in flight; the sums keep the order of k
        double yr[CG_AHEAD][NC], w[CG_AHEAD], s[CG_AHEAD];
#pragma unroll
        for (int u = 0; u < CG_AHEAD; ++u) {
            const double* y = a.other + (size_t)a.ids[k + 4 * u] * d;
            w[u] = a.alpha * a.vals[k + 4 * u];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int c = lane + 64 * j;
                yr[u][j] = (c < d) ? y[c] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < CG_AHEAD; ++u) {
            s[u] = 0.0;
#pragma unroll
            for (int j = 0; j < NC; ++j) s[u] += yr[u][j] * vr[j];
            s[u] = wave_sum(s[u]);
        }
#pragma unroll
        for (int u = 0; u < CG_AHEAD; ++u) {
            const double coef = FIRST ? (1.0 + w[u]) - w[u] * s[u] : w[u] * s[u];
#pragma unroll
            for (int j = 0; j < NC; ++j) al[j] += coef * yr[u][j];
        }
    }
    for (; k < hi; k += 4) {
        const double* y = a.other + (size_t)a.ids[k] * d;
        const double w = a.alpha * a.vals[k];
        double yr[NC], s = 0.0;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            yr[j] = (c < d) ? y[c] : 0.0;
            s += yr[j] * vr[j];
        }
        s = wave_sum(s);
        const double coef = FIRST ? (1.0 + w) - w * s : w * s;
#pragma unroll
        for (int j = 0; j < NC; ++j) al[j] += coef * yr[j];
    }
    for (int cp = wave; cp < d; cp += 4) {                         // G is symmetric: row cp is column cp, read along the lanes
        const double* g = a.G + (size_t)cp * d;
        const double vc = v[cp];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int c = lane + 64 * j;
            if (c < d) ag[j] += g[c] * vc;
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = lane + 64 * j;
        if (c < d) { pl[wave][c] = al[j]; pg[wave][c] = ag[j]; }
    }
}

template <int NC>
__global__ __launch_bounds__(256) void k_ials_cg_fit(IalsArgs a) {
    __shared__ double xs[IALS_CG_MAXD], rs_[IALS_CG_MAXD], ps[IALS_CG_MAXD], aps[IALS_CG_MAXD];
    __shared__ double pl[4][IALS_CG_MAXD], pg[4][IALS_CG_MAXD];
    __shared__ double wred[4];
    const int tid = threadIdx.x, d = a.d;
    for (int64_t e = blockIdx.x; e < a.n; e += gridDim.x) {
        const int64_t lo = a.ptr[e], hi = a.ptr[e + 1];
        if (lo == hi) {                                            // b = 0: the minimiser is 0
            if (tid < d) a.own[(size_t)e * d + tid] = 0.0;
            continue;
        }
        __syncthreads();                                           // the last entity's readers are done
        if (tid < d) xs[tid] = a.own[(size_t)e * d + tid];
        __syncthreads();
        cg_pass<NC, true>(a, lo, hi, xs, pl, pg);
        __syncthreads();
        if (tid < d) {
            const double ls = ((pl[0][tid] + pl[1][tid]) + pl[2][tid]) + pl[3][tid];
            const double gs = ((pg[0][tid] + pg[1][tid]) + pg[2][tid]) + pg[3][tid];
            const double r = ls - (gs + a.lambda * xs[tid]);
            rs_[tid] = r;
            ps[tid] = r;
        }
        double rs = block_dot(rs_, rs_, d, wred);                  // its barriers publish rs_ and ps too
        const double stop = 0x1p-104 * rs;
        for (int step = 0; step < a.cg_steps && rs > stop; ++step) {
            cg_pass<NC, false>(a, lo, hi, ps, pl, pg);
            __syncthreads();
            if (tid < d) {
                const double ls = ((pl[0][tid] + pl[1][tid]) + pl[2][tid]) + pl[3][tid];
                const double gs = ((pg[0][tid] + pg[1][tid]) + pg[2][tid]) + pg[3][tid];
                aps[tid] = (gs + a.lambda * ps[tid]) + ls;
            }
            const double pap = block_dot(ps, aps, d, wred);        // its first barrier publishes aps
            const double al = rs / pap;
            if (tid < d) {                                         // thread c owns component c of x, r, p
                xs[tid] += al * ps[tid];
                rs_[tid] -= al * aps[tid];
            }
            const double rn = block_dot(rs_, rs_, d, wred);
            if (tid < d) ps[tid] = rs_[tid] + (rn / rs) * ps[tid];
            rs = rn;
            __syncthreads();                                       // p is whole before the next pass reads it
        }
        if (tid < d) a.own[(size_t)e * d + tid] = xs[tid];
    }
}

// per-user part of the loss: x^T G x + lambda |x|^2 + sum_{i in N(u)} (c (1 - s)^2 - s^2); G = Y^T Y
template <int NC>
__global__ __launch_bounds__(256) void k_ials_loss_users_wide(IalsArgs a, double* per_user) {
    __shared__ double x[IALS_CG_MAXD];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = a.d;
    for (int64_t e = blockIdx.x; e < a.n; e += gridDim.x) {
        __syncthreads();
        if (tid < d) x[tid] = a.own[(size_t)e * d + tid];
        __syncthreads();
        double part = 0.0;
        if (tid < d) {
            double gx = 0.0;
            for (int c = 0; c < d; ++c) gx += a.G[(size_t)c * d + tid] * x[c];    // column tid = row tid, read along the lanes
            part = x[tid] * (gx + a.lambda * x[tid]);
        }
        double xr[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) xr[j] = (lane + 64 * j < d) ? x[lane + 64 * j] : 0.0;
        const int64_t lo = a.ptr[e], hi = a.ptr[e + 1];
        for (int64_t k = lo + wave; k < hi; k += 4) {
            const double* y = a.other + (size_t)a.ids[k] * d;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int c = lane + 64 * j;
                s += ((c < d) ? y[c] : 0.0) * xr[j];
            }
            s = wave_sum(s);
            const double cc = 1.0 + a.alpha * a.vals[k];
            const double om = 1.0 - s;
            if (lane == 0) part += cc * (om * om) - s * s;
        }
        red[tid] = part;
        __syncthreads();
        for (int o = 128; o >= 1; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) per_user[e] = red[0];
    }
}

// calls launch(std::integral_constant<int, NC>) for NC = ceil(d / 64), the components per lane, with the grid of one block
// per entity
template <class Launch>
hipError_t with_nc(const IalsArgs& a, Launch launch) {
    const dim3 grid((unsigned)std::min<int64_t>(a.n, 65535));
    switch ((a.d + 63) / 64) {
        case 1: launch(std::integral_constant<int, 1>(), grid); break;
        case 2: launch(std::integral_constant<int, 2>(), grid); break;
        case 3: launch(std::integral_constant<int, 3>(), grid); break;
        default: launch(std::integral_constant<int, 4>(), grid); break;
    }
    return hipGetLastError();
}

}  // namespace

namespace tfr {

hipError_t ials_cg_queue_fit(const IalsArgs& a, hipStream_t s) {
    return with_nc(a, [&](auto nc, dim3 grid) { hipLaunchKernelGGL(k_ials_cg_fit<decltype(nc)::value>, grid, dim3(256), 0, s, a); });
}

hipError_t ials_cg_queue_loss_users(tfr_ials* m) {
    const IalsArgs a = ials_side_args(m, 0);
    return with_nc(a, [&](auto nc, dim3 grid) {
        hipLaunchKernelGGL(k_ials_loss_users_wide<decltype(nc)::value>, grid, dim3(256), 0, m->stream, a, m->per_user.get());
    });
}

}  // namespace tfr
