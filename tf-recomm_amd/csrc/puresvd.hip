// puresvd.hip - PureSVD on gfx950 (tfr_psvd_*): the rank-d truncated SVD of the binary user x item matrix X by a
// randomised subspace iteration, float64 throughout.  r = factors + oversample <= 128 columns.
//   V <- orth(V0);  `iterations` times: W = X V, Z = X^T W, V <- orth(Z);  W = X V, T = W^T W, (lambda, Qe) = eig(T);
//   sigma_j = sqrt(max(lambda_j, 0)), Q = V Qe[:, :factors], P = X Q.
//
// k_psvd_spmm: out[row, :] = the sum over the row's list, in list order, of in[id, :].  One wave per row (or per chunk of
//   a long list); lane l owns the columns 2 l and 2 l + 1, so a gathered row is one 16-byte load per lane where r is
//   even (two 8-byte loads where it is odd: the rows are then not 16-byte aligned).  A whole wave takes a row at every
//   width: the lanes past r / 2 and the column past an odd r are masked, nothing is padded, and the kernel is compiled
//   for even / odd r x row / chunk only (a lane-count parameter would change no instruction).  The wave loads 64 ids at a
//   time, one per lane, and hands them round with readlane; the rows of PSVD_AHEAD entries are loaded before the first of
//   them is added, and the adds stay in list order.  A list of more than PSVD_CHUNK entries is cut (als_common.h
//   plan_chunks): a first launch gives every chunk a wave, which leaves the chunk's sum in `partial`; the row's wave then
//   adds the sums in chunk order.  Adds only, no atomics: the result is the same bits as the NumPy restatement.
// orth(Z) is CholeskyQR twice; a pass is S = Z^T Z (ials.hip's Gram launches), R = chol(S) upper with R^-1 (k_psvd_chol:
//   one workgroup, the lower factor in LDS, inverted in place column by column from the last), V = Z R^-1 (k_ease_gemm).
// k_psvd_jacobi: cyclic Jacobi on T in the LDS of one workgroup.  m = r rounded up to even; a sweep is m - 1 rounds; round
//   t pairs (t, m - 1) and ((t + k) mod (m - 1), (t - k) mod (m - 1)) for k = 1 .. m / 2 - 1 (the circle method; an index
//   r, which only an odd r has, sits out).  The pairs of a round are disjoint: their rotations are computed from T as the
//   round finds it, applied to the rows, then to the columns (and to the columns of the accumulated rotations).  A pair
//   is rotated where |t_pq| > PSVD_ROT_REL * max|T as given|; a sweep without a rotation ends the iteration.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "tfrecomm.h"
#include "dispatch.h"
#include "ials_model.h"
#include "ease.h"
#include "puresvd.h"

namespace {

using tfr::fail;

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int PSVD_SLOT = PSVD_MAX_R * PSVD_MAX_R;       // doubles per r x r matrix of `small`
enum { SM_S = 0, SM_R, SM_RINV, SM_T, SM_QE, SM_ROT, SM_MATS };
constexpr int64_t SM_LAMBDA = (int64_t)SM_MATS * PSVD_SLOT, SM_NORMS = SM_LAMBDA + PSVD_MAX_R, SM_S2 = SM_NORMS + PSVD_MAX_R,
                  SM_TOTAL = SM_S2 + PSVD_MAX_R;

// s0, s1 += in[ids[t], c], in[ids[t], c + 1] over t in [lo, hi), t ascending
template <bool EVEN>
__device__ __forceinline__ void psvd_sum(const int32_t* ids, int64_t lo, int64_t hi, const double* in, int r, int lane, int c, bool on0,
                                         bool on1, double& s0, double& s1) {
    for (int64_t b = lo; b < hi; b += 64) {
        const int nb = (int)(hi - b < 64 ? hi - b : 64);
        const int32_t mine = lane < nb ? ids[b + lane] : 0;
        for (int g = 0; g < nb; g += PSVD_AHEAD) {
            double v0[PSVD_AHEAD], v1[PSVD_AHEAD];
#pragma unroll
            for (int d = 0; d < PSVD_AHEAD; ++d) {
                const bool live = g + d < nb;            // wave-uniform
                const int32_t id = __builtin_amdgcn_readlane(mine, live ? g + d : 0);
                const double* src = in + (int64_t)id * r + c;
                if (EVEN) {
                    f64x2 t = {0.0, 0.0};
                    if (live && on0) t = *reinterpret_cast<const f64x2*>(src);
                    v0[d] = t.x; v1[d] = t.y;
                } else {
                    v0[d] = live && on0 ? src[0] : 0.0;
                    v1[d] = live && on1 ? src[1] : 0.0;
                }
            }
#pragma unroll
            for (int d = 0; d < PSVD_AHEAD; ++d) {
                if (g + d < nb) { s0 += v0[d]; s1 += v1[d]; }
            }
        }
    }
}

// PART: wave w sums chunk w into ch.partial[w]; else wave w writes row w of out, from its list or from its chunks' sums
template <bool EVEN, bool PART>
__global__ __launch_bounds__(64 * PSVD_WAVES) void k_psvd_spmm(PsvdSpmmArgs a, tfr::ChunkArgs ch) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * PSVD_WAVES + (threadIdx.x >> 6);
    if (w >= (PART ? ch.n : a.n)) return;
    const int r = a.r, c = 2 * lane;
    const bool on0 = c < r, on1 = c + 1 < r;
    double s0 = 0.0, s1 = 0.0;
    double* dst;
    if (PART) {
        psvd_sum<EVEN>(a.ids, ch.lo[w], ch.hi[w], a.in, r, lane, c, on0, on1, s0, s1);
        dst = ch.partial + w * r;
    } else {
        const int32_t nch = ch.ccount[w];
        if (nch > 0) {
            const double* pp = ch.partial + (int64_t)ch.cfirst[w] * r + c;
            for (int32_t k = 0; k < nch; ++k, pp += r) {
                if (on0) s0 += pp[0];
                if (on1) s1 += pp[1];
            }
        } else {
            psvd_sum<EVEN>(a.ids, a.ptr[w], a.ptr[w + 1], a.in, r, lane, c, on0, on1, s0, s1);
        }
        dst = a.out + w * r;
    }
    if (EVEN) {
        if (on0) { f64x2 t = {s0, s1}; *reinterpret_cast<f64x2*>(dst + c) = t; }
    } else {
        if (on0) dst[c] = s0;
        if (on1) dst[c + 1] = s1;
    }
}

// S = L L^T in LDS, R = L^T and R^-1 = (L^-1)^T out.  A refused pivot leaves tag * 1024 + column + 1 in the word.
__global__ __launch_bounds__(PSVD_DENSE_THREADS) void k_psvd_chol(PsvdCholArgs a, int32_t tag) {
    extern __shared__ __attribute__((aligned(16))) double psvd_lds[];
    const int tid = threadIdx.x, r = a.r, ld = psvd_ld(r);
    double* L = psvd_lds;
    double* dg = L + r * ld;                             // the diagonal of S as given
    if (*a.err != 0) return;                             // an earlier pass was refused: its word stays
    for (int e = tid; e < r * r; e += PSVD_DENSE_THREADS) {
        const int i = e / r, j = e % r;
        const double v = a.S[e];
        L[i * ld + j] = j <= i ? v : 0.0;
        if (i == j) dg[i] = v;
    }
    __syncthreads();
    for (int c = 0; c < r; ++c) {
        const double p = L[c * ld + c];
        if (!(p > 0.0 && p > PSVD_PIVOT_REL * dg[c]) || !isfinite(p)) {    // the same value in every thread
            if (tid == 0) *a.err = tag * 1024 + c + 1;
            return;
        }
        const double d = sqrt(p);
        __syncthreads();
        for (int i = c + 1 + tid; i < r; i += PSVD_DENSE_THREADS) L[i * ld + c] = L[i * ld + c] / d;
        if (tid == 0) L[c * ld + c] = d;
        __syncthreads();
        const int m = r - c - 1;
        for (int e = tid; e < m * m; e += PSVD_DENSE_THREADS) {
            const int i = c + 1 + e / m, j = c + 1 + e % m;
            if (j <= i) L[i * ld + j] -= L[i * ld + c] * L[j * ld + c];
        }
        __syncthreads();
    }
    for (int e = tid; e < r * r; e += PSVD_DENSE_THREADS) {
        const int i = e / r, j = e % r;
        a.R[e] = j >= i ? L[j * ld + i] : 0.0;
    }
    __syncthreads();
    // W = L^-1 in place, columns from the last: W[i][j] = -(sum over k in (j, i], ascending, of W[i][k] L[k][j]) / L[j][j]
    for (int j = r - 1; j >= 0; --j) {
        const int i = j + 1 + tid;
        const double dj = L[j * ld + j];
        double s = 0.0;
        if (i < r)
            for (int k = j + 1; k <= i; ++k) s += L[i * ld + k] * L[k * ld + j];
        __syncthreads();
        if (i < r) L[i * ld + j] = -s / dj;
        if (tid == 0) L[j * ld + j] = 1.0 / dj;
        __syncthreads();
    }
    for (int e = tid; e < r * r; e += PSVD_DENSE_THREADS) {
        const int i = e / r, j = e % r;
        a.Rinv[e] = j >= i ? L[j * ld + i] : 0.0;
    }
}

__global__ __launch_bounds__(PSVD_DENSE_THREADS) void k_psvd_jacobi(PsvdJacobiArgs a) {
    extern __shared__ __attribute__((aligned(16))) double psvd_lds[];
    constexpr int NT = PSVD_DENSE_THREADS;
    const int tid = threadIdx.x, r = a.r, ld = psvd_ld(r);
    double* T = psvd_lds;
    double* red = T + r * ld;                            // 512 doubles: the reduction, then cc, ss, lam, pp, qq and the count
    double* cc = red;
    double* ss = red + PSVD_MAX_R / 2;
    double* lam = red + PSVD_MAX_R;
    int32_t* pp = reinterpret_cast<int32_t*>(red + 2 * PSVD_MAX_R);
    int32_t* qq = pp + PSVD_MAX_R / 2;
    int32_t& n_rot = qq[PSVD_MAX_R / 2];
    double* Q = a.rot_in_lds ? red + 512 : a.rot;
    const int ldq = a.rot_in_lds ? ld : r;

    double mx = 0.0;
    for (int e = tid; e < r * r; e += NT) {
        const int i = e / r, j = e % r;
        const double v = a.T[e];
        T[i * ld + j] = v;
        Q[i * ldq + j] = i == j ? 1.0 : 0.0;
        mx = fmax(mx, fabs(v));
    }
    red[tid] = mx;
    __syncthreads();
    for (int o = NT / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
    }
    const double thr = PSVD_ROT_REL * red[0];
    __syncthreads();

    const int m = (r + 1) & ~1, half = m / 2;
    int sweeps = 0;
    for (;;) {
        if (sweeps == PSVD_SWEEP_CAP) { sweeps = PSVD_SWEEP_CAP + 1; break; }
        ++sweeps;
        if (tid == 0) n_rot = 0;
        __syncthreads();
        for (int t = 0; t < m - 1; ++t) {
            if (tid < half) {
                const int x = tid == 0 ? t : (t + tid) % (m - 1), y = tid == 0 ? m - 1 : (t - tid + m - 1) % (m - 1);
                const int p = x < y ? x : y, q = x < y ? y : x;
                double c = 1.0, s = 0.0;
                if (q < r) {
                    const double apq = T[p * ld + q];
                    if (fabs(apq) > thr) {
                        const double theta = (T[q * ld + q] - T[p * ld + p]) / (2.0 * apq);
                        const double tn = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(tn * tn + 1.0);
                        s = tn * c;
                        atomicAdd(&n_rot, 1);
                    }
                }
                pp[tid] = p; qq[tid] = q; cc[tid] = c; ss[tid] = s;
            }
            __syncthreads();
            for (int e = tid; e < half * r; e += NT) {   // rows p and q of every pair
                const int k = e / r, col = e % r;
                const double s = ss[k];
                if (s != 0.0) {
                    const double c = cc[k];
                    const int p = pp[k], q = qq[k];
                    const double x = T[p * ld + col], y = T[q * ld + col];
                    T[p * ld + col] = c * x - s * y;
                    T[q * ld + col] = s * x + c * y;
                }
            }
            __syncthreads();
            for (int e = tid; e < half * r; e += NT) {   // columns p and q, of T and of the rotations
                const int k = e / r, row = e % r;
                const double s = ss[k];
                if (s != 0.0) {
                    const double c = cc[k];
                    const int p = pp[k], q = qq[k];
                    double x = T[row * ld + p], y = T[row * ld + q];
                    T[row * ld + p] = c * x - s * y;
                    T[row * ld + q] = s * x + c * y;
                    x = Q[row * ldq + p]; y = Q[row * ldq + q];
                    Q[row * ldq + p] = c * x - s * y;
                    Q[row * ldq + q] = s * x + c * y;
                }
            }
            __syncthreads();
            if (tid < half && ss[tid] != 0.0) {
                T[pp[tid] * ld + qq[tid]] = 0.0;
                T[qq[tid] * ld + pp[tid]] = 0.0;
            }
            __syncthreads();
        }
        if (n_rot == 0) break;
        __syncthreads();                                 // every thread has read the count before thread 0 clears it
    }
    if (tid == 0) *a.sweeps = sweeps;
    if (tid < r) lam[tid] = T[tid * ld + tid];
    __syncthreads();
    if (tid < r) {
        // descending, equal values by column index; the entry of largest magnitude (lowest index on a tie) is positive
        const double mine = lam[tid];
        int rank = 0;
        for (int j = 0; j < r; ++j) rank += (lam[j] > mine || (lam[j] == mine && j < tid)) ? 1 : 0;
        double best = -1.0;
        int at = 0;
        for (int k = 0; k < r; ++k) {
            const double v = fabs(Q[k * ldq + tid]);
            if (v > best) { best = v; at = k; }
        }
        const bool flip = Q[at * ldq + tid] < 0.0;
        a.lambda[rank] = mine;
        for (int k = 0; k < r; ++k) {
            const double v = Q[k * ldq + tid];
            a.Q[k * r + rank] = v == 0.0 ? 0.0 : flip ? -v : v;
        }
    }
}

// norms[j] = || B[:, j] - s2[j] Q[:, j] ||_2: one block per column, thread t the rows t, t + 256, ..., then a halving tree
__global__ __launch_bounds__(256) void k_psvd_resid(const double* B, const double* Q, const double* s2, int64_t n, int f, double* norms) {
    __shared__ double red[256];
    const int tid = threadIdx.x, j = blockIdx.x;
    double part = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
        const double d = B[i * f + j] - s2[j] * Q[i * f + j];
        part += d * d;
    }
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) norms[j] = sqrt(red[0]);
}

// dst[t] = float(src[t]), round to nearest even
__global__ __launch_bounds__(256) void k_psvd_export_f32(const double* src, int64_t count, float* dst) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256) dst[t] = __double2float_rn(src[t]);
}

thread_local tfr::ErrText g_psvd_err;

void launch_spmm(const PsvdSpmmArgs& a, const tfr::ChunkArgs& ch, hipStream_t s) {
    if (a.n < 1) return;
    const dim3 rows((unsigned)((a.n + PSVD_WAVES - 1) / PSVD_WAVES)), parts((unsigned)((ch.n + PSVD_WAVES - 1) / PSVD_WAVES));
    tfr::with_bool(a.r % 2 == 0, [&](auto even) {
        constexpr bool EV = decltype(even)::value;
        if (ch.n) hipLaunchKernelGGL((k_psvd_spmm<EV, true>), parts, dim3(64 * PSVD_WAVES), 0, s, a, ch);
        hipLaunchKernelGGL((k_psvd_spmm<EV, false>), rows, dim3(64 * PSVD_WAVES), 0, s, a, ch);
    });
}

// out = X in (side 0: [n_users, width] from [n_items, width]) or X^T in (side 1), queued
int product(tfr_psvd* m, int side, const double* in, int width, double* out) {
    const tfr::DevChunks& c = m->chunks[side];
    LISTCHK(g_psvd_err, m->partial[side].reserve(std::max<int64_t>(1, c.n * width), m->stream));
    PsvdSpmmArgs a;
    a.ptr = side ? m->pi.get() : m->pu.get();
    a.ids = side ? m->iu.get() : m->items.get();
    a.in = in; a.out = out; a.n = side ? m->n_items : m->n_users; a.r = width;
    launch_spmm(a, c.args(m->partial[side]), m->stream);
    LISTCHK(g_psvd_err, hipGetLastError());
    return TFR_OK;
}

double* mat(tfr_psvd* m, int which) { return m->small.get() + (int64_t)which * PSVD_SLOT; }

// the small matrices, and the Gram partials of blocks of n_a and of n_b rows (psvd_gram_slices: the larger slice count)
int reserve_small(tfr_psvd* m, int64_t n_a, int64_t n_b, int cols) {
    LISTCHK(g_psvd_err, m->small.reserve(SM_TOTAL, m->stream));
    LISTCHK(g_psvd_err, m->gram_partial.reserve(psvd_gram_slices(n_a, n_b) * cols * cols, m->stream));
    return TFR_OK;
}

void gemm(hipStream_t s, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int M, int N, int K) {
    EaseGemmArgs g;
    g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.ta = 0; g.tb = 0; g.sign = 1; g.beta = 0; g.lower = 0; g.kskip = 0;
    ease_launch_gemm(g, s);
}

// one CholeskyQR pass, queued: S, R, R^-1 of src [n, cols], dst = src R^-1
int orth_pass(tfr_psvd* m, int64_t n, int cols, const double* src, double* dst, int tag) {
    hipStream_t s = m->stream;
    tfr::ials_launch_gram(src, n, cols, m->gram_partial, mat(m, SM_S), s);
    LISTCHK(g_psvd_err, hipGetLastError());
    PsvdCholArgs c;
    c.S = mat(m, SM_S); c.R = mat(m, SM_R); c.Rinv = mat(m, SM_RINV); c.err = m->err; c.r = cols;
    hipLaunchKernelGGL(k_psvd_chol, dim3(1), dim3(PSVD_DENSE_THREADS), (size_t)psvd_mat_lds(cols) + 4096, s, c, (int32_t)tag);
    LISTCHK(g_psvd_err, hipGetLastError());
    gemm(s, src, cols, mat(m, SM_RINV), cols, dst, cols, (int)n, cols, cols);
    LISTCHK(g_psvd_err, hipGetLastError());
    return TFR_OK;
}

// orth(buf) in place through tmp, queued; tag names the call in the pivot word
int orth(tfr_psvd* m, int64_t n, int cols, double* buf, double* tmp, int call) {
    if (int rc = orth_pass(m, n, cols, buf, tmp, 2 * call)) return rc;
    return orth_pass(m, n, cols, tmp, buf, 2 * call + 1);
}

int queue_jacobi(tfr_psvd* m, int r) {
    PsvdJacobiArgs j;
    j.T = mat(m, SM_T); j.rot = mat(m, SM_ROT); j.lambda = m->small.get() + SM_LAMBDA; j.Q = mat(m, SM_QE);
    j.sweeps = m->err.get() + 1; j.r = r; j.rot_in_lds = psvd_rot_in_lds(r) ? 1 : 0;
    hipLaunchKernelGGL(k_psvd_jacobi, dim3(1), dim3(PSVD_DENSE_THREADS), (size_t)psvd_jacobi_lds(r), m->stream, j);
    LISTCHK(g_psvd_err, hipGetLastError());
    return TFR_OK;
}

int pivot_error(const char* who, int32_t word) {
    const int tag = (word - 1) / 1024, col = (word - 1) % 1024;
    return fail(g_psvd_err, TFR_ERR_ARG,
                "%s: orthonormalisation %d, pass %d: the pivot of column %d is not positive and finite: the block has fewer "
                "independent columns than r", who, tag / 2, tag % 2 + 1, col);
}

// the dense kernels' dynamic LDS limits, set by every entry that launches them (slim.hip's way: the attribute is per device)
int set_lds_limits() {
    LISTCHK(g_psvd_err, hipFuncSetAttribute(reinterpret_cast<const void*>(k_psvd_chol), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)(psvd_mat_lds(PSVD_MAX_R) + 4096)));
    LISTCHK(g_psvd_err, hipFuncSetAttribute(reinterpret_cast<const void*>(k_psvd_jacobi), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)psvd_jacobi_lds_max()));
    return TFR_OK;
}

bool all_finite(const double* x, int64_t n) {
    for (int64_t e = 0; e < n; ++e)
        if (!std::isfinite(x[e])) return false;
    return true;
}

int upload_chunks(tfr_psvd* m, tfr::DevChunks& dst, const int64_t* indptr, int64_t rows) {
    const std::vector<int64_t> ptr(indptr, indptr + rows + 1);
    const tfr::ChunkPlan p = tfr::plan_chunks(ptr, rows, PSVD_CHUNK);
    LISTCHK(g_psvd_err, dst.upload(p, rows, m->stream));
    return TFR_OK;
}

const char* const NOT_FITTED = "no factors: call tfr_psvd_fit or tfr_psvd_set_factors first";

}  // namespace

extern "C" {

const char* tfr_psvd_last_error(void) { return g_psvd_err.text; }

int tfr_psvd_plan(int64_t n_users, int64_t n_items, int32_t factors, int32_t oversample, int32_t* r, int32_t* lanes, int32_t* chunk,
                  int32_t* ahead, int32_t* sweep_cap, int64_t* lds_bytes, int64_t* device_bytes, int64_t* gram_slices) {
    PsvdPlan p;
    if (!psvd_plan(n_users, n_items, factors, oversample, &p))
        return fail(g_psvd_err, TFR_ERR_ARG, "psvd plan: need positive counts, factors >= 1, oversample >= 0 and r = factors + oversample = %lld <= %d",
                    (long long)factors + oversample, PSVD_MAX_R);
    if (r) *r = p.r;
    if (lanes) *lanes = p.lanes;
    if (chunk) *chunk = p.chunk;
    if (ahead) *ahead = p.ahead;
    if (sweep_cap) *sweep_cap = p.sweep_cap;
    if (lds_bytes) *lds_bytes = p.lds;
    if (device_bytes) *device_bytes = p.device_bytes;
    if (gram_slices) *gram_slices = p.gram_slices;
    return TFR_OK;
}

int tfr_psvd_destroy(tfr_psvd* m) { return m ? tfr::destroy_handle(m, {m->ev[0], m->ev[1]}) : TFR_OK; }

int tfr_psvd_create(tfr_psvd** out, int64_t n_users, int64_t n_items, int32_t factors, int32_t oversample, int32_t device) {
    if (!out) return fail(g_psvd_err, TFR_ERR_ARG, "out is null");
    *out = nullptr;
    if (int rc = tfr::check_counts(g_psvd_err, n_users, n_items)) return rc;
    if (factors < 1 || oversample < 0) return fail(g_psvd_err, TFR_ERR_ARG, "need factors >= 1 and oversample >= 0 (got %d, %d)", factors, oversample);
    const int64_t r = (int64_t)factors + oversample;
    if (r > PSVD_MAX_R) return fail(g_psvd_err, TFR_ERR_ARG, "r = factors + oversample = %lld is past the widest block of %d columns", (long long)r, PSVD_MAX_R);
    tfr_psvd* m = nullptr;
    if (int rc = tfr::create_handle(g_psvd_err, "psvd_create", &m, n_users, n_items, device)) return rc;
    m->factors = factors; m->r = (int32_t)r;
    hipError_t e = m->err.reserve(2, m->stream);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreate(&m->ev[k]);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP;
        tfr_psvd_destroy(m);
        return fail(g_psvd_err, code, "psvd_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

// A load forgets the factors (item_lists.h load_lists); the chunk tables of both orientations follow the lists.
int tfr_psvd_load(tfr_psvd* m, const int64_t* indptr, const int32_t* items) {
    std::vector<int64_t> pi;                             // the items' indptr, as load_lists made it
    if (int rc = tfr::load_lists(g_psvd_err, m, indptr, items, [m] { m->has_ritz = false; m->fold_n = -1; }, &pi)) return rc;
    m->loaded = false;
    if (int rc = upload_chunks(m, m->chunks[0], indptr, m->n_users)) return rc;
    if (int rc = upload_chunks(m, m->chunks[1], pi.data(), m->n_items)) return rc;
    m->loaded = true;
    return TFR_OK;
}

int tfr_psvd_fit(tfr_psvd* m, const double* V0, int32_t iterations, float* ms) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (!m->loaded) return fail(g_psvd_err, TFR_ERR_STATE, "fit: no data: call tfr_psvd_load first");
    if (!V0) return fail(g_psvd_err, TFR_ERR_ARG, "fit: null start block");
    if (iterations < 0) return fail(g_psvd_err, TFR_ERR_ARG, "fit: negative iterations");
    const int64_t U = m->n_users, I = m->n_items;
    const int r = m->r, f = m->factors;
    if (!all_finite(V0, I * r)) return fail(g_psvd_err, TFR_ERR_ARG, "fit: the start block holds a value that is not finite");
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    m->fitted = false;
    m->has_ritz = false;
    m->fold_n = -1;                                      // rows folded in from the earlier factors are not this fit's
    if (int rc = set_lds_limits()) return rc;
    LISTCHK(g_psvd_err, m->bi[0].reserve(I * r, s));
    LISTCHK(g_psvd_err, m->bi[1].reserve(I * r, s));
    LISTCHK(g_psvd_err, m->bu.reserve(U * r, s));
    LISTCHK(g_psvd_err, m->Q.reserve(I * f, s));
    LISTCHK(g_psvd_err, m->P.reserve(U * f, s));
    if (int rc = reserve_small(m, U, I, r)) return rc;
    LISTCHK(g_psvd_err, hipMemcpyAsync(m->bi[0], V0, (size_t)I * r * 8, hipMemcpyHostToDevice, s));
    LISTCHK(g_psvd_err, hipMemsetAsync(m->err, 0, 8, s));

    // the stages alternate: orth, then (products, orth) per iteration, then the eigen step with the last products.  ev[0]
    // and ev[1] bracket one stage at a time, so the stream is drained between stages: a fit is a few dozen launches
    float parts[3] = {0.f, 0.f, 0.f};
    auto timed = [&](int kind, auto&& body) -> int {
        (void)hipEventRecord(m->ev[0], s);
        if (int rc = body()) return rc;
        (void)hipEventRecord(m->ev[1], s);
        LISTCHK(g_psvd_err, hipStreamSynchronize(s));
        float t = 0.f;
        if (hipEventElapsedTime(&t, m->ev[0], m->ev[1]) == hipSuccess) parts[kind] += t;
        if (ms) { ms[0] = parts[0]; ms[1] = parts[1]; ms[2] = parts[2]; }
        if (kind == 1) {                                 // a refused pivot ends the fit here: nothing runs on its block
            int32_t word = 0;
            LISTCHK(g_psvd_err, hipMemcpy(&word, m->err, 4, hipMemcpyDeviceToHost));
            if (word != 0) return pivot_error("fit", word);
        }
        return TFR_OK;
    };
    int cur = 0;
    if (int rc = timed(1, [&] { return orth(m, I, r, m->bi[0], m->bi[1], 0); })) return rc;
    for (int it = 0; it < iterations; ++it) {
        if (int rc = timed(0, [&] {
                if (int rc2 = product(m, 0, m->bi[cur], r, m->bu)) return rc2;
                return product(m, 1, m->bu, r, m->bi[1 - cur]);
            })) return rc;
        cur = 1 - cur;
        if (int rc = timed(1, [&] { return orth(m, I, r, m->bi[cur], m->bi[1 - cur], it + 1); })) return rc;
    }
    if (int rc = timed(2, [&] {
            if (int rc2 = product(m, 0, m->bi[cur], r, m->bu)) return rc2;
            tfr::ials_launch_gram(m->bu, U, r, m->gram_partial, mat(m, SM_T), s);
            LISTCHK(g_psvd_err, hipGetLastError());
            if (int rc2 = queue_jacobi(m, r)) return rc2;
            gemm(s, m->bi[cur], r, mat(m, SM_QE), r, m->Q, f, (int)I, f, r);
            LISTCHK(g_psvd_err, hipGetLastError());
            return product(m, 0, m->Q, f, m->P);
        })) return rc;
    int32_t words[2] = {0, 0};
    std::vector<double> lam((size_t)r);
    LISTCHK(g_psvd_err, hipMemcpy(words, m->err, 8, hipMemcpyDeviceToHost));
    LISTCHK(g_psvd_err, hipMemcpy(lam.data(), m->small.get() + SM_LAMBDA, (size_t)r * 8, hipMemcpyDeviceToHost));
    m->n_sweeps = words[1];
    if (words[1] > PSVD_SWEEP_CAP) return fail(g_psvd_err, TFR_ERR_ARG, "fit: the eigen step still rotated in sweep %d, its last", PSVD_SWEEP_CAP);
    m->ritz = lam;
    m->sigma.assign((size_t)f, 0.0);
    for (int j = 0; j < f; ++j) m->sigma[(size_t)j] = sqrt(std::max(lam[(size_t)j], 0.0));
    m->has_ritz = true;
    m->fitted = true;
    return TFR_OK;
}

int tfr_psvd_get(tfr_psvd* m, int32_t what, double* out) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (what < 0 || what > 3) return fail(g_psvd_err, TFR_ERR_ARG, "get: what must be 0 (sigma), 1 (Q), 2 (P) or 3 (the Ritz values)");
    if (!m->fitted) return fail(g_psvd_err, TFR_ERR_STATE, "get: %s", NOT_FITTED);
    if (what == 3 && !m->has_ritz) return fail(g_psvd_err, TFR_ERR_STATE, "get: no Ritz values: the factors were set, not fitted");
    if (!out) return fail(g_psvd_err, TFR_ERR_ARG, "get: null out");
    if (what == 0) { memcpy(out, m->sigma.data(), m->sigma.size() * 8); return TFR_OK; }
    if (what == 3) { memcpy(out, m->ritz.data(), m->ritz.size() * 8); return TFR_OK; }
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    const int64_t n = (what == 1 ? m->n_items : m->n_users) * m->factors;
    LISTCHK(g_psvd_err, hipMemcpyAsync(out, what == 1 ? m->Q.get() : m->P.get(), (size_t)n * 8, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_psvd_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_psvd_sweeps(tfr_psvd* m, int32_t* out) {
    if (!m || !out) return fail(g_psvd_err, TFR_ERR_ARG, "sweeps: null argument");
    *out = m->n_sweeps;
    return TFR_OK;
}

int tfr_psvd_set_factors(tfr_psvd* m, const double* Q, const double* sigma) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (!Q || !sigma) return fail(g_psvd_err, TFR_ERR_ARG, "set_factors: null array");
    if (!m->loaded) return fail(g_psvd_err, TFR_ERR_STATE, "set_factors: no data: call tfr_psvd_load first (P = X Q needs the lists)");
    const int f = m->factors;
    if (!all_finite(Q, m->n_items * f)) return fail(g_psvd_err, TFR_ERR_ARG, "set_factors: an item factor is not finite");
    for (int j = 0; j < f; ++j)
        if (!(sigma[j] >= 0.0) || !std::isfinite(sigma[j])) return fail(g_psvd_err, TFR_ERR_ARG, "set_factors: singular value %d is negative or not finite", j);
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    m->fitted = false;
    m->has_ritz = false;
    m->fold_n = -1;
    LISTCHK(g_psvd_err, m->Q.reserve(m->n_items * f, s));
    LISTCHK(g_psvd_err, m->P.reserve(m->n_users * f, s));
    LISTCHK(g_psvd_err, hipMemcpyAsync(m->Q, Q, (size_t)m->n_items * f * 8, hipMemcpyHostToDevice, s));
    if (int rc = product(m, 0, m->Q, f, m->P)) return rc;
    LISTCHK(g_psvd_err, hipStreamSynchronize(s));
    m->sigma.assign(sigma, sigma + f);
    m->fitted = true;
    return TFR_OK;
}

int tfr_psvd_residuals(tfr_psvd* m, double* out) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (!m->loaded) return fail(g_psvd_err, TFR_ERR_STATE, "residuals: no data: call tfr_psvd_load first");
    if (!m->fitted) return fail(g_psvd_err, TFR_ERR_STATE, "residuals: %s", NOT_FITTED);
    if (!out) return fail(g_psvd_err, TFR_ERR_ARG, "residuals: null out");
    const int f = m->factors;
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    LISTCHK(g_psvd_err, m->blk_out.reserve(m->n_users * f, s));
    LISTCHK(g_psvd_err, m->blk_in.reserve(m->n_items * f, s));
    LISTCHK(g_psvd_err, m->small.reserve(SM_TOTAL, s));
    std::vector<double> s2((size_t)f);
    for (int j = 0; j < f; ++j) s2[(size_t)j] = m->sigma[(size_t)j] * m->sigma[(size_t)j];
    LISTCHK(g_psvd_err, hipMemcpy(m->small.get() + SM_S2, s2.data(), (size_t)f * 8, hipMemcpyHostToDevice));
    if (int rc = product(m, 0, m->Q, f, m->blk_out)) return rc;
    if (int rc = product(m, 1, m->blk_out, f, m->blk_in)) return rc;
    hipLaunchKernelGGL(k_psvd_resid, dim3((unsigned)f), dim3(256), 0, s, m->blk_in.get(), m->Q.get(), m->small.get() + SM_S2, m->n_items, f,
                       m->small.get() + SM_NORMS);
    LISTCHK(g_psvd_err, hipGetLastError());
    LISTCHK(g_psvd_err, hipMemcpyAsync(out, m->small.get() + SM_NORMS, (size_t)f * 8, hipMemcpyDeviceToHost, s));
    LISTCHK(g_psvd_err, hipStreamSynchronize(s));
    for (int j = 0; j < f; ++j) out[j] = out[j] / s2[0];
    return TFR_OK;
}

int tfr_psvd_multiply(tfr_psvd* m, int32_t side, const double* in, int32_t cols, double* out) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (side < 0 || side > 1) return fail(g_psvd_err, TFR_ERR_ARG, "multiply: side must be 0 (X in) or 1 (X^T in)");
    if (cols < 1 || cols > PSVD_MAX_R) return fail(g_psvd_err, TFR_ERR_ARG, "multiply: cols must be in [1, %d] (got %d)", PSVD_MAX_R, cols);
    if (!in || !out) return fail(g_psvd_err, TFR_ERR_ARG, "multiply: null array");
    if (!m->loaded) return fail(g_psvd_err, TFR_ERR_STATE, "multiply: no data: call tfr_psvd_load first");
    const int64_t n_in = side ? m->n_users : m->n_items, n_out = side ? m->n_items : m->n_users;
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    LISTCHK(g_psvd_err, m->blk_in.reserve(n_in * cols, s));
    LISTCHK(g_psvd_err, m->blk_out.reserve(n_out * cols, s));
    LISTCHK(g_psvd_err, hipMemcpyAsync(m->blk_in, in, (size_t)n_in * cols * 8, hipMemcpyHostToDevice, s));
    if (int rc = product(m, side, m->blk_in, cols, m->blk_out)) return rc;
    LISTCHK(g_psvd_err, hipMemcpyAsync(out, m->blk_out, (size_t)n_out * cols * 8, hipMemcpyDeviceToHost, s));
    LISTCHK(g_psvd_err, hipStreamSynchronize(s));
    return TFR_OK;
}

// The product kernel alone on a zeroed device block, `reps` times, each between two events: what tools/bench_puresvd.py reports
// per call (tfr_psvd_multiply's wall time is mostly its two copies).
int tfr_psvd_product_ms(tfr_psvd* m, int32_t side, int32_t cols, int32_t reps, float* ms_out) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (side < 0 || side > 1) return fail(g_psvd_err, TFR_ERR_ARG, "product_ms: side must be 0 (X in) or 1 (X^T in)");
    if (cols < 1 || cols > PSVD_MAX_R) return fail(g_psvd_err, TFR_ERR_ARG, "product_ms: cols must be in [1, %d] (got %d)", PSVD_MAX_R, cols);
    if (reps < 1 || !ms_out) return fail(g_psvd_err, TFR_ERR_ARG, "product_ms: reps must be positive and ms_out not null");
    if (!m->loaded) return fail(g_psvd_err, TFR_ERR_STATE, "product_ms: no data: call tfr_psvd_load first");
    const int64_t n_in = side ? m->n_users : m->n_items, n_out = side ? m->n_items : m->n_users;
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    LISTCHK(g_psvd_err, m->blk_in.reserve(n_in * cols, s));
    LISTCHK(g_psvd_err, m->blk_out.reserve(n_out * cols, s));
    LISTCHK(g_psvd_err, hipMemsetAsync(m->blk_in, 0, (size_t)n_in * cols * 8, s));
    for (int k = 0; k < reps; ++k) {
        (void)hipEventRecord(m->ev[0], s);
        if (int rc = product(m, side, m->blk_in, cols, m->blk_out)) return rc;
        (void)hipEventRecord(m->ev[1], s);
        LISTCHK(g_psvd_err, hipStreamSynchronize(s));
        if (hipEventElapsedTime(&ms_out[k], m->ev[0], m->ev[1]) != hipSuccess) ms_out[k] = 0.f;
    }
    return TFR_OK;
}

int tfr_psvd_orthonormalise(tfr_psvd* m, int64_t n, double* block, int32_t cols, double* S_out, double* R_out) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (n < 1 || n > 0x7fffffffLL) return fail(g_psvd_err, TFR_ERR_ARG, "orthonormalise: n must be a positive int32");
    if (cols < 1 || cols > PSVD_MAX_R) return fail(g_psvd_err, TFR_ERR_ARG, "orthonormalise: cols must be in [1, %d] (got %d)", PSVD_MAX_R, cols);
    if (!block) return fail(g_psvd_err, TFR_ERR_ARG, "orthonormalise: null block");
    if (!all_finite(block, n * cols)) return fail(g_psvd_err, TFR_ERR_ARG, "orthonormalise: the block holds a value that is not finite");
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    LISTCHK(g_psvd_err, m->blk_in.reserve(n * cols, s));
    LISTCHK(g_psvd_err, m->blk_out.reserve(n * cols, s));
    if (int rc = set_lds_limits()) return rc;
    if (int rc = reserve_small(m, n, n, cols)) return rc;
    LISTCHK(g_psvd_err, hipMemcpyAsync(m->blk_in, block, (size_t)n * cols * 8, hipMemcpyHostToDevice, s));
    LISTCHK(g_psvd_err, hipMemsetAsync(m->err, 0, 8, s));
    const size_t mb = (size_t)cols * cols * 8;
    for (int pass = 0; pass < 2; ++pass) {
        if (int rc = orth_pass(m, n, cols, pass ? m->blk_out : m->blk_in, pass ? m->blk_in : m->blk_out, pass)) return rc;
        if (S_out) LISTCHK(g_psvd_err, hipMemcpyAsync(S_out + (size_t)pass * cols * cols, mat(m, SM_S), mb, hipMemcpyDeviceToHost, s));
        if (R_out) LISTCHK(g_psvd_err, hipMemcpyAsync(R_out + (size_t)pass * cols * cols, mat(m, SM_R), mb, hipMemcpyDeviceToHost, s));
        LISTCHK(g_psvd_err, hipStreamSynchronize(s));    // the next pass overwrites S and R
    }
    int32_t word = 0;
    LISTCHK(g_psvd_err, hipMemcpy(&word, m->err, 4, hipMemcpyDeviceToHost));
    if (word != 0) return pivot_error("orthonormalise", word);
    LISTCHK(g_psvd_err, hipMemcpy(block, m->blk_in, (size_t)n * cols * 8, hipMemcpyDeviceToHost));
    return TFR_OK;
}

int tfr_psvd_eig(tfr_psvd* m, const double* T, int32_t r, double* lambda_out, double* Q_out) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (r < 1 || r > PSVD_MAX_R) return fail(g_psvd_err, TFR_ERR_ARG, "eig: r must be in [1, %d] (got %d)", PSVD_MAX_R, r);
    if (!T || !lambda_out || !Q_out) return fail(g_psvd_err, TFR_ERR_ARG, "eig: null array");
    if (!all_finite(T, (int64_t)r * r)) return fail(g_psvd_err, TFR_ERR_ARG, "eig: the matrix holds a value that is not finite");
    for (int i = 0; i < r; ++i)
        for (int j = 0; j < i; ++j)
            if (T[i * r + j] != T[j * r + i]) return fail(g_psvd_err, TFR_ERR_ARG, "eig: entries (%d, %d) and (%d, %d) differ", i, j, j, i);
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    if (int rc = set_lds_limits()) return rc;
    LISTCHK(g_psvd_err, m->small.reserve(SM_TOTAL, s));
    LISTCHK(g_psvd_err, hipMemcpyAsync(mat(m, SM_T), T, (size_t)r * r * 8, hipMemcpyHostToDevice, s));
    if (int rc = queue_jacobi(m, r)) return rc;
    int32_t sweeps = 0;
    LISTCHK(g_psvd_err, hipMemcpyAsync(&sweeps, m->err.get() + 1, 4, hipMemcpyDeviceToHost, s));
    LISTCHK(g_psvd_err, hipMemcpyAsync(lambda_out, m->small.get() + SM_LAMBDA, (size_t)r * 8, hipMemcpyDeviceToHost, s));
    LISTCHK(g_psvd_err, hipMemcpyAsync(Q_out, mat(m, SM_QE), (size_t)r * r * 8, hipMemcpyDeviceToHost, s));
    LISTCHK(g_psvd_err, hipStreamSynchronize(s));
    m->n_sweeps = sweeps;
    if (sweeps > PSVD_SWEEP_CAP) return fail(g_psvd_err, TFR_ERR_ARG, "eig: the iteration still rotated in sweep %d, its last", PSVD_SWEEP_CAP);
    return TFR_OK;
}

int tfr_psvd_fold_in(tfr_psvd* m, int64_t n, const int64_t* indptr, const int32_t* ids, double* out) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (n < 0 || n > 0x7fffffffLL) return fail(g_psvd_err, TFR_ERR_ARG, "fold_in: n must be a non-negative int32");
    if (!m->fitted) return fail(g_psvd_err, TFR_ERR_STATE, "fold_in: %s", NOT_FITTED);
    if (int rc = tfr::check_csr(g_psvd_err, "fold_in", "list", true, true, indptr, ids, n, m->n_items)) return rc;
    m->fold_n = -1;
    if (n == 0) { m->fold_n = 0; return TFR_OK; }
    const int f = m->factors;
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    LISTCHK(g_psvd_err, hipStreamSynchronize(s));        // the chunk tables are replaced by plain copies
    if (int rc = tfr::stage_csr(g_psvd_err, m, m->q_ptr, m->q_ids, indptr, ids, n)) return rc;
    if (int rc = upload_chunks(m, m->fold_chunks, indptr, n)) return rc;
    LISTCHK(g_psvd_err, m->fold_partial.reserve(std::max<int64_t>(1, m->fold_chunks.n * f), s));
    LISTCHK(g_psvd_err, m->fold.reserve(n * f, s));
    PsvdSpmmArgs a;
    a.ptr = m->q_ptr; a.ids = m->q_ids; a.in = m->Q; a.out = m->fold; a.n = n; a.r = f;
    launch_spmm(a, m->fold_chunks.args(m->fold_partial), s);
    LISTCHK(g_psvd_err, hipGetLastError());
    if (out) LISTCHK(g_psvd_err, hipMemcpyAsync(out, m->fold, (size_t)n * f * 8, hipMemcpyDeviceToHost, s));
    LISTCHK(g_psvd_err, hipStreamSynchronize(s));
    m->fold_n = n;
    return TFR_OK;
}

int tfr_psvd_export_f32(tfr_psvd* m, int32_t which, int64_t row_lo, int64_t n_rows, void* dst_devptr) {
    if (!m) return fail(g_psvd_err, TFR_ERR_ARG, "null model");
    if (which < 0 || which > 2) return fail(g_psvd_err, TFR_ERR_ARG, "export_f32: which must be 0 (Q), 1 (P) or 2 (the last fold-in)");
    if (!m->fitted) return fail(g_psvd_err, TFR_ERR_STATE, "export_f32: %s", NOT_FITTED);
    if (which == 2 && m->fold_n < 0) return fail(g_psvd_err, TFR_ERR_STATE, "export_f32: no fold-in rows: call tfr_psvd_fold_in first");
    const int64_t rows = which == 0 ? m->n_items : which == 1 ? m->n_users : m->fold_n;
    if (row_lo < 0 || n_rows < 0 || row_lo > rows || n_rows > rows - row_lo)
        return fail(g_psvd_err, TFR_ERR_ARG, "export_f32: rows [%lld, %lld + %lld) are not inside the %lld rows", (long long)row_lo, (long long)row_lo,
                    (long long)n_rows, (long long)rows);
    if (n_rows == 0) return TFR_OK;
    if (!dst_devptr) return fail(g_psvd_err, TFR_ERR_ARG, "export_f32: null destination");
    LISTCHK(g_psvd_err, hipSetDevice(m->device));
    const double* src = (which == 0 ? m->Q.get() : which == 1 ? m->P.get() : m->fold.get()) + row_lo * m->factors;
    const int64_t count = n_rows * m->factors;
    hipLaunchKernelGGL(k_psvd_export_f32, dim3((unsigned)std::min<int64_t>((count + 255) / 256, 1 << 20)), dim3(256), 0, m->stream, src, count,
                       static_cast<float*>(dst_devptr));
    LISTCHK(g_psvd_err, hipGetLastError());
    LISTCHK(g_psvd_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

}  // extern "C"
