// ials.hip - implicit-feedback ALS (Hu, Koren, Volinsky: weighted matrix factorisation) on the GPU, float64, 1 <= d <= 64.
//   R: user x item CSR of strictly positive values.  p_ui = 1 on stored pairs, 0 elsewhere; c_ui = 1 + alpha r_ui on
//   stored pairs, 1 elsewhere.  One half-sweep, for every entity u with list N(u) in CSR order and partner table Y:
//       G   = Y^T Y                                         (k_ials_gram_tiled + k_ials_gram_sum, once per half-sweep)
//       A_u = G + sum_{i in N(u)} w_ui y_i y_i^T + lambda I   w_ui = alpha r_ui = c_ui - 1
//       b_u = sum_{i in N(u)} c_ui y_i                        c_ui = 1 + w_ui
//       x_u = A_u^{-1} b_u                                    (one-wave Cholesky, als_common.h); an empty list gives exactly 0
//   One 256-thread block per entity builds the sums from 32-row tiles of partner rows staged in LDS: thread tid keeps the
//   A entries t = tid + 256 q (row t / d, column t % d) in registers, up to 16 of them, and thread tid < d the b entry tid.
//   Lists longer than the chunk size are cut into chunks: k_ials_partial builds each chunk's sums in its own block, the
//   entity's block adds them in list order.  No atomics anywhere: every sum has a fixed order and the results are
//   bit-identical from run to run, whatever the grid.
//   The Gram, for both this path and the conjugate-gradient one (ials_cg.hip), any d <= 256: cut into row slices whose size
//   depends on n only; one block per (slice, 64 x 64 output tile), thread (tr, tc) = (tid / 16, tid % 16) keeps the 4 x 4
//   entries at rows 4 tr.., columns 4 tc.. of the tile; the slice's rows ascend, 32 at a time through LDS; the slices'
//   partials are added in ascending slice order.  Entries (r, c) and (c, r) add the same products in the same order: G is
//   bitwise symmetric.  Below 24 columns a tile is mostly padding and one block per slice keeps the whole d x d partial
//   (k_ials_gram_narrow): the same sums in the same order, so the same bits; the width alone chooses.
//   Loss: L = sum_u [ x_u^T G x_u + sum_{i in N(u)} (c_ui (1 - s_ui)^2 - s_ui^2) ] + lambda (||X||^2 + trace(G)),
//   s_ui = x_u . y_i, G = Y^T Y - the dense U x I matrix is never formed.
//   Fold-in (tfr_ials_fold_in): the row a half-sweep would give an entity with a list the model does not hold.  The same
//   k_ials_partial / k_ials_fit (k_ials_cg_fit on a conjugate-gradient handle) run on an argument block made of the call's
//   lists, a fold buffer as the own rows, the partner table and G; the call's lists get a chunk plan and partial sums of
//   their own.  G is computed only when the handle's tag (gram_of) does not already name the partner's table.  Three
//   per-element kernels move the rows: k_ials_rows_gather (warm start), k_ials_rows_scatter (into named rows) and
//   k_ials_export_f32 (float32 rows into a caller's device buffer, tfr_ials_export_f32).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <vector>
#include <algorithm>
#include "tfrecomm.h"
#include "devbuf.h"
#include "als_common.h"
#include "ials_model.h"

using tfr::DevBuf;

namespace {

constexpr int IALS_MAXD = 64;
constexpr int IALS_LD = IALS_MAXD + 1;   // LDS row stride: lane r of the Cholesky walks row r, the odd stride spreads the banks
constexpr int IALS_SLOTS = IALS_MAXD * IALS_MAXD / 256;   // A entries per thread at d = 64
constexpr int GRAM_T = 64;               // output tile edge of the Gram
constexpr int GRAM_LD = GRAM_T + 4;      // LDS row stride of a staged tile: 16-byte aligned rows, shifted banks
constexpr int GRAM_NARROW_D = 23;        // widest table of the narrow Gram: measured faster than a mostly empty tile below 24
constexpr int GRAM_NARROW_SLOTS = (GRAM_NARROW_D * GRAM_NARROW_D + 255) / 256;
// IALS_TILE, the Gram slice rule, the handle and IalsArgs: ials_model.h, shared with the conjugate-gradient path (ials_cg.hip)

// Sums over the list entries [lo, hi): acc[q] += sum_k (w_k y_k[r]) y_k[c] for the A entries t = tid + 256 q = r d + c,
// accb += sum_k c_k y_k[tid]; 32-row tiles staged in LDS, k ascending.
__device__ __forceinline__ void ials_accumulate(const IalsArgs& a, int64_t lo, int64_t hi, double (&acc)[IALS_SLOTS], double& accb,
                                                double (*rows)[IALS_LD], double* wk, double* ck) {
    const int tid = threadIdx.x, d = a.d, dd = d * d;
    int rc[IALS_SLOTS];                                            // r << 8 | c of each live slot
#pragma unroll
    for (int q = 0; q < IALS_SLOTS; ++q) {
        const int t = tid + 256 * q;
        rc[q] = (t < dd) ? ((t / d) << 8 | (t % d)) : -1;
    }
    for (int64_t s = lo; s < hi; s += IALS_TILE) {
        const int nk = (int)((hi - s < IALS_TILE) ? hi - s : IALS_TILE);
        for (int t = tid; t < nk * d; t += 256) {
            const int k = t / d, c = t % d;
            rows[k][c] = a.other[(size_t)a.ids[s + k] * d + c];
        }
        if (tid < nk) {
            const double w = a.alpha * a.vals[s + tid];
            wk[tid] = w;
            ck[tid] = 1.0 + w;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < IALS_SLOTS; ++q) {
            if (rc[q] >= 0) {
                const int r = rc[q] >> 8, c = rc[q] & 255;
                double sacc = acc[q];
                for (int k = 0; k < nk; ++k) sacc += (wk[k] * rows[k][r]) * rows[k][c];
                acc[q] = sacc;
            }
        }
        if (tid < d) {
            double sb = accb;
            for (int k = 0; k < nk; ++k) sb += ck[k] * rows[k][tid];
            accb = sb;
        }
        __syncthreads();
    }
}

// one (slice, row tile, column tile): partial[slice][r d + c] for r, c of the tile
__global__ __launch_bounds__(256) void k_ials_gram_tiled(const double* T, int64_t n, int d, int64_t slice_rows, int nt, double* partial) {
    __shared__ double ra[IALS_TILE][GRAM_LD];
    __shared__ double rb[IALS_TILE][GRAM_LD];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int64_t sl = blockIdx.x / (nt * nt);
    const int tile = (int)(blockIdx.x % (nt * nt)), r0 = (tile / nt) * GRAM_T, c0 = (tile % nt) * GRAM_T;
    const int64_t lo = sl * slice_rows, hi = (lo + slice_rows < n) ? lo + slice_rows : n;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int64_t s = lo; s < hi; s += IALS_TILE) {
        const int nk = (int)((hi - s < IALS_TILE) ? hi - s : IALS_TILE);
        for (int t = tid; t < nk * GRAM_T; t += 256) {       // columns past d are staged as 0 and never written out
            const int k = t / GRAM_T, c = t % GRAM_T;
            const double* row = T + (size_t)(s + k) * d;
            ra[k][c] = (r0 + c < d) ? row[r0 + c] : 0.0;
            rb[k][c] = (c0 + c < d) ? row[c0 + c] : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = ra[k][4 * tr + i]; b[i] = rb[k][4 * tc + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
        }
        __syncthreads();
    }
    double* pp = partial + (size_t)sl * d * d;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = r0 + 4 * tr + i, c = c0 + 4 * tc + j;
            if (r < d && c < d) pp[(size_t)r * d + c] = acc[i][j];
        }
}

// one slice of a table of at most GRAM_NARROW_D columns, where a 64 x 64 tile would be mostly padding: thread tid keeps
// the entries t = tid + 256 q = r d + c of the slice's partial; the same products in the same order as the tiled kernel
__global__ __launch_bounds__(256) void k_ials_gram_narrow(const double* T, int64_t n, int d, int64_t slice_rows, double* partial) {
    __shared__ double rows[IALS_TILE][GRAM_NARROW_D + 1];
    const int tid = threadIdx.x, dd = d * d;
    const int64_t sl = blockIdx.x, lo = sl * slice_rows, hi = (lo + slice_rows < n) ? lo + slice_rows : n;
    double acc[GRAM_NARROW_SLOTS];
#pragma unroll
    for (int q = 0; q < GRAM_NARROW_SLOTS; ++q) acc[q] = 0.0;
    for (int64_t s = lo; s < hi; s += IALS_TILE) {
        const int nk = (int)((hi - s < IALS_TILE) ? hi - s : IALS_TILE);
        for (int t = tid; t < nk * d; t += 256) rows[t / d][t % d] = T[(size_t)s * d + t];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GRAM_NARROW_SLOTS; ++q) {
            const int t = tid + 256 * q;
            if (t < dd) {
                const int r = t / d, c = t % d;
                double sacc = acc[q];
                for (int k = 0; k < nk; ++k) sacc += rows[k][r] * rows[k][c];
                acc[q] = sacc;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < GRAM_NARROW_SLOTS; ++q) { const int t = tid + 256 * q; if (t < dd) partial[(size_t)sl * dd + t] = acc[q]; }
}

// G[t] = the slices' partials added in ascending slice order
__global__ __launch_bounds__(256) void k_ials_gram_sum(const double* partial, int64_t n_slices, int d, double* G) {
    const int dd = d * d;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= dd) return;
    double s = 0.0;
    for (int64_t sl = 0; sl < n_slices; ++sl) s += partial[(size_t)sl * dd + t];
    G[t] = s;
}

// partial sums of one chunk of a long list
__global__ __launch_bounds__(256) void k_ials_partial(IalsArgs a, tfr::ChunkArgs ch) {
    __shared__ double rows[IALS_TILE][IALS_LD];
    __shared__ double wk[IALS_TILE], ck[IALS_TILE];
    for (int64_t c = blockIdx.x; c < ch.n; c += gridDim.x) {
        double acc[IALS_SLOTS], accb;
        tfr::zero_slots(acc, accb);
        __syncthreads();
        ials_accumulate(a, ch.lo[c], ch.hi[c], acc, accb, rows, wk, ck);
        tfr::store_chunk_partial(ch, c, a.d, acc, accb);
    }
}

__global__ __launch_bounds__(256) void k_ials_fit(IalsArgs a, tfr::ChunkArgs ch) {
    __shared__ double A[IALS_MAXD][IALS_LD];
    __shared__ double rows[IALS_TILE][IALS_LD];
    __shared__ double wk[IALS_TILE], ck[IALS_TILE];
    __shared__ double bvec[IALS_MAXD], xvec[IALS_MAXD];
    const int tid = threadIdx.x, d = a.d;
    for (int64_t e = blockIdx.x; e < a.n; e += gridDim.x) {
        const int64_t lo = a.ptr[e], hi = a.ptr[e + 1];
        if (lo == hi) {                                            // b = 0: the minimiser is 0
            if (tid < d) a.own[(size_t)e * d + tid] = 0.0;
            continue;
        }
        double acc[IALS_SLOTS], accb;
        tfr::zero_slots(acc, accb);
        __syncthreads();
        const int32_t nch = ch.ccount[e];
        if (nch > 0) tfr::add_chunk_partials(ch, e, nch, d, acc, accb);
        else ials_accumulate(a, lo, hi, acc, accb, rows, wk, ck);
        tfr::slots_to_matrix(acc, d, A, [&](int t, double s, bool diag) { return (a.G[t] + s) + (diag ? a.lambda : 0.0); });
        if (tid < d) bvec[tid] = accb;
        __syncthreads();
        if (tid < 64) tfr::chol_wave_solve<IALS_LD>(A, bvec, xvec, d);
        __syncthreads();
        if (tid < d) a.own[(size_t)e * d + tid] = xvec[tid];
    }
}

// per-user part of the loss: x^T G x + lambda |x|^2 + sum_{i in N(u)} (c (1 - s)^2 - s^2); G = Y^T Y.
// Thread tid < d holds x_tid ((G x)_tid + lambda x_tid), thread tid the list entries lo + tid + 256 j; both go into
// red[tid], summed by a halving tree.
__global__ __launch_bounds__(256) void k_ials_loss_users(IalsArgs a, double* per_user) {
    __shared__ double x[IALS_MAXD];
    __shared__ double red[256];
    const int tid = threadIdx.x, d = a.d;
    for (int64_t e = blockIdx.x; e < a.n; e += gridDim.x) {
        __syncthreads();
        if (tid < d) x[tid] = a.own[(size_t)e * d + tid];
        __syncthreads();
        double part = 0.0;
        if (tid < d) {
            double gx = 0.0;
            for (int c = 0; c < d; ++c) gx += a.G[tid * d + c] * x[c];
            part = x[tid] * (gx + a.lambda * x[tid]);
        }
        const int64_t lo = a.ptr[e], hi = a.ptr[e + 1];
        for (int64_t k = lo + tid; k < hi; k += 256) {
            const double* y = a.other + (size_t)a.ids[k] * d;
            double s = 0.0;
            for (int c = 0; c < d; ++c) s += x[c] * y[c];
            const double cc = 1.0 + a.alpha * a.vals[k];
            const double om = 1.0 - s;
            part += cc * (om * om) - s * s;
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

// loss = (sum of per_user: 256 strided sums, then a halving tree) + lambda trace(G); one block
__global__ __launch_bounds__(256) void k_ials_loss_reduce(const double* per_user, int64_t n, const double* G, int d, double lambda, double* out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int64_t k = tid; k < n; k += 256) part += per_user[k];
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        double tr = 0.0;
        for (int c = 0; c < d; ++c) tr += G[c * d + c];
        out[0] = red[0] + lambda * tr;
    }
}

// Fold-in's three copies, one lane per element t = e d + c, coalesced along the row; the stride loop only covers counts
// past the grid cap.  rows[] holds distinct rows (checked on the host), so no two lanes write one element.
// fold[e] = tab[rows[e]]: the conjugate-gradient warm start
__global__ __launch_bounds__(256) void k_ials_rows_gather(const double* tab, const int32_t* rows, int64_t n, int d, double* fold) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n * d; t += (int64_t)gridDim.x * 256)
        fold[t] = tab[(size_t)rows[t / d] * d + t % d];
}

// tab[rows[e]] = fold[e]
__global__ __launch_bounds__(256) void k_ials_rows_scatter(const double* fold, const int32_t* rows, int64_t n, int d, double* tab) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n * d; t += (int64_t)gridDim.x * 256)
        tab[(size_t)rows[t / d] * d + t % d] = fold[t];
}

// dst[t] = float(src[t]), round to nearest even: overflow gives infinity, float32 subnormals are kept
__global__ __launch_bounds__(256) void k_ials_export_f32(const double* src, int64_t count, float* dst) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256)
        dst[t] = __double2float_rn(src[t]);
}

inline dim3 per_element_grid(int64_t count) { return dim3((unsigned)std::min<int64_t>((count + 255) / 256, 1 << 20)); }

thread_local char g_ials_err[512] = "";
int ials_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_ials_err, sizeof(g_ials_err), fmt, ap);
    va_end(ap);
    return code;
}
#define IALSCHK(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return ials_fail(e_ == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, \
                                               "%s: %s", #expr, hipGetErrorString(e_));                \
    } while (0)

// G = tab[side]^T tab[side] for any d <= 256, queued on the model's stream
hipError_t queue_gram(tfr_ials* m, int side) {
    tfr::ials_launch_gram(m->tab[side].get(), m->n[side], m->d, m->gram_partial.get(), m->G.get(), m->stream);
    m->gram_of = side;
    return hipGetLastError();
}

// every entity of the argument block solved from a.G, queued: the long lists' chunks first (Cholesky path; the
// conjugate-gradient path reads no chunk table).  A half-sweep and a fold-in differ in the block they hand over, not here.
hipError_t queue_fit(tfr_ials* m, const IalsArgs& a, const tfr::ChunkArgs& ch) {
    if (a.cg_steps) return tfr::ials_cg_queue_fit(a, m->stream);
    if (ch.n) hipLaunchKernelGGL(k_ials_partial, dim3((unsigned)std::min<int64_t>(ch.n, 65535)), dim3(256), 0, m->stream, a, ch);
    hipLaunchKernelGGL(k_ials_fit, dim3((unsigned)std::min<int64_t>(a.n, 65535)), dim3(256), 0, m->stream, a, ch);
    return hipGetLastError();
}

// one half-sweep of `side`, queued: the partner table's Gram, then every entity.  It rewrites side's table; the tag names
// the partner's from the Gram on, so a Gram of side's table kept from before is not taken for current afterwards.
hipError_t queue_half(tfr_ials* m, int side) {
    hipError_t e = queue_gram(m, 1 - side);
    if (e != hipSuccess) return e;
    return queue_fit(m, tfr::ials_side_args(m, side), m->chunks[side].args(m->partial));
}

int finish_timed(tfr_ials* m, float* elapsed_ms) {
    (void)hipEventRecord(m->ev1, m->stream);
    IALSCHK(hipStreamSynchronize(m->stream));
    if (elapsed_ms) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->ev0, m->ev1) != hipSuccess) ms = 0.f;
        *elapsed_ms = ms;
    }
    return TFR_OK;
}

}  // namespace

// The Gram launches for any caller (ials_model.h): G = T^T T of T [n, d], d <= 256, through `partial`
void tfr::ials_launch_gram(const double* T, int64_t n, int d, double* partial, double* G, hipStream_t s) {
    const int64_t rows = gram_slice_rows(n), ns = (n + rows - 1) / rows;
    const int nt = (d + GRAM_T - 1) / GRAM_T;
    if (d <= GRAM_NARROW_D)
        hipLaunchKernelGGL(k_ials_gram_narrow, dim3((unsigned)ns), dim3(256), 0, s, T, n, d, rows, partial);
    else
        hipLaunchKernelGGL(k_ials_gram_tiled, dim3((unsigned)(ns * nt * nt)), dim3(256), 0, s, T, n, d, rows, nt, partial);
    hipLaunchKernelGGL(k_ials_gram_sum, dim3((unsigned)((d * d + 255) / 256)), dim3(256), 0, s, partial, ns, d, G);
}

extern "C" {

const char* tfr_ials_last_error(void) { return g_ials_err; }

int tfr_ials_destroy(tfr_ials* m) {
    if (!m) return TFR_OK;
    (void)hipSetDevice(m->device);                       // the buffers are freed with the model's device current
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->ev0) (void)hipEventDestroy(m->ev0);
    if (m->ev1) (void)hipEventDestroy(m->ev1);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return TFR_OK;
}

// both creators: cg_steps = 0 is the Cholesky path (d <= 64), cg_steps > 0 the conjugate-gradient path (d <= 256)
static int ials_create(tfr_ials** out, int64_t n_users, int64_t n_items, int32_t d, double lambda_, double alpha, int32_t cg_steps,
                       int32_t device) {
    const int maxd = cg_steps ? IALS_CG_MAXD : IALS_MAXD;
    if (n_users < 1 || n_items < 1 || n_users > 0x7fffffffLL || n_items > 0x7fffffffLL || d < 1 || d > maxd)
        return ials_fail(TFR_ERR_ARG, "need 1 <= d <= %d and positive int32 table sizes", maxd);
    if (!(lambda_ > 0.0) || !std::isfinite(lambda_)) return ials_fail(TFR_ERR_ARG, "lambda must be positive and finite");
    if (!(alpha >= 0.0) || !std::isfinite(alpha)) return ials_fail(TFR_ERR_ARG, "alpha must be non-negative and finite");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return ials_fail(TFR_ERR_HIP, "no HIP device available - this library has no CPU path");
    if (device < 0 || device >= ndev) return ials_fail(TFR_ERR_ARG, "device %d not in [0,%d)", device, ndev);
    IALSCHK(hipSetDevice(device));
    tfr_ials* m = new (std::nothrow) tfr_ials();
    if (!m) return ials_fail(TFR_ERR_NOMEM, "host allocation failed");
    m->n[0] = n_users; m->n[1] = n_items; m->d = d; m->lambda = lambda_; m->alpha = alpha; m->device = device;
    m->cg_steps = cg_steps;
    const int64_t max_slices = std::max((n_users + gram_slice_rows(n_users) - 1) / gram_slice_rows(n_users),
                                        (n_items + gram_slice_rows(n_items) - 1) / gram_slice_rows(n_items));
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    for (int z = 0; z < 2 && e == hipSuccess; ++z) {
        e = m->tab[z].reserve(m->n[z] * d, m->stream);
        if (e == hipSuccess) e = hipMemsetAsync(m->tab[z], 0, (size_t)m->n[z] * d * 8, m->stream);
    }
    if (e == hipSuccess) e = m->G.reserve((int64_t)d * d, m->stream);
    if (e == hipSuccess) e = m->gram_partial.reserve(max_slices * d * d, m->stream);
    if (e == hipSuccess) e = m->per_user.reserve(n_users, m->stream);
    if (e == hipSuccess) e = m->loss.reserve(1, m->stream);
    if (e == hipSuccess) e = hipEventCreate(&m->ev0);
    if (e == hipSuccess) e = hipEventCreate(&m->ev1);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP;
        tfr_ials_destroy(m);
        return ials_fail(code, "ials_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

int tfr_ials_create(tfr_ials** out, int64_t n_users, int64_t n_items, int32_t d, double lambda_, double alpha, int32_t device) {
    if (!out) return ials_fail(TFR_ERR_ARG, "out is null");
    *out = nullptr;
    return ials_create(out, n_users, n_items, d, lambda_, alpha, 0, device);
}

int tfr_ials_create_cg(tfr_ials** out, int64_t n_users, int64_t n_items, int32_t d, double lambda_, double alpha, int32_t cg_steps,
                       int32_t device) {
    if (!out) return ials_fail(TFR_ERR_ARG, "out is null");
    *out = nullptr;
    if (cg_steps < 1 || cg_steps > 1024) return ials_fail(TFR_ERR_ARG, "need 1 <= cg_steps <= 1024");
    return ials_create(out, n_users, n_items, d, lambda_, alpha, cg_steps, device);
}

int tfr_ials_set(tfr_ials* m, const double* X, const double* Y) {
    if (!m) return ials_fail(TFR_ERR_ARG, "null model");
    IALSCHK(hipSetDevice(m->device));
    if ((X && m->gram_of == 0) || (Y && m->gram_of == 1)) m->gram_of = -1;
    if (X) IALSCHK(hipMemcpyAsync(m->tab[0], X, (size_t)m->n[0] * m->d * 8, hipMemcpyHostToDevice, m->stream));
    if (Y) IALSCHK(hipMemcpyAsync(m->tab[1], Y, (size_t)m->n[1] * m->d * 8, hipMemcpyHostToDevice, m->stream));
    IALSCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_ials_get(tfr_ials* m, double* X, double* Y) {
    if (!m) return ials_fail(TFR_ERR_ARG, "null model");
    IALSCHK(hipSetDevice(m->device));
    if (X) IALSCHK(hipMemcpyAsync(X, m->tab[0], (size_t)m->n[0] * m->d * 8, hipMemcpyDeviceToHost, m->stream));
    if (Y) IALSCHK(hipMemcpyAsync(Y, m->tab[1], (size_t)m->n[1] * m->d * 8, hipMemcpyDeviceToHost, m->stream));
    IALSCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

// The user x item CSR.  Everything is checked and both orientations and their chunk tables are built on the host before
// any device work, so a refused load leaves the model as it was.
int tfr_ials_load(tfr_ials* m, const int64_t* indptr, const int32_t* items, const double* vals, int32_t chunk) {
    if (!m || !indptr) return ials_fail(TFR_ERR_ARG, "load: null model or indptr");
    if (chunk == 0) chunk = 512;
    if (chunk < IALS_TILE || chunk % IALS_TILE) return ials_fail(TFR_ERR_ARG, "load: chunk must be a positive multiple of %d", IALS_TILE);
    const int64_t nu = m->n[0], ni = m->n[1];
    if (indptr[0] != 0) return ials_fail(TFR_ERR_ARG, "load: indptr must start at 0");
    for (int64_t u = 0; u < nu; ++u)
        if (indptr[u + 1] < indptr[u]) return ials_fail(TFR_ERR_ARG, "load: indptr decreases at row %lld", (long long)u);
    const int64_t nnz = indptr[nu];
    if (nnz > 0 && (!items || !vals)) return ials_fail(TFR_ERR_ARG, "load: null items or values");
    for (int64_t u = 0; u < nu; ++u)
        for (int64_t k = indptr[u]; k < indptr[u + 1]; ++k) {
            if (items[k] < 0 || items[k] >= ni) return ials_fail(TFR_ERR_OOB, "load: row %lld: item %d out of range", (long long)u, items[k]);
            if (k > indptr[u] && items[k] <= items[k - 1])
                return ials_fail(TFR_ERR_ARG, "load: row %lld is not strictly increasing", (long long)u);
            if (!(vals[k] > 0.0) || !std::isfinite(vals[k]))
                return ials_fail(TFR_ERR_ARG, "load: row %lld: values must be positive and finite", (long long)u);
        }
    // the item-major orientation: users ascend inside each item's list because the rows are walked in order
    std::vector<int64_t> pu(indptr, indptr + nu + 1), pi((size_t)ni + 1, 0);
    for (int64_t k = 0; k < nnz; ++k) pi[(size_t)items[k] + 1]++;
    for (int64_t i = 0; i < ni; ++i) pi[(size_t)i + 1] += pi[(size_t)i];
    std::vector<int64_t> cur(pi.begin(), pi.end() - 1);
    std::vector<int32_t> iu((size_t)nnz);
    std::vector<double> vi((size_t)nnz);
    for (int64_t u = 0; u < nu; ++u)
        for (int64_t k = indptr[u]; k < indptr[u + 1]; ++k) {
            const int64_t p = cur[(size_t)items[k]]++;
            iu[(size_t)p] = (int32_t)u;
            vi[(size_t)p] = vals[k];
        }
    const tfr::ChunkPlan plan[2] = {tfr::plan_chunks(pu, nu, chunk), tfr::plan_chunks(pi, ni, chunk)};
    const int64_t max_chunks = (int64_t)std::max(plan[0].ent.size(), plan[1].ent.size());

    IALSCHK(hipSetDevice(m->device));
    IALSCHK(hipStreamSynchronize(m->stream));
    m->loaded = false;
    const int64_t cap = std::max<int64_t>(1, nnz);
    for (int z = 0; z < 2; ++z) {
        IALSCHK(m->ptr[z].reserve(m->n[z] + 1, m->stream));
        IALSCHK(m->ids[z].reserve(cap, m->stream));
        IALSCHK(m->vals[z].reserve(cap, m->stream));
        IALSCHK(m->chunks[z].upload(plan[z], m->n[z], m->stream));
    }
    // the chunks' partial sums: the conjugate-gradient path forms no per-row matrix and reads no chunk table
    IALSCHK(m->partial.reserve(m->cg_steps ? 1 : std::max<int64_t>(1, max_chunks * (m->d * m->d + m->d)), m->stream));
    IALSCHK(hipMemcpy(m->ptr[0], pu.data(), pu.size() * 8, hipMemcpyHostToDevice));
    IALSCHK(hipMemcpy(m->ptr[1], pi.data(), pi.size() * 8, hipMemcpyHostToDevice));
    if (nnz) {
        IALSCHK(hipMemcpy(m->ids[0], items, (size_t)nnz * 4, hipMemcpyHostToDevice));
        IALSCHK(hipMemcpy(m->vals[0], vals, (size_t)nnz * 8, hipMemcpyHostToDevice));
        IALSCHK(hipMemcpy(m->ids[1], iu.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
        IALSCHK(hipMemcpy(m->vals[1], vi.data(), (size_t)nnz * 8, hipMemcpyHostToDevice));
    }
    m->loaded = true;
    return TFR_OK;
}

// what a fold-in refuses, all of it on the host: TFR_OK, or the code with the message set
static int fold_in_check(const tfr_ials* m, int32_t side, int64_t n, const int64_t* indptr, const int32_t* ids, const double* vals,
                         int32_t chunk, const int32_t* rows, const double* start) {
    if (side < 0 || side > 1) return ials_fail(TFR_ERR_ARG, "fold_in: side must be 0 or 1");
    if (n < 0 || n > 0x7fffffffLL || !indptr) return ials_fail(TFR_ERR_ARG, "fold_in: need 0 <= n < 2^31 and an indptr");
    if (chunk < IALS_TILE || chunk % IALS_TILE) return ials_fail(TFR_ERR_ARG, "fold_in: chunk must be a positive multiple of %d", IALS_TILE);
    if (start && !m->cg_steps) return ials_fail(TFR_ERR_ARG, "fold_in: a start is for conjugate-gradient handles only");
    if (indptr[0] != 0) return ials_fail(TFR_ERR_ARG, "fold_in: indptr must start at 0");
    for (int64_t e = 0; e < n; ++e)
        if (indptr[e + 1] < indptr[e]) return ials_fail(TFR_ERR_ARG, "fold_in: indptr decreases at list %lld", (long long)e);
    if (indptr[n] > 0 && (!ids || !vals)) return ials_fail(TFR_ERR_ARG, "fold_in: null ids or values");
    const int64_t n_other = m->n[1 - side];
    for (int64_t e = 0; e < n; ++e)
        for (int64_t k = indptr[e]; k < indptr[e + 1]; ++k) {
            if (ids[k] < 0 || ids[k] >= n_other) return ials_fail(TFR_ERR_OOB, "fold_in: list %lld: id %d out of range", (long long)e, ids[k]);
            if (k > indptr[e] && ids[k] <= ids[k - 1])
                return ials_fail(TFR_ERR_ARG, "fold_in: list %lld is not strictly increasing", (long long)e);
            if (!(vals[k] > 0.0) || !std::isfinite(vals[k]))
                return ials_fail(TFR_ERR_ARG, "fold_in: list %lld: values must be positive and finite", (long long)e);
        }
    if (rows) {
        for (int64_t e = 0; e < n; ++e) {
            if (rows[e] < 0) return ials_fail(TFR_ERR_ARG, "fold_in: rows[%lld] is negative", (long long)e);
            if (rows[e] >= m->n[side]) return ials_fail(TFR_ERR_OOB, "fold_in: rows[%lld] = %d out of range", (long long)e, rows[e]);
        }
        std::vector<int32_t> sorted(rows, rows + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return ials_fail(TFR_ERR_ARG, "fold_in: rows repeats a row");
    }
    return TFR_OK;
}

// The rows a half-sweep of `side` would give entities with these lists: the half-sweep's kernels on an argument block whose
// lists are the caller's, whose own rows are the fold buffer and whose partner table and Gram are the model's.  The lists,
// their chunk plan and the chunks' partial sums live in the handle's fold_* members: nothing a sweep reads is touched, except
// side's rows `rows` when they are asked for.
int tfr_ials_fold_in(tfr_ials* m, int32_t side, int64_t n, const int64_t* indptr, const int32_t* ids, const double* vals, int32_t chunk,
                     const int32_t* rows, const double* start, double* out, float* elapsed_ms) {
    if (!m) return ials_fail(TFR_ERR_ARG, "null model");
    if (chunk == 0) chunk = 512;
    const int rc = fold_in_check(m, side, n, indptr, ids, vals, chunk, rows, start);
    if (rc != TFR_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.f;
    if (n == 0) return TFR_OK;
    const int d = m->d;
    const int64_t nnz = indptr[n], cap = std::max<int64_t>(1, nnz);
    tfr::ChunkPlan plan;                                   // the conjugate-gradient path forms no per-row matrix: no chunks
    if (!m->cg_steps) plan = tfr::plan_chunks(std::vector<int64_t>(indptr, indptr + n + 1), n, chunk);

    IALSCHK(hipSetDevice(m->device));
    m->fold_n = -1;
    IALSCHK(m->fold_ptr.reserve(n + 1, m->stream));
    IALSCHK(m->fold_ids.reserve(cap, m->stream));
    IALSCHK(m->fold_vals.reserve(cap, m->stream));
    IALSCHK(m->fold.reserve(n * d, m->stream));
    IALSCHK(hipMemcpy(m->fold_ptr, indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
    if (nnz) {
        IALSCHK(hipMemcpy(m->fold_ids, ids, (size_t)nnz * 4, hipMemcpyHostToDevice));
        IALSCHK(hipMemcpy(m->fold_vals, vals, (size_t)nnz * 8, hipMemcpyHostToDevice));
    }
    if (rows) {
        IALSCHK(m->fold_rows.reserve(n, m->stream));
        IALSCHK(hipMemcpy(m->fold_rows, rows, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    tfr::ChunkArgs ch{};
    if (!m->cg_steps) {
        IALSCHK(m->fold_chunks.upload(plan, n, m->stream));
        IALSCHK(m->fold_partial.reserve(std::max<int64_t>(1, m->fold_chunks.n * (d * d + d)), m->stream));
        ch = m->fold_chunks.args(m->fold_partial);
    }

    (void)hipEventRecord(m->ev0, m->stream);
    if (m->cg_steps) {                                     // the start: the caller's, else the rows as they stand, else 0
        if (start) IALSCHK(hipMemcpyAsync(m->fold, start, (size_t)n * d * 8, hipMemcpyHostToDevice, m->stream));
        else if (rows) hipLaunchKernelGGL(k_ials_rows_gather, per_element_grid(n * d), dim3(256), 0, m->stream, m->tab[side].get(),
                                          m->fold_rows.get(), n, d, m->fold.get());
        else IALSCHK(hipMemsetAsync(m->fold, 0, (size_t)n * d * 8, m->stream));
    }
    if (m->gram_of != 1 - side) IALSCHK(queue_gram(m, 1 - side));
    const IalsArgs a{n, m->fold_ptr.get(), m->fold_ids.get(), m->fold_vals.get(), m->fold.get(), m->tab[1 - side].get(), m->G.get(),
                     m->lambda, m->alpha, d, m->cg_steps};
    IALSCHK(queue_fit(m, a, ch));
    // the scatter writes side's table; the tag names the partner's here, so no Gram of side's table is kept as current
    if (rows) hipLaunchKernelGGL(k_ials_rows_scatter, per_element_grid(n * d), dim3(256), 0, m->stream, m->fold.get(), m->fold_rows.get(), n,
                                 d, m->tab[side].get());
    IALSCHK(hipGetLastError());
    if (out) IALSCHK(hipMemcpyAsync(out, m->fold, (size_t)n * d * 8, hipMemcpyDeviceToHost, m->stream));
    const int done = finish_timed(m, elapsed_ms);
    if (done == TFR_OK) m->fold_n = n;
    return done;
}

// float64 rows as float32, device to device: X (0), Y (1) or the rows of the last fold-in (2)
int tfr_ials_export_f32(tfr_ials* m, int32_t which, int64_t row_lo, int64_t n_rows, void* d_dst) {
    if (!m || which < 0 || which > 2) return ials_fail(TFR_ERR_ARG, "export_f32: null model or bad table");
    if (which == 2 && m->fold_n < 0) return ials_fail(TFR_ERR_STATE, "export_f32: no fold-in yet");
    const int64_t have = which == 2 ? m->fold_n : m->n[which];
    if (row_lo < 0 || n_rows < 0 || row_lo > have || n_rows > have - row_lo)
        return ials_fail(TFR_ERR_ARG, "export_f32: rows [%lld, %lld + %lld) are not inside the %lld there are", (long long)row_lo,
                         (long long)row_lo, (long long)n_rows, (long long)have);
    if (n_rows == 0) return TFR_OK;
    if (!d_dst) return ials_fail(TFR_ERR_ARG, "export_f32: null destination");
    IALSCHK(hipSetDevice(m->device));
    const double* src = (which == 2 ? m->fold.get() : m->tab[which].get()) + (size_t)row_lo * m->d;
    hipLaunchKernelGGL(k_ials_export_f32, per_element_grid(n_rows * m->d), dim3(256), 0, m->stream, src, n_rows * m->d,
                       static_cast<float*>(d_dst));
    IALSCHK(hipGetLastError());
    IALSCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_ials_half(tfr_ials* m, int32_t side, float* elapsed_ms) {
    if (!m || side < 0 || side > 1) return ials_fail(TFR_ERR_ARG, "bad arguments");
    if (!m->loaded) return ials_fail(TFR_ERR_STATE, "no data: call tfr_ials_load first");
    IALSCHK(hipSetDevice(m->device));
    (void)hipEventRecord(m->ev0, m->stream);
    IALSCHK(queue_half(m, side));
    return finish_timed(m, elapsed_ms);
}

int tfr_ials_sweep(tfr_ials* m, int32_t n_iterations, float* elapsed_ms) {
    if (!m || n_iterations < 0) return ials_fail(TFR_ERR_ARG, "bad arguments");
    if (!m->loaded) return ials_fail(TFR_ERR_STATE, "no data: call tfr_ials_load first");
    IALSCHK(hipSetDevice(m->device));
    (void)hipEventRecord(m->ev0, m->stream);
    for (int it = 0; it < n_iterations; ++it) {
        IALSCHK(queue_half(m, 0));
        IALSCHK(queue_half(m, 1));
    }
    return finish_timed(m, elapsed_ms);
}

int tfr_ials_gram(tfr_ials* m, int32_t side, double* G_out) {
    if (!m || side < 0 || side > 1 || !G_out) return ials_fail(TFR_ERR_ARG, "bad arguments");
    IALSCHK(hipSetDevice(m->device));
    IALSCHK(queue_gram(m, side));
    IALSCHK(hipMemcpyAsync(G_out, m->G, (size_t)m->d * m->d * 8, hipMemcpyDeviceToHost, m->stream));
    IALSCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_ials_loss(tfr_ials* m, double* loss_out) {
    if (!m || !loss_out) return ials_fail(TFR_ERR_ARG, "bad arguments");
    if (!m->loaded) return ials_fail(TFR_ERR_STATE, "no data: call tfr_ials_load first");
    IALSCHK(hipSetDevice(m->device));
    IALSCHK(queue_gram(m, 1));
    const IalsArgs a = tfr::ials_side_args(m, 0);
    if (m->cg_steps) IALSCHK(tfr::ials_cg_queue_loss_users(m));
    else hipLaunchKernelGGL(k_ials_loss_users, dim3((unsigned)std::min<int64_t>(a.n, 65535)), dim3(256), 0, m->stream, a, m->per_user.get());
    hipLaunchKernelGGL(k_ials_loss_reduce, dim3(1), dim3(256), 0, m->stream, m->per_user.get(), a.n, m->G.get(), m->d, m->lambda,
                       m->loss.get());
    IALSCHK(hipGetLastError());
    IALSCHK(hipMemcpyAsync(loss_out, m->loss, 8, hipMemcpyDeviceToHost, m->stream));
    IALSCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

}  // extern "C"
