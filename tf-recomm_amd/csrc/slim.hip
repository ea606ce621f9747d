// slim.hip - SLIM on gfx950 (tfr_slim_*): one non-negative (or signed) elastic-net regression per item column,
// solved by cyclic coordinate descent on the Gram matrix.
//   A = X^T X + beta I in float64 (ease.hip's k_ease_gram with lambda = beta, or a caller's matrix), d = its diagonal.
//   Column j minimises 1/2 w^T A w - a_j^T w + l1 sum|w| with w[j] = 0.  The solver keeps q[i] = a_j[i] - sum over k != i of
//   A[i, k] w[k], so the new value of coordinate i is a function of q[i] alone, and a coordinate that does not change reads
//   no row of A.
//
// k_slim_cd: one workgroup per column, columns past the grid in strides.  q lives in dynamic LDS (8 n bytes after a head of
//   SLIM_HEAD bytes), w in the workgroup's own row of a global scratch.  The workgroup examines SLIM_T consecutive coordinates
//   at once: each thread computes the new value and the change of its coordinate from the q of the moment, a ballot finds the
//   first changed lane of each wave, one LDS exchange the first changed wave.  The coordinates before it are unchanged by
//   their own formula, so the sequential sweep would have passed them without touching q; the one update is applied by all
//   threads (row i of A is column i: contiguous), and the scan resumes behind it.  A window without a change moves on by
//   SLIM_T.  This is the sequential order of include/tfrecomm.h, coordinate for coordinate, and every operation on q is
//   element-wise with the product and the difference rounded separately, so how the threads split k does not enter the bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include "tfrecomm.h"
#include "svd_kernels.h"
#include "slim.h"

// q[k] - (dl * A[i, k]) is two roundings.  The pragma covers the expressions written in this unit; the inline __dmul_rn /
// __dsub_rn of the HIP headers are compiled under the headers' own setting and fuse after inlining, so they are not used.
#pragma clang fp contract(off)

namespace {

using tfr::fail;
using tfr::check_k;
using tfr::window;

__global__ __launch_bounds__(256) void k_slim_diag(const double* A, double* diag, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) diag[i] = A[i * n + i];
}

__global__ __launch_bounds__(SLIM_T) void k_slim_cd(SlimCdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char slim_lds[];
    double* sdl = reinterpret_cast<double*>(slim_lds);                        // [2][SLIM_WAVES]: the first change of each wave
    int* sidx = reinterpret_cast<int*>(slim_lds + 2 * SLIM_WAVES * 8);        // [2][SLIM_WAVES]: its thread, or -1
    double* red = reinterpret_cast<double*>(slim_lds + 2 * SLIM_WAVES * 12);  // [SLIM_WAVES]: the waves' max|w|
    double* q = reinterpret_cast<double*>(slim_lds + SLIM_HEAD);              // [n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = a.n;
    const bool positive = a.positive != 0;
    const double l1 = a.l1;
    double* w = a.w + (int64_t)blockIdx.x * n;
    int par = 0;

    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        const double* aj = a.A + j * n;
        for (int64_t k = tid; k < n; k += SLIM_T) {
            q[k] = aj[k];
            w[k] = 0.0;
        }
        __syncthreads();

        int32_t sweep = 0, updates = 0, conv = 0;
        while (sweep < a.max_iter) {
            ++sweep;
            double dmax = 0.0;
            int64_t base = 0;
            while (base < n) {
                const int64_t i = base + tid;
                double wn = 0.0, dl = 0.0;
                if (i < n && i != j) {
                    const double di = a.diag[i];
                    if (di > 0.0) {
                        const double qi = q[i];
                        const double t = (positive ? qi : fabs(qi)) - l1;
                        if (t > 0.0) wn = positive ? t / di : copysign(t / di, qi);
                        dl = wn - w[i];
                    }
                }
                const unsigned long long mask = __ballot(dl != 0.0);
                if (mask == 0) {
                    if (lane == 0) sidx[par * SLIM_WAVES + wave] = -1;
                } else if (lane == __ffsll(mask) - 1) {
                    sidx[par * SLIM_WAVES + wave] = tid;
                    sdl[par * SLIM_WAVES + wave] = dl;
                }
                __syncthreads();
                int hit = -1;
                double d = 0.0;
#pragma unroll
                for (int v = SLIM_WAVES - 1; v >= 0; --v) {
                    const int t = sidx[par * SLIM_WAVES + v];
                    if (t >= 0) { hit = t; d = sdl[par * SLIM_WAVES + v]; }
                }
                par ^= 1;                                // the next exchange writes the other slots: no barrier after these reads
                if (hit < 0) {
                    base += SLIM_T;
                    continue;
                }
                const int64_t is = base + hit;
                if (tid == hit) w[is] = wn;
                const double* row = a.A + is * n;
                for (int64_t k0 = tid; k0 < n; k0 += SLIM_AHEAD * SLIM_T) {
                    double r[SLIM_AHEAD];                // the row's loads go out together
#pragma unroll
                    for (int u = 0; u < SLIM_AHEAD; ++u) {
                        const int64_t k = k0 + u * SLIM_T;
                        r[u] = k < n ? row[k] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < SLIM_AHEAD; ++u) {
                        const int64_t k = k0 + u * SLIM_T;
                        if (k < n && k != is) {
                            const double p = d * r[u];   // rounded here (this unit is compiled with fp contract off) ...
                            q[k] = q[k] - p;             // ... and here
                        }
                    }
                }
                ++updates;
                dmax = fmax(dmax, fabs(d));
                __syncthreads();                         // q and w[is] are whole before the next window reads them
                base = is + 1;
            }
            double mw = 0.0;
            for (int64_t k = tid; k < n; k += SLIM_T) mw = fmax(mw, fabs(w[k]));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mw = fmax(mw, __shfl_xor(mw, o));
            if (lane == 0) red[wave] = mw;
            __syncthreads();                             // the next write of red comes after a window's barrier
            mw = red[0];
#pragma unroll
            for (int v = 1; v < SLIM_WAVES; ++v) mw = fmax(mw, red[v]);
            if (dmax <= a.tol * mw) {
                conv = 1;
                break;
            }
        }

        bool bad = false;
        for (int64_t k = tid; k < n; k += SLIM_T) {
            const double v = w[k];
            if (v != 0.0) a.W[k * n + j] = __double2float_rn(v);
            bad = bad || !isfinite(v);
        }
        if (bad) *a.err = (int32_t)(j + 1);              // any of the bad columns will do
        if (tid == 0) {
            a.sweeps[j] = sweep;
            a.updates[j] = updates;
            a.converged[j] = conv;
        }
        __syncthreads();                                 // the next column's q and w start after the last reads of this one
    }
}

thread_local tfr::ErrText g_slim_err;

// what the serving drivers of item_lists.h ask of a family: the scoring is EASE's, kernels and plan, under SLIM's own cap
struct SlimServe {
    using Model = tfr_slim;
    using Args = EaseScoreArgs;
    using Plan = EasePlan;
    static bool plan(int which, int64_t n_items, int k, int64_t n_rows, Plan* p) {
        return n_items <= SLIM_MAX_ITEMS && ease_plan(which, n_items, k, n_rows, p);
    }
    static constexpr const char* load_fn = "tfr_slim_load";
    static constexpr const char* not_fitted = "no weights: call tfr_slim_solve or tfr_slim_set_weights first";

    static Args args(const Model* m) {
        Args a = {};
        a.B = m->W;
        return a;
    }

    template <int MODE>
    static void launch(const Args& a, hipStream_t s) { ease_launch_score(MODE, a, s); }
};

int slim_reserve_gram(tfr_slim* m) {
    LISTCHK(g_slim_err, m->A.reserve(m->n_items * m->n_items, m->stream));
    LISTCHK(g_slim_err, m->diag.reserve(m->n_items, m->stream));
    return TFR_OK;
}

void slim_launch_diag(tfr_slim* m) {
    const int64_t blocks = (m->n_items + 255) / 256;
    hipLaunchKernelGGL(k_slim_diag, dim3((unsigned)blocks), dim3(256), 0, m->stream, m->A.get(), m->diag.get(), m->n_items);
}

}  // namespace

extern "C" {

const char* tfr_slim_last_error(void) { return g_slim_err.text; }

int tfr_slim_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t which, int32_t* window_out, int32_t* grid, int64_t* lds_bytes,
                  int32_t* w_in_lds, int64_t* f64_bytes, int64_t* f32_bytes, int32_t* slice_width, int32_t* slices,
                  int64_t* row_chunk, int32_t* look_ahead) {
    if (which < 0 || which > 1) return fail(g_slim_err, TFR_ERR_ARG, "slim plan: which must be 0 (fit) or 1 (scoring)");
    if (n_items < 1 || n_items > SLIM_MAX_ITEMS || n_rows < 0)
        return fail(g_slim_err, TFR_ERR_ARG, "slim plan: n_rows >= 0 and 1 <= n_items <= %lld (the cap: a column's residual must fit the LDS)",
                    (long long)SLIM_MAX_ITEMS);
    if (int rc = check_k(g_slim_err, "slim plan", k)) return rc;
    SlimPlan p;
    EasePlan e;
    if (!slim_plan(n_items, &p) || !ease_plan(which, n_items, k, n_rows, &e))
        return fail(g_slim_err, TFR_ERR_ARG, "slim plan: no plan for k %d over %lld items", k, (long long)n_items);
    if (window_out) *window_out = p.window;
    if (grid) *grid = p.grid;
    if (lds_bytes) *lds_bytes = (int64_t)(which ? std::max(e.lds, tfr::topk_merge_lds(e.slices, k)) : p.lds);
    if (w_in_lds) *w_in_lds = p.w_in_lds;
    if (f64_bytes) *f64_bytes = p.f64_bytes;
    if (f32_bytes) *f32_bytes = p.f32_bytes;
    if (slice_width) *slice_width = e.width;
    if (slices) *slices = e.slices;
    if (row_chunk) *row_chunk = e.chunk;
    if (look_ahead) *look_ahead = e.ahead;
    return TFR_OK;
}

int tfr_slim_destroy(tfr_slim* m) { return m ? tfr::destroy_handle(m, {m->ev0, m->ev1}) : TFR_OK; }

int tfr_slim_create(tfr_slim** out, int64_t n_users, int64_t n_items, double beta, int32_t device) {
    if (!out) return fail(g_slim_err, TFR_ERR_ARG, "out is null");
    *out = nullptr;
    // an item count past the cap is refused with the cap's own message
    if (int rc = tfr::check_counts(g_slim_err, n_users, std::min(n_items, SLIM_MAX_ITEMS))) return rc;
    if (n_items > SLIM_MAX_ITEMS)
        return fail(g_slim_err, TFR_ERR_ARG, "%lld items are past the cap of %lld (a column's float64 residual must fit the LDS of one workgroup)",
                    (long long)n_items, (long long)SLIM_MAX_ITEMS);
    if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(g_slim_err, TFR_ERR_ARG, "beta must be non-negative and finite");
    tfr_slim* m = nullptr;
    if (int rc = tfr::create_handle(g_slim_err, "slim_create", &m, n_users, n_items, device)) return rc;
    m->beta = beta;
    hipError_t e = m->err.reserve(1, m->stream);
    if (e == hipSuccess) e = hipEventCreate(&m->ev0);
    if (e == hipSuccess) e = hipEventCreate(&m->ev1);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP;
        tfr_slim_destroy(m);
        return fail(g_slim_err, code, "slim_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

// A load forgets the Gram matrix, the weights and the statistics (item_lists.h load_lists clears `fitted`).
int tfr_slim_load(tfr_slim* m, const int64_t* indptr, const int32_t* items) {
    return tfr::load_lists(g_slim_err, m, indptr, items, [m] { m->has_gram = false; m->solved = false; m->gram_ms = 0.f; });
}

int tfr_slim_gram(tfr_slim* m) {
    if (!m) return fail(g_slim_err, TFR_ERR_ARG, "null model");
    if (!m->loaded) return fail(g_slim_err, TFR_ERR_STATE, "no data: call tfr_slim_load first");
    EasePlan p;
    if (!ease_plan(0, m->n_items, 1, 0, &p)) return fail(g_slim_err, TFR_ERR_ARG, "gram: no plan");
    LISTCHK(g_slim_err, hipSetDevice(m->device));
    m->has_gram = false;
    if (int rc = slim_reserve_gram(m)) return rc;
    hipStream_t s = m->stream;
    (void)hipEventRecord(m->ev0, s);
    EaseGramArgs a = {};
    a.pu = m->pu; a.items = m->items; a.pi = m->pi; a.iu = m->iu; a.G = m->A; a.n_items = m->n_items; a.lambda = m->beta;
    ease_launch_gram(a, p.slices, s);
    LISTCHK(g_slim_err, hipGetLastError());
    slim_launch_diag(m);
    LISTCHK(g_slim_err, hipGetLastError());
    (void)hipEventRecord(m->ev1, s);
    LISTCHK(g_slim_err, hipStreamSynchronize(s));
    if (hipEventElapsedTime(&m->gram_ms, m->ev0, m->ev1) != hipSuccess) m->gram_ms = 0.f;
    m->has_gram = true;
    return TFR_OK;
}

int tfr_slim_set_gram(tfr_slim* m, const double* A) {
    if (!m) return fail(g_slim_err, TFR_ERR_ARG, "null model");
    if (!A) return fail(g_slim_err, TFR_ERR_ARG, "set_gram: null matrix");
    const int64_t n = m->n_items;
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(A[i * n + j])) return fail(g_slim_err, TFR_ERR_ARG, "set_gram: entry (%lld, %lld) is not finite", (long long)i, (long long)j);
        for (int64_t j = 0; j < i; ++j)
            if (memcmp(&A[i * n + j], &A[j * n + i], 8) != 0)
                return fail(g_slim_err, TFR_ERR_ARG, "set_gram: entries (%lld, %lld) and (%lld, %lld) differ", (long long)i, (long long)j,
                            (long long)j, (long long)i);
    }
    LISTCHK(g_slim_err, hipSetDevice(m->device));
    m->has_gram = false;
    if (int rc = slim_reserve_gram(m)) return rc;
    LISTCHK(g_slim_err, hipMemcpyAsync(m->A, A, (size_t)n * n * 8, hipMemcpyHostToDevice, m->stream));
    slim_launch_diag(m);
    LISTCHK(g_slim_err, hipGetLastError());
    LISTCHK(g_slim_err, hipStreamSynchronize(m->stream));
    m->gram_ms = 0.f;
    m->has_gram = true;
    return TFR_OK;
}

int tfr_slim_get_gram(tfr_slim* m, int64_t row_lo, int64_t n_rows, double* out) {
    if (!m) return fail(g_slim_err, TFR_ERR_ARG, "null model");
    if (!m->has_gram) return fail(g_slim_err, TFR_ERR_STATE, "no Gram matrix: call tfr_slim_gram or tfr_slim_set_gram first");
    if (int rc = window(g_slim_err, m, "get_gram", row_lo, n_rows)) return rc;
    if (n_rows == 0) return TFR_OK;
    if (!out) return fail(g_slim_err, TFR_ERR_ARG, "get_gram: null out");
    LISTCHK(g_slim_err, hipSetDevice(m->device));
    LISTCHK(g_slim_err, hipMemcpyAsync(out, m->A.get() + row_lo * m->n_items, (size_t)n_rows * m->n_items * 8, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_slim_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_slim_solve(tfr_slim* m, double l1, int32_t positive, int32_t max_iter, double tol, float* elapsed_ms) {
    if (!m) return fail(g_slim_err, TFR_ERR_ARG, "null model");
    if (!(l1 >= 0.0) || !std::isfinite(l1)) return fail(g_slim_err, TFR_ERR_ARG, "solve: l1 must be non-negative and finite");
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(g_slim_err, TFR_ERR_ARG, "solve: tol must be non-negative and finite");
    if (max_iter < 1) return fail(g_slim_err, TFR_ERR_ARG, "solve: max_iter must be at least 1 (got %d)", max_iter);
    if (!m->has_gram) return fail(g_slim_err, TFR_ERR_STATE, "no Gram matrix: call tfr_slim_gram or tfr_slim_set_gram first");
    const int64_t n = m->n_items;
    SlimPlan p;
    if (!slim_plan(n, &p)) return fail(g_slim_err, TFR_ERR_ARG, "solve: no plan for %lld items", (long long)n);
    LISTCHK(g_slim_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    m->fitted = false;
    m->solved = false;
    LISTCHK(g_slim_err, m->W.reserve(n * n, s));
    LISTCHK(g_slim_err, m->w.reserve((int64_t)p.grid * n, s));
    LISTCHK(g_slim_err, m->sweeps.reserve(n, s));
    LISTCHK(g_slim_err, m->updates.reserve(n, s));
    LISTCHK(g_slim_err, m->converged.reserve(n, s));
    static size_t attr = 0;                              // static + dynamic LDS must stay within 160 KiB: ask for what is needed
    if (p.lds > attr) {
        LISTCHK(g_slim_err, hipFuncSetAttribute(reinterpret_cast<const void*>(k_slim_cd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        attr = p.lds;
    }
    LISTCHK(g_slim_err, hipMemsetAsync(m->err, 0, 4, s));
    (void)hipEventRecord(m->ev0, s);
    LISTCHK(g_slim_err, hipMemsetAsync(m->W, 0, (size_t)n * n * 4, s));
    SlimCdArgs a = {};
    a.A = m->A; a.diag = m->diag; a.w = m->w; a.W = m->W;
    a.sweeps = m->sweeps; a.updates = m->updates; a.converged = m->converged; a.err = m->err;
    a.n = n; a.l1 = l1; a.tol = tol; a.positive = positive ? 1 : 0; a.max_iter = max_iter;
    hipLaunchKernelGGL(k_slim_cd, dim3((unsigned)p.grid), dim3(SLIM_T), p.lds, s, a);
    LISTCHK(g_slim_err, hipGetLastError());
    (void)hipEventRecord(m->ev1, s);
    int32_t bad = 0;
    LISTCHK(g_slim_err, hipMemcpyAsync(&bad, m->err, 4, hipMemcpyDeviceToHost, s));
    LISTCHK(g_slim_err, hipStreamSynchronize(s));
    if (bad != 0) return fail(g_slim_err, TFR_ERR_ARG, "solve: the weights of column %d left the finite range", bad - 1);
    if (elapsed_ms) {
        elapsed_ms[0] = m->gram_ms;
        if (hipEventElapsedTime(&elapsed_ms[1], m->ev0, m->ev1) != hipSuccess) elapsed_ms[1] = 0.f;
    }
    m->fitted = true;
    m->solved = true;
    return TFR_OK;
}

int tfr_slim_get_stats(tfr_slim* m, int32_t* sweeps, int32_t* updates, int32_t* converged) {
    if (!m) return fail(g_slim_err, TFR_ERR_ARG, "null model");
    if (!m->solved) return fail(g_slim_err, TFR_ERR_STATE, "no statistics: they are those of a tfr_slim_solve");
    LISTCHK(g_slim_err, hipSetDevice(m->device));
    const size_t bytes = (size_t)m->n_items * 4;
    if (sweeps) LISTCHK(g_slim_err, hipMemcpyAsync(sweeps, m->sweeps, bytes, hipMemcpyDeviceToHost, m->stream));
    if (updates) LISTCHK(g_slim_err, hipMemcpyAsync(updates, m->updates, bytes, hipMemcpyDeviceToHost, m->stream));
    if (converged) LISTCHK(g_slim_err, hipMemcpyAsync(converged, m->converged, bytes, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_slim_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_slim_get_weights(tfr_slim* m, int64_t row_lo, int64_t n_rows, float* out) {
    if (!m) return fail(g_slim_err, TFR_ERR_ARG, "null model");
    if (!m->fitted) return fail(g_slim_err, TFR_ERR_STATE, "no weights: call tfr_slim_solve or tfr_slim_set_weights first");
    if (int rc = window(g_slim_err, m, "get_weights", row_lo, n_rows)) return rc;
    if (n_rows == 0) return TFR_OK;
    if (!out) return fail(g_slim_err, TFR_ERR_ARG, "get_weights: null out");
    LISTCHK(g_slim_err, hipSetDevice(m->device));
    LISTCHK(g_slim_err, hipMemcpyAsync(out, m->W.get() + row_lo * m->n_items, (size_t)n_rows * m->n_items * 4, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_slim_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

// Rows [row_lo, row_lo + n_rows) of W from a host array, under tfr_ease_set_weights' rules: checked before any device work; a
// handle without weights takes all rows at once, which makes it fitted; a fitted one takes any window.  The statistics of
// an earlier solve no longer describe the weights and are forgotten.
int tfr_slim_set_weights(tfr_slim* m, int64_t row_lo, int64_t n_rows, const float* in) {
    if (!m) return fail(g_slim_err, TFR_ERR_ARG, "null model");
    if (int rc = window(g_slim_err, m, "set_weights", row_lo, n_rows)) return rc;
    if (n_rows > 0 && !in) return fail(g_slim_err, TFR_ERR_ARG, "set_weights: null weights");
    const int64_t n = m->n_items;
    for (int64_t e = 0; e < n_rows * n; ++e)
        if (!std::isfinite(in[e]))
            return fail(g_slim_err, TFR_ERR_ARG, "set_weights: the weight (%lld, %lld) is not finite", (long long)(row_lo + e / n), (long long)(e % n));
    if (!m->fitted && n_rows != n) return fail(g_slim_err, TFR_ERR_STATE, "set_weights: a model without weights takes all %lld rows at once", (long long)n);
    if (n_rows == 0) return TFR_OK;
    LISTCHK(g_slim_err, hipSetDevice(m->device));
    LISTCHK(g_slim_err, m->W.reserve(n * n, m->stream));
    LISTCHK(g_slim_err, hipMemcpyAsync(m->W.get() + row_lo * n, in, (size_t)n_rows * n * 4, hipMemcpyHostToDevice, m->stream));
    LISTCHK(g_slim_err, hipStreamSynchronize(m->stream));
    m->fitted = true;
    m->solved = false;
    return TFR_OK;
}

int tfr_slim_topk(tfr_slim* m, const int32_t* users, int64_t n, int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                  int32_t* items_out, float* scores_out) {
    return tfr::topk_users<SlimServe>(g_slim_err, m, users, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_slim_topk_lists(tfr_slim* m, const int64_t* list_indptr, const int32_t* list_items, int64_t n, int32_t k,
                        const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    return tfr::topk_lists<SlimServe>(g_slim_err, m, list_indptr, list_items, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_slim_rank_items(tfr_slim* m, const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
                        const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    return tfr::rank_users<SlimServe>(g_slim_err, m, users, n, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

}  // extern "C"
