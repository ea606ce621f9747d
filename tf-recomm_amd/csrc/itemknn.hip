// itemknn.hip - item-based nearest neighbours on gfx950 (tfr_knn_*): a sparse x sparse product.
//   X: the binary user x item matrix (a CSR pattern, rows strictly increasing).  n_i = users of item i, c_ij = users with
//   both i and j.  sim(i, j) is a float64 function of (c_ij, n_i, n_j) rounded once to float32 (knn_sim).  The neighbours
//   of i are the K items j != i, c_ij > 0 with the largest key (score_tile.h topk_key: score descending, id ascending).
//   score(u, j) = sum over i in N(u), ascending, of sim(i, j) where j is among i's K neighbours: a float32 chain from +0.
//
// k_knn_cooc: one block per (item i, slice of KNN_W_FIT columns).  uint32 counters of the slice in LDS.  Each wave takes 64
//   users of N(i) at a time: lane l loads user l's row bounds and finds the part of the row inside the slice (two binary
//   searches), so 64 dependent chains run side by side; then the wave walks the 64 parts, lanes striding over the columns,
//   and adds 1 with an LDS integer atomic.  Integer adds commute: the counts are exact whatever the order.  Then each wave
//   scans a quarter of the counters 64 at a time, forms the keys and appends those above its running K-th key to a queue of
//   its own by ballot and prefix count; a queue that cannot take 64 more is sorted (score_tile.h wave_sort_desc) and cut
//   to K.  Wave 0 then takes in the other three queues and writes part[row, slice]; launch_topk_merge joins the slices.
//   Keys within a row are distinct, so neither the fill order nor the split over waves reaches the result.
// k_knn_score<R, MODE>: one wave per (query, slice of KNN_W_SCORE columns) with a float32 accumulator of its own in LDS,
//   four waves per block, no block barrier.  For the query's items i ascending, KNN_SCORE_AHEAD at a time: the lanes load
//   the items' neighbour rows (coalesced, R rounds of 64 slots), then add them item by item with plain LDS read-add-write.
//   One item's columns are distinct and one wave's LDS operations execute in order: the chain has the stated order.
//   Excluded columns are then overwritten with NaN, which no sum of finite scores gives.  MODE 0 (top-K): scan, keys, queue,
//   part[query, slice].  MODE 1 (ranking): the targets inside the slice get their key.  MODE 2: lane t counts the slots of
//   the slice whose key beats target t's; the slices' counts meet in an integer atomic.
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
#include "svd_kernels.h"
#include "score_tile.h"
#include "topk.h"
#include "itemknn.h"

namespace {

using tfr::topk_key;
using tfr::wave_lds_sync;

enum { KNN_COSINE = 0, KNN_JACCARD = 1, KNN_COUNT = 2 };

// float64 with IEEE operations from the three integers, rounded once to float32
__device__ __forceinline__ float knn_sim(int metric, uint32_t c, int64_t ni, int64_t nj, double shrink) {
    double s;
    if (metric == KNN_COSINE) s = (double)c / (sqrt((double)ni * (double)nj) + shrink);
    else if (metric == KNN_JACCARD) s = (double)c / ((double)(ni + nj - (int64_t)c) + shrink);
    else s = (double)c;
    return __double2float_rn(s);
}

// first position in the increasing x[lo, hi) whose value is not below v
__device__ __forceinline__ int64_t knn_lower_bound(const int32_t* x, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)x[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <int CAP>
__global__ __launch_bounds__(256) void k_knn_cooc(KnnFitArgs a) {
    __shared__ uint32_t counts[KNN_W_FIT];
    __shared__ uint64_t queue[KNN_WAVES][CAP];
    __shared__ int32_t wcnt[KNN_WAVES];
    static_assert(sizeof(counts) + sizeof(queue) + sizeof(wcnt) == knn_fit_lds(CAP), "knn_plan reports another LDS size");
    static_assert(CAP >= KNN_KMAX + 64 || CAP == 256, "a queue must hold K plus one append");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.y, K = a.K;
    const int64_t lo = (int64_t)slice * KNN_W_FIT;
    const int width = (int)(a.n_items - lo < KNN_W_FIT ? a.n_items - lo : KNN_W_FIT);
    uint64_t* q = queue[wave];

    for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const int64_t i = a.row_lo + r;
        const int64_t p0 = a.pi[i], p1 = a.pi[i + 1];
        for (int t = tid; t < width; t += 256) counts[t] = 0;
        __syncthreads();

        for (int64_t b = p0 + wave * 64; b < p1; b += 64 * KNN_WAVES) {
            unsigned long long st = 0, en = 0;
            if (b + lane < p1) {
                const int32_t u = a.iu[b + lane];
                const int64_t ulo = a.pu[u], uhi = a.pu[u + 1];
                const int64_t s0 = knn_lower_bound(a.items, ulo, uhi, lo);
                st = (unsigned long long)s0;
                en = (unsigned long long)knn_lower_bound(a.items, s0, uhi, lo + width);
            }
            const int nb = (int)(p1 - b < 64 ? p1 - b : 64);
            for (int z = 0; z < nb; ++z) {
                const int64_t zs = (int64_t)__shfl(st, z), ze = (int64_t)__shfl(en, z);
                for (int64_t t = zs + lane; t < ze; t += 64) atomicAdd(&counts[(int64_t)a.items[t] - lo], 1u);
            }
        }
        __syncthreads();

        int qn = 0;
        uint64_t thr = 0;
        for (int base = wave * 64; base < width; base += 64 * KNN_WAVES) {
            const int j = base + lane;
            const uint32_t c = j < width ? counts[j] : 0u;
            const bool ok = c > 0 && lo + j != i;
            uint64_t key = 0;
            if (ok) key = topk_key(knn_sim(a.metric, c, p1 - p0, a.pi[lo + j + 1] - a.pi[lo + j], a.shrink), lo + j);
            knn_offer<CAP>(q, qn, thr, K, lane, ok, key);
        }
        if (qn > 0) knn_compact<CAP>(q, qn, thr, K, lane);
        if (lane == 0) wcnt[wave] = qn;
        __syncthreads();

        if (wave == 0) {
            for (int w = 1; w < KNN_WAVES; ++w) {
                const int n = wcnt[w];
                for (int off = 0; off < n; off += 64) {
                    const bool ok = off + lane < n;
                    knn_offer<CAP>(q, qn, thr, K, lane, ok, ok ? queue[w][off + lane] : 0);
                }
            }
            if (qn > 0) knn_compact<CAP>(q, qn, thr, K, lane);
            uint64_t* dst = a.part + ((size_t)r * a.slices + slice) * K;
            for (int t = lane; t < K; t += 64) dst[t] = t < qn ? q[t] : 0;
        }
        // the next row's appends to the other waves' queues come after two more barriers, which wave 0 joins when it is done
    }
}

template <int R, int MODE>
__global__ __launch_bounds__(256) void k_knn_score(KnnScoreArgs a) {
    __shared__ float acc[KNN_WAVES][KNN_W_SCORE];
    __shared__ uint64_t queue[KNN_WAVES][KNN_SCORE_CAP];
    static_assert(sizeof(acc) + sizeof(queue) == knn_score_lds(), "knn_plan reports another LDS size");
    static_assert(KNN_SCORE_CAP >= KNN_KMAX + 64, "a queue must hold k plus one append");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * KNN_WAVES + wave;
    if (w >= a.n * a.slices) return;                     // waves never meet at a block barrier
    const int64_t qi = a.q_lo + w / a.slices;
    const int slice = (int)(w % a.slices);
    const int64_t row = a.users ? (int64_t)a.users[qi] : qi;
    const int64_t l0 = a.ptr[row], l1 = a.ptr[row + 1];
    const int64_t lo = (int64_t)slice * KNN_W_SCORE;
    const int width = (int)(a.n_items - lo < KNN_W_SCORE ? a.n_items - lo : KNN_W_SCORE);
    const int K = a.K;
    float* A = acc[wave];

    for (int t = lane; t < width; t += 64) A[t] = 0.f;
    wave_lds_sync();
    for (int64_t g = l0; g < l1; g += KNN_SCORE_AHEAD) {
        int32_t nj[KNN_SCORE_AHEAD][R];
        float ns[KNN_SCORE_AHEAD][R];
#pragma unroll
        for (int d = 0; d < KNN_SCORE_AHEAD; ++d) {
            const bool has = g + d < l1;
            const int64_t base = has ? (int64_t)a.ids[g + d] * K : 0;
#pragma unroll
            for (int rr = 0; rr < R; ++rr) {
                const int slot = lane + 64 * rr;
                nj[d][rr] = -1;
                ns[d][rr] = 0.f;
                if (has && slot < K) { nj[d][rr] = a.nb_items[base + slot]; ns[d][rr] = a.nb_scores[base + slot]; }
            }
        }
#pragma unroll
        for (int d = 0; d < KNN_SCORE_AHEAD; ++d) {
#pragma unroll
            for (int rr = 0; rr < R; ++rr) {
                const int64_t col = (int64_t)nj[d][rr] - lo;
                if (nj[d][rr] >= 0 && col >= 0 && col < width) A[col] += ns[d][rr];
            }
            wave_lds_sync();                             // item d's adds stand before item d + 1's reads
        }
    }
    if (a.xptr) {
        const int64_t x0 = a.xptr[qi], x1 = a.xptr[qi + 1];
        for (int64_t t = x0 + lane; t < x1; t += 64) {
            const int64_t col = (int64_t)a.xids[t] - lo;
            if (col >= 0 && col < width) A[col] = __builtin_nanf("");
        }
        wave_lds_sync();
    }

    if (MODE == 0) {
        uint64_t* q = queue[wave];
        int qn = 0;
        uint64_t thr = 0;
        for (int base = 0; base < width; base += 64) {
            const int j = base + lane;
            const float v = j < width ? A[j] : __builtin_nanf("");
            const bool ok = !__builtin_isnan(v);
            knn_offer<KNN_SCORE_CAP>(q, qn, thr, a.k, lane, ok, ok ? topk_key(v, lo + j) : 0);
        }
        if (qn > 0) knn_compact<KNN_SCORE_CAP>(q, qn, thr, a.k, lane);
        uint64_t* dst = a.part + (size_t)w * a.k;        // w = (query of the chunk) * slices + slice
        for (int t = lane; t < a.k; t += 64) dst[t] = t < qn ? q[t] : 0;
    } else if (MODE == 1) {
        const int64_t t0 = a.tptr[qi], t1 = a.tptr[qi + 1];
        for (int64_t t = t0 + lane; t < t1; t += 64) {
            const int64_t col = (int64_t)a.tids[t] - lo;
            if (col >= 0 && col < width) {
                const float v = A[col];
                const bool ranked = !__builtin_isnan(v);
                a.tkeys[t] = ranked ? topk_key(v, lo + col) : 0;
                a.ranks[t] = ranked ? 0 : -1;
            }
        }
    } else {
        const int64_t t0 = a.tptr[qi], t1 = a.tptr[qi + 1];
        for (int64_t tb = t0; tb < t1; tb += 64) {
            const uint64_t tk = tb + lane < t1 ? a.tkeys[tb + lane] : 0;
            if (__ballot(tk != 0) == 0) continue;
            int32_t above = 0;
            for (int j = 0; j < width; ++j) {
                const float v = A[j];                    // one address for the wave: a broadcast read
                if (!__builtin_isnan(v)) above += topk_key(v, lo + j) > tk ? 1 : 0;
            }
            if (tk != 0 && above > 0) atomicAdd(&a.ranks[tb + lane], above);
        }
    }
}

thread_local char g_knn_err[512] = "";
int knn_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_knn_err, sizeof(g_knn_err), fmt, ap);
    va_end(ap);
    return code;
}
#define KNNCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return knn_fail(e_ == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, \
                                              "%s: %s", #expr, hipGetErrorString(e_));                \
    } while (0)

// a CSR of n rows over ids in [0, bound): indptr from `from0 ? 0 : anything >= 0` and non-decreasing, rows strictly
// increasing (`strict`) or non-decreasing.  TFR_OK, or the code with the message set.
int knn_check_csr(const char* who, const char* what, bool from0, bool strict, const int64_t* indptr, const int32_t* ids, int64_t n,
                  int64_t bound) {
    if (!indptr) return knn_fail(TFR_ERR_ARG, "%s: null %s indptr", who, what);
    if (from0 ? indptr[0] != 0 : indptr[0] < 0) return knn_fail(TFR_ERR_ARG, "%s: %s indptr must start at 0", who, what);
    for (int64_t r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) return knn_fail(TFR_ERR_ARG, "%s: %s indptr decreases at row %lld", who, what, (long long)r);
    if (indptr[n] > indptr[0] && !ids) return knn_fail(TFR_ERR_ARG, "%s: %s indptr without ids", who, what);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            if (ids[e] < 0 || ids[e] >= bound)
                return knn_fail(TFR_ERR_OOB, "%s: %s row %lld: id %d out of range", who, what, (long long)r, ids[e]);
            if (e > indptr[r] && (strict ? ids[e] <= ids[e - 1] : ids[e] < ids[e - 1]))
                return knn_fail(TFR_ERR_ARG, "%s: %s row %lld is not %s", who, what, (long long)r,
                                strict ? "strictly increasing" : "non-decreasing");
        }
    return TFR_OK;
}

int knn_check_users(const char* who, const tfr_knn* m, const int32_t* users, int64_t n) {
    if (!users) return knn_fail(TFR_ERR_ARG, "%s: null users", who);
    for (int64_t q = 0; q < n; ++q)
        if (users[q] < 0 || users[q] >= m->n_users) return knn_fail(TFR_ERR_OOB, "%s: user id %d out of range", who, users[q]);
    return TFR_OK;
}

// a host CSR onto the device: indptr as it stands, the ids [0, indptr[n])
int knn_stage_csr(tfr_knn* m, tfr::DevBuf<int64_t>& dp, tfr::DevBuf<int32_t>& di, const int64_t* indptr, const int32_t* ids, int64_t n) {
    KNNCHK(dp.reserve(n + 1, m->stream));
    KNNCHK(di.reserve(std::max<int64_t>(1, indptr[n]), m->stream));
    KNNCHK(hipMemcpyAsync(dp, indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, m->stream));
    if (indptr[n] > 0) KNNCHK(hipMemcpyAsync(di, ids, (size_t)indptr[n] * 4, hipMemcpyHostToDevice, m->stream));
    return TFR_OK;
}

template <int MODE>
void launch_knn_score(const KnnScoreArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.n * a.slices + KNN_WAVES - 1) / KNN_WAVES));
    const int R = knn_rounds(a.K);
    void (*kernel)(KnnScoreArgs) = k_knn_score<4, MODE>;
    if (R == 1) kernel = k_knn_score<1, MODE>;
    if (R == 2) kernel = k_knn_score<2, MODE>;
    hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, a);
}

// the query side of an argument block: the resident rows named by staged users, or staged lists
struct KnnQuery { const int32_t* users; const int64_t* ptr; const int32_t* ids; };

KnnScoreArgs knn_score_args(const tfr_knn* m, const KnnQuery& q) {
    KnnScoreArgs a = {};
    a.users = q.users; a.ptr = q.ptr; a.ids = q.ids;
    a.nb_items = m->nb_items; a.nb_scores = m->nb_scores;
    a.n_items = m->n_items; a.K = m->K;
    return a;
}

// top-K of n queries whose lists are on the device; the exclusion CSR is the host's, already checked
int knn_topk_run(tfr_knn* m, const char* who, const KnnQuery& q, int64_t n, int32_t k, const int64_t* xip, const int32_t* xit,
                 int32_t* items_out, float* scores_out) {
    KnnPlan p;
    if (!knn_plan(1, m->n_items, k, n, &p))
        return knn_fail(TFR_ERR_ARG, "%s: no plan for k %d over %lld items (slices * k <= %lld)", who, k, (long long)m->n_items,
                        (long long)tfr::TOPK_MERGE_KEYS);
    hipStream_t s = m->stream;
    if (xip) if (int rc = knn_stage_csr(m, m->x_ptr, m->x_ids, xip, xit, n)) return rc;
    KNNCHK(m->out_items.reserve(n * k, s));
    if (scores_out) KNNCHK(m->out_scores.reserve(n * k, s));
    KNNCHK(m->part.reserve(p.chunk * p.slices * k, s));
    KnnScoreArgs a = knn_score_args(m, q);
    if (xip) { a.xptr = m->x_ptr; a.xids = m->x_ids; }
    a.part = m->part; a.k = k; a.slices = p.slices;
    for (int64_t c0 = 0; c0 < n; c0 += p.chunk) {
        a.q_lo = c0;
        a.n = n - c0 < p.chunk ? n - c0 : p.chunk;
        launch_knn_score<0>(a, s);
        KNNCHK(hipGetLastError());
        tfr::TopkMergeArgs g;
        memset(&g, 0, sizeof(g));
        g.part = m->part; g.items_out = m->out_items.get() + c0 * k;
        g.scores_out = scores_out ? m->out_scores.get() + c0 * k : nullptr;
        g.n_rows = a.n; g.k = k; g.slices = p.slices;
        tfr::launch_topk_merge(g, s);
        KNNCHK(hipGetLastError());
    }
    KNNCHK(hipMemcpyAsync(items_out, m->out_items, (size_t)n * k * 4, hipMemcpyDeviceToHost, s));
    if (scores_out) KNNCHK(hipMemcpyAsync(scores_out, m->out_scores, (size_t)n * k * 4, hipMemcpyDeviceToHost, s));
    KNNCHK(hipStreamSynchronize(s));
    return TFR_OK;
}

int knn_check_k(const char* who, int32_t k) {
    return k < 1 || k > KNN_KMAX ? knn_fail(TFR_ERR_ARG, "%s: k must be in [1, %d] (got %d)", who, KNN_KMAX, k) : TFR_OK;
}

}  // namespace

extern "C" {

const char* tfr_knn_last_error(void) { return g_knn_err; }

int tfr_knn_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t which, int32_t* slice_width, int32_t* slices, int64_t* row_chunk,
                 int64_t* lds_bytes, int32_t* look_ahead) {
    if (which < 0 || which > 1) return knn_fail(TFR_ERR_ARG, "knn plan: which must be 0 (fit) or 1 (scoring)");
    if (n_items < 1 || n_items > 0x7fffffffLL || n_rows < 0) return knn_fail(TFR_ERR_ARG, "knn plan: n_rows >= 0 and 1 <= n_items < 2^31");
    if (int rc = knn_check_k("knn plan", k)) return rc;
    KnnPlan p;
    if (!knn_plan(which, n_items, k, n_rows, &p))
        return knn_fail(TFR_ERR_ARG, "knn plan: %lld items need more than %lld / k slices", (long long)n_items, (long long)tfr::TOPK_MERGE_KEYS);
    if (slice_width) *slice_width = p.width;
    if (slices) *slices = p.slices;
    if (row_chunk) *row_chunk = p.chunk;
    if (lds_bytes) *lds_bytes = (int64_t)std::max(p.lds, tfr::topk_merge_lds(p.slices, k));
    if (look_ahead) *look_ahead = p.ahead;
    return TFR_OK;
}

int tfr_knn_destroy(tfr_knn* m) {
    if (!m) return TFR_OK;
    (void)hipSetDevice(m->device);                       // the buffers are freed with the model's device current
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->ev0) (void)hipEventDestroy(m->ev0);
    if (m->ev1) (void)hipEventDestroy(m->ev1);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return TFR_OK;
}

int tfr_knn_create(tfr_knn** out, int64_t n_users, int64_t n_items, int32_t K, int32_t metric, double shrink, int32_t device) {
    if (!out) return knn_fail(TFR_ERR_ARG, "out is null");
    *out = nullptr;
    if (n_users < 1 || n_items < 1 || n_users > 0x7fffffffLL || n_items > 0x7fffffffLL)
        return knn_fail(TFR_ERR_ARG, "need positive int32 user and item counts");
    if (int rc = knn_check_k("create", K)) return rc;
    if (metric < KNN_COSINE || metric > KNN_COUNT) return knn_fail(TFR_ERR_ARG, "metric must be 0 (cosine), 1 (jaccard) or 2 (count)");
    if (!(shrink >= 0.0) || !std::isfinite(shrink)) return knn_fail(TFR_ERR_ARG, "shrink must be non-negative and finite");
    if (metric == KNN_COUNT && shrink != 0.0) return knn_fail(TFR_ERR_ARG, "the count metric takes no shrink");
    KnnPlan p;
    if (!knn_plan(0, n_items, K, n_items, &p))
        return knn_fail(TFR_ERR_ARG, "%lld items at K %d need more than %lld / K slices", (long long)n_items, K, (long long)tfr::TOPK_MERGE_KEYS);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return knn_fail(TFR_ERR_HIP, "no HIP device available - this library has no CPU path");
    if (device < 0 || device >= ndev) return knn_fail(TFR_ERR_ARG, "device %d not in [0,%d)", device, ndev);
    KNNCHK(hipSetDevice(device));
    tfr_knn* m = new (std::nothrow) tfr_knn();
    if (!m) return knn_fail(TFR_ERR_NOMEM, "host allocation failed");
    m->n_users = n_users; m->n_items = n_items; m->K = K; m->metric = metric; m->shrink = shrink; m->device = device;
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = m->nb_items.reserve(n_items * K, m->stream);
    if (e == hipSuccess) e = m->nb_scores.reserve(n_items * K, m->stream);
    if (e == hipSuccess) e = hipEventCreate(&m->ev0);
    if (e == hipSuccess) e = hipEventCreate(&m->ev1);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP;
        tfr_knn_destroy(m);
        return knn_fail(code, "knn_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

// The user CSR.  Everything is checked and the transpose built on the host before any device work, so a refused load
// leaves the model as it was.  A load forgets the fitted neighbours.
int tfr_knn_load(tfr_knn* m, const int64_t* indptr, const int32_t* items) {
    if (!m) return knn_fail(TFR_ERR_ARG, "null model");
    const int64_t nu = m->n_users, ni = m->n_items;
    if (int rc = knn_check_csr("load", "user", true, true, indptr, items, nu, ni)) return rc;
    const int64_t nnz = indptr[nu];
    // the item-major orientation: users ascend inside each item's list because the rows are walked in order
    std::vector<int64_t> pi((size_t)ni + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) pi[(size_t)items[e] + 1]++;
    for (int64_t i = 0; i < ni; ++i) pi[(size_t)i + 1] += pi[(size_t)i];
    std::vector<int64_t> cur(pi.begin(), pi.end() - 1);
    std::vector<int32_t> iu((size_t)nnz);
    for (int64_t u = 0; u < nu; ++u)
        for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) iu[(size_t)cur[(size_t)items[e]]++] = (int32_t)u;

    KNNCHK(hipSetDevice(m->device));
    KNNCHK(hipStreamSynchronize(m->stream));
    m->loaded = false;
    m->fitted = false;
    const int64_t cap = std::max<int64_t>(1, nnz);
    KNNCHK(m->pu.reserve(nu + 1, m->stream));
    KNNCHK(m->pi.reserve(ni + 1, m->stream));
    KNNCHK(m->items.reserve(cap, m->stream));
    KNNCHK(m->iu.reserve(cap, m->stream));
    KNNCHK(hipMemcpy(m->pu, indptr, (size_t)(nu + 1) * 8, hipMemcpyHostToDevice));
    KNNCHK(hipMemcpy(m->pi, pi.data(), pi.size() * 8, hipMemcpyHostToDevice));
    if (nnz) {
        KNNCHK(hipMemcpy(m->items, items, (size_t)nnz * 4, hipMemcpyHostToDevice));
        KNNCHK(hipMemcpy(m->iu, iu.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
    }
    m->loaded = true;
    return TFR_OK;
}

int tfr_knn_fit(tfr_knn* m, float* elapsed_ms) {
    if (!m) return knn_fail(TFR_ERR_ARG, "null model");
    if (!m->loaded) return knn_fail(TFR_ERR_STATE, "no data: call tfr_knn_load first");
    KnnPlan p;
    if (!knn_plan(0, m->n_items, m->K, m->n_items, &p)) return knn_fail(TFR_ERR_ARG, "fit: no plan");
    KNNCHK(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    m->fitted = false;
    KNNCHK(m->part.reserve(p.chunk * p.slices * m->K, s));
    (void)hipEventRecord(m->ev0, s);
    KnnFitArgs a = {};
    a.pu = m->pu; a.items = m->items; a.pi = m->pi; a.iu = m->iu; a.part = m->part;
    a.n_items = m->n_items; a.shrink = m->shrink; a.K = m->K; a.slices = p.slices; a.metric = m->metric;
    for (int64_t r0 = 0; r0 < m->n_items; r0 += p.chunk) {
        a.row_lo = r0;
        a.n_rows = m->n_items - r0 < p.chunk ? m->n_items - r0 : p.chunk;
        const dim3 g((unsigned)std::min<int64_t>(a.n_rows, KNN_GRID_ROWS), (unsigned)p.slices);
        void (*kernel)(KnnFitArgs) = p.cap == 256 ? k_knn_cooc<256> : k_knn_cooc<512>;
        hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, a);
        KNNCHK(hipGetLastError());
        tfr::TopkMergeArgs mg;
        memset(&mg, 0, sizeof(mg));
        mg.part = m->part; mg.items_out = m->nb_items.get() + r0 * m->K; mg.scores_out = m->nb_scores.get() + r0 * m->K;
        mg.n_rows = a.n_rows; mg.k = m->K; mg.slices = p.slices;
        tfr::launch_topk_merge(mg, s);
        KNNCHK(hipGetLastError());
    }
    (void)hipEventRecord(m->ev1, s);
    KNNCHK(hipStreamSynchronize(s));
    if (elapsed_ms) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->ev0, m->ev1) != hipSuccess) ms = 0.f;
        *elapsed_ms = ms;
    }
    m->fitted = true;
    return TFR_OK;
}

static int knn_window(const tfr_knn* m, const char* who, int64_t row_lo, int64_t n_rows) {
    if (row_lo < 0 || n_rows < 0 || row_lo > m->n_items || n_rows > m->n_items - row_lo)
        return knn_fail(TFR_ERR_ARG, "%s: rows [%lld, %lld + %lld) are not inside the %lld items", who, (long long)row_lo,
                        (long long)row_lo, (long long)n_rows, (long long)m->n_items);
    return TFR_OK;
}

int tfr_knn_get_neighbours(tfr_knn* m, int64_t row_lo, int64_t n_rows, int32_t* items_out, float* scores_out) {
    if (!m) return knn_fail(TFR_ERR_ARG, "null model");
    if (!m->fitted) return knn_fail(TFR_ERR_STATE, "no neighbours: call tfr_knn_fit or tfr_knn_set_neighbours first");
    if (int rc = knn_window(m, "get_neighbours", row_lo, n_rows)) return rc;
    if (n_rows == 0) return TFR_OK;
    KNNCHK(hipSetDevice(m->device));
    const size_t off = (size_t)row_lo * m->K, cnt = (size_t)n_rows * m->K;
    if (items_out) KNNCHK(hipMemcpyAsync(items_out, m->nb_items.get() + off, cnt * 4, hipMemcpyDeviceToHost, m->stream));
    if (scores_out) KNNCHK(hipMemcpyAsync(scores_out, m->nb_scores.get() + off, cnt * 4, hipMemcpyDeviceToHost, m->stream));
    KNNCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

// Rows [row_lo, row_lo + n_rows) of the neighbour lists from host arrays.  Checked before any device work.  The rows not
// named keep what they hold; on a handle without lists they are set empty first.
int tfr_knn_set_neighbours(tfr_knn* m, int64_t row_lo, int64_t n_rows, const int32_t* items, const float* scores) {
    if (!m) return knn_fail(TFR_ERR_ARG, "null model");
    if (int rc = knn_window(m, "set_neighbours", row_lo, n_rows)) return rc;
    if (n_rows > 0 && (!items || !scores)) return knn_fail(TFR_ERR_ARG, "set_neighbours: null items or scores");
    const int K = m->K;
    std::vector<int32_t> seen;
    for (int64_t r = 0; r < n_rows; ++r) {
        seen.clear();
        for (int c = 0; c < K; ++c) {
            const int32_t j = items[r * K + c];
            if (j == -1) continue;
            if (j < -1 || j >= m->n_items) return knn_fail(TFR_ERR_OOB, "set_neighbours: row %lld: id %d out of range", (long long)(row_lo + r), j);
            if (j == row_lo + r) return knn_fail(TFR_ERR_ARG, "set_neighbours: row %lld lists itself", (long long)(row_lo + r));
            if (!std::isfinite(scores[r * K + c]))
                return knn_fail(TFR_ERR_ARG, "set_neighbours: row %lld: the score of item %d is not finite", (long long)(row_lo + r), j);
            seen.push_back(j);
        }
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
            return knn_fail(TFR_ERR_ARG, "set_neighbours: row %lld repeats an item", (long long)(row_lo + r));
    }
    KNNCHK(hipSetDevice(m->device));
    if (!m->fitted) {                                    // every row empty first: item -1 (every byte 0xff), score -inf
        const std::vector<float> pad((size_t)m->n_items * K, -INFINITY);
        KNNCHK(hipMemsetAsync(m->nb_items, 0xff, pad.size() * 4, m->stream));
        KNNCHK(hipMemcpy(m->nb_scores, pad.data(), pad.size() * 4, hipMemcpyHostToDevice));
    }
    if (n_rows > 0) {
        const size_t off = (size_t)row_lo * K, cnt = (size_t)n_rows * K;
        KNNCHK(hipMemcpyAsync(m->nb_items.get() + off, items, cnt * 4, hipMemcpyHostToDevice, m->stream));
        KNNCHK(hipMemcpyAsync(m->nb_scores.get() + off, scores, cnt * 4, hipMemcpyHostToDevice, m->stream));
    }
    KNNCHK(hipStreamSynchronize(m->stream));
    m->fitted = true;
    return TFR_OK;
}

int tfr_knn_topk(tfr_knn* m, const int32_t* users, int64_t n, int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                 int32_t* items_out, float* scores_out) {
    if (!m) return knn_fail(TFR_ERR_ARG, "null model");
    if (n < 0) return knn_fail(TFR_ERR_ARG, "top-K: negative n");
    if (int rc = knn_check_k("top-K", k)) return rc;
    if (!m->loaded) return knn_fail(TFR_ERR_STATE, "top-K: no data: call tfr_knn_load first");
    if (!m->fitted) return knn_fail(TFR_ERR_STATE, "top-K: no neighbours: call tfr_knn_fit or tfr_knn_set_neighbours first");
    if (n == 0) return TFR_OK;
    if (!items_out) return knn_fail(TFR_ERR_ARG, "top-K: null items_out");
    if (int rc = knn_check_users("top-K", m, users, n)) return rc;
    if (excl_indptr) if (int rc = knn_check_csr("top-K", "exclusion", false, false, excl_indptr, excl_items, n, m->n_items)) return rc;
    KNNCHK(hipSetDevice(m->device));
    KNNCHK(m->q_users.reserve(n, m->stream));
    KNNCHK(hipMemcpyAsync(m->q_users, users, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    return knn_topk_run(m, "top-K", KnnQuery{m->q_users, m->pu, m->items}, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_knn_topk_lists(tfr_knn* m, const int64_t* list_indptr, const int32_t* list_items, int64_t n, int32_t k,
                       const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    if (!m) return knn_fail(TFR_ERR_ARG, "null model");
    if (n < 0) return knn_fail(TFR_ERR_ARG, "top-K of lists: negative n");
    if (int rc = knn_check_k("top-K of lists", k)) return rc;
    if (!m->fitted) return knn_fail(TFR_ERR_STATE, "top-K of lists: no neighbours: call tfr_knn_fit or tfr_knn_set_neighbours first");
    if (n == 0) return TFR_OK;
    if (!items_out) return knn_fail(TFR_ERR_ARG, "top-K of lists: null items_out");
    if (int rc = knn_check_csr("top-K of lists", "list", true, true, list_indptr, list_items, n, m->n_items)) return rc;
    if (excl_indptr)
        if (int rc = knn_check_csr("top-K of lists", "exclusion", false, false, excl_indptr, excl_items, n, m->n_items)) return rc;
    KNNCHK(hipSetDevice(m->device));
    if (int rc = knn_stage_csr(m, m->q_ptr, m->q_ids, list_indptr, list_items, n)) return rc;
    return knn_topk_run(m, "top-K of lists", KnnQuery{nullptr, m->q_ptr, m->q_ids}, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_knn_rank_items(tfr_knn* m, const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
                       const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    if (!m) return knn_fail(TFR_ERR_ARG, "null model");
    if (n < 0) return knn_fail(TFR_ERR_ARG, "rank: negative n");
    if (!m->loaded) return knn_fail(TFR_ERR_STATE, "rank: no data: call tfr_knn_load first");
    if (!m->fitted) return knn_fail(TFR_ERR_STATE, "rank: no neighbours: call tfr_knn_fit or tfr_knn_set_neighbours first");
    if (n == 0) return TFR_OK;
    if (int rc = knn_check_users("rank", m, users, n)) return rc;
    if (int rc = knn_check_csr("rank", "target", false, true, tgt_indptr, tgt_items, n, m->n_items)) return rc;
    if (excl_indptr) if (int rc = knn_check_csr("rank", "exclusion", false, false, excl_indptr, excl_items, n, m->n_items)) return rc;
    const int64_t t0 = tgt_indptr[0], n_tgt = tgt_indptr[n] - t0;
    if (n_tgt == 0) return TFR_OK;
    if (!ranks_out) return knn_fail(TFR_ERR_ARG, "rank: null ranks_out");
    KnnPlan p;                                           // the ranking merges nothing: only the slicing of the plan is used
    if (!knn_plan(1, m->n_items, 1, n, &p)) return knn_fail(TFR_ERR_ARG, "rank: no plan");
    KNNCHK(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    KNNCHK(m->q_users.reserve(n, s));
    KNNCHK(hipMemcpyAsync(m->q_users, users, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (int rc = knn_stage_csr(m, m->t_ptr, m->t_ids, tgt_indptr, tgt_items, n)) return rc;
    if (excl_indptr) if (int rc = knn_stage_csr(m, m->x_ptr, m->x_ids, excl_indptr, excl_items, n)) return rc;
    KNNCHK(m->tkeys.reserve(tgt_indptr[n], s));
    KNNCHK(m->ranks.reserve(tgt_indptr[n], s));
    KnnScoreArgs a = knn_score_args(m, KnnQuery{m->q_users, m->pu, m->items});
    if (excl_indptr) { a.xptr = m->x_ptr; a.xids = m->x_ids; }
    a.tptr = m->t_ptr; a.tids = m->t_ids; a.tkeys = m->tkeys; a.ranks = m->ranks;
    a.q_lo = 0; a.n = n; a.k = 1; a.slices = p.slices;
    launch_knn_score<1>(a, s);
    KNNCHK(hipGetLastError());
    launch_knn_score<2>(a, s);
    KNNCHK(hipGetLastError());
    KNNCHK(hipMemcpyAsync(ranks_out, m->ranks.get() + t0, (size_t)n_tgt * 4, hipMemcpyDeviceToHost, s));
    KNNCHK(hipStreamSynchronize(s));
    return TFR_OK;
}

}  // extern "C"
