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
// k_knn_cooc_w: the same block for tfr_knn_fit_weighted, over slices of KNN_W_WFIT columns:
//   uint64 LDS sums S_ij of fixed-point user weights in place of the counts, by 64-bit integer LDS atomics, exact in any
//   order; sim = (float)((double)S_ij * 2^-shift * row_scale[i] * col_scale[j]); a candidate by S_ij > 0.
// k_knn_score<R, MODE>: one wave per (query, slice of KNN_W_SCORE columns) with a float32 accumulator of its own in LDS,
//   four waves per block, no block barrier.  For the query's items i ascending, KNN_SCORE_AHEAD at a time: the lanes load
//   the items' neighbour rows (coalesced, R rounds of 64 slots), then add them item by item with plain LDS read-add-write.
//   One item's columns are distinct and one wave's LDS operations execute in order: the chain has the stated order.
//   Excluded columns are then overwritten with NaN, which no sum of finite scores gives.  MODE 0 (top-K): scan, keys, queue,
//   part[query, slice].  MODE 1 (ranking): the targets inside the slice get their key.  MODE 2: lane t counts the slots of
//   the slice whose key beats target t's; the slices' counts meet in an integer atomic.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "tfrecomm.h"
#include "svd_kernels.h"
#include "itemknn.h"

namespace {

using tfr::topk_key;
using tfr::wave_lds_sync;
using tfr::fail;
using tfr::check_k;
using tfr::window;

// the weighted fit's similarity: the exact integer sum scaled by a power of two, then two float64 products left to right
// (no add: nothing contracts into an fma), rounded once to float32
__device__ __forceinline__ float knn_wsim(unsigned long long s, double unit, double row_scale, double col_scale) {
    return __double2float_rn((double)s * unit * row_scale * col_scale);
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

        tfr::count_row<KNN_WAVES>(a, counts, p0, p1, lo, width, lane, wave);
        __syncthreads();

        int qn = 0;
        uint64_t thr = 0;
        for (int base = wave * 64; base < width; base += 64 * KNN_WAVES) {
            const int j = base + lane;
            const uint32_t c = j < width ? counts[j] : 0u;
            const bool ok = c > 0 && lo + j != i;
            uint64_t key = 0;
            if (ok) key = topk_key(knn_sim(a.metric, c, p1 - p0, a.pi[lo + j + 1] - a.pi[lo + j], a.shrink), lo + j);
            tfr::queue_offer<CAP>(q, qn, thr, K, lane, ok, key);
        }
        if (qn > 0) tfr::queue_compact<CAP>(q, qn, thr, K, lane);
        if (lane == 0) wcnt[wave] = qn;
        __syncthreads();

        if (wave == 0) {
            for (int w = 1; w < KNN_WAVES; ++w) {
                const int n = wcnt[w];
                for (int off = 0; off < n; off += 64) {
                    const bool ok = off + lane < n;
                    tfr::queue_offer<CAP>(q, qn, thr, K, lane, ok, ok ? queue[w][off + lane] : 0);
                }
            }
            if (qn > 0) tfr::queue_compact<CAP>(q, qn, thr, K, lane);
            uint64_t* dst = a.part + ((size_t)r * a.slices + slice) * K;
            for (int t = lane; t < K; t += 64) dst[t] = t < qn ? q[t] : 0;
        }
        // the next row's appends to the other waves' queues come after two more barriers, which wave 0 joins when it is done
    }
}

// k_knn_cooc with uint64 sums of user weights for the counts and knn_wsim for the similarity; everything from the scan on is
// the same text.  (One body behind both kernels was tried: it changed k_knn_cooc<256>'s code)
template <int CAP>
__global__ __launch_bounds__(256) void k_knn_cooc_w(KnnWFitArgs a) {
    __shared__ unsigned long long sums[KNN_W_WFIT];
    __shared__ uint64_t queue[KNN_WAVES][CAP];
    __shared__ int32_t wcnt[KNN_WAVES];
    static_assert(sizeof(sums) + sizeof(queue) + sizeof(wcnt) == knn_wfit_lds(CAP), "knn_plan reports another LDS size");
    static_assert(CAP >= KNN_KMAX + 64 || CAP == 256, "a queue must hold K plus one append");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.y, K = a.K;
    const int64_t lo = (int64_t)slice * KNN_W_WFIT;
    const int width = (int)(a.n_items - lo < KNN_W_WFIT ? a.n_items - lo : KNN_W_WFIT);
    uint64_t* q = queue[wave];

    for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const int64_t i = a.row_lo + r;
        const int64_t p0 = a.pi[i], p1 = a.pi[i + 1];
        const double rs = a.row_scale[i];
        for (int t = tid; t < width; t += 256) sums[t] = 0;
        __syncthreads();

        tfr::count_row<KNN_WAVES>(a, sums, p0, p1, lo, width, lane, wave);
        __syncthreads();

        int qn = 0;
        uint64_t thr = 0;
        for (int base = wave * 64; base < width; base += 64 * KNN_WAVES) {
            const int j = base + lane;
            const unsigned long long c = j < width ? sums[j] : 0ull;
            const bool ok = c > 0 && lo + j != i;
            uint64_t key = 0;
            if (ok) key = topk_key(knn_wsim(c, a.unit, rs, a.col_scale[lo + j]), lo + j);
            tfr::queue_offer<CAP>(q, qn, thr, K, lane, ok, key);
        }
        if (qn > 0) tfr::queue_compact<CAP>(q, qn, thr, K, lane);
        if (lane == 0) wcnt[wave] = qn;
        __syncthreads();

        if (wave == 0) {
            for (int w = 1; w < KNN_WAVES; ++w) {
                const int n = wcnt[w];
                for (int off = 0; off < n; off += 64) {
                    const bool ok = off + lane < n;
                    tfr::queue_offer<CAP>(q, qn, thr, K, lane, ok, ok ? queue[w][off + lane] : 0);
                }
            }
            if (qn > 0) tfr::queue_compact<CAP>(q, qn, thr, K, lane);
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
    tfr::score_tail<MODE, KNN_SCORE_CAP>(a, A, queue[wave], qi, w, lo, width, lane);
}

thread_local tfr::ErrText g_knn_err;

// what the serving drivers of item_lists.h ask of a family
struct KnnServe {
    using Model = tfr_knn;
    using Args = KnnScoreArgs;
    using Plan = KnnPlan;
    static constexpr auto plan = knn_plan;
    static constexpr const char* load_fn = "tfr_knn_load";
    static constexpr const char* not_fitted = "no neighbours: call tfr_knn_fit or tfr_knn_set_neighbours first";

    static Args args(const Model* m) {
        Args a = {};
        a.nb_items = m->nb_items; a.nb_scores = m->nb_scores;
        a.K = m->K;
        return a;
    }

    template <int MODE>
    static void launch(const Args& a, hipStream_t s) {
        const dim3 g((unsigned)((a.n * a.slices + KNN_WAVES - 1) / KNN_WAVES));
        const int R = knn_rounds(a.K);
        void (*kernel)(KnnScoreArgs) = k_knn_score<4, MODE>;
        if (R == 1) kernel = k_knn_score<1, MODE>;
        if (R == 2) kernel = k_knn_score<2, MODE>;
        hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, a);
    }
};

// The launches of a fit, timed by the handle's events: per row chunk the kernel over (rows, slices), then the merge into
// the handle's lists.  a: the family's own fields set; the CSR, part, n_items, K and slices are set here.  The model's
// device is current and `fitted` is false on entry.
template <class Args>
int run_fit(tfr_knn* m, const KnnPlan& p, Args a, void (*kernel)(Args), float* elapsed_ms) {
    hipStream_t s = m->stream;
    LISTCHK(g_knn_err, m->part.reserve(p.chunk * p.slices * m->K, s));
    (void)hipEventRecord(m->ev0, s);
    a.pu = m->pu; a.items = m->items; a.pi = m->pi; a.iu = m->iu; a.part = m->part;
    a.n_items = m->n_items; a.K = m->K; a.slices = p.slices;
    for (int64_t r0 = 0; r0 < m->n_items; r0 += p.chunk) {
        a.row_lo = r0;
        a.n_rows = m->n_items - r0 < p.chunk ? m->n_items - r0 : p.chunk;
        const dim3 g((unsigned)std::min<int64_t>(a.n_rows, KNN_GRID_ROWS), (unsigned)p.slices);
        hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, a);
        LISTCHK(g_knn_err, hipGetLastError());
        tfr::TopkMergeArgs mg;
        memset(&mg, 0, sizeof(mg));
        mg.part = m->part; mg.items_out = m->nb_items.get() + r0 * m->K; mg.scores_out = m->nb_scores.get() + r0 * m->K;
        mg.n_rows = a.n_rows; mg.k = m->K; mg.slices = p.slices;
        tfr::launch_topk_merge(mg, s);
        LISTCHK(g_knn_err, hipGetLastError());
    }
    (void)hipEventRecord(m->ev1, s);
    LISTCHK(g_knn_err, hipStreamSynchronize(s));
    if (elapsed_ms) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->ev0, m->ev1) != hipSuccess) ms = 0.f;
        *elapsed_ms = ms;
    }
    m->fitted = true;
    return TFR_OK;
}

}  // namespace

void knn_launch_cooc(const KnnFitArgs& a, int cap, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(cap == 256 ? k_knn_cooc<256> : k_knn_cooc<512>, grid, dim3(256), 0, s, a);
}

extern "C" {

const char* tfr_knn_last_error(void) { return g_knn_err.text; }

int tfr_knn_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t which, int32_t* slice_width, int32_t* slices, int64_t* row_chunk,
                 int64_t* lds_bytes, int32_t* look_ahead) {
    if (which < 0 || which > 1) return fail(g_knn_err, TFR_ERR_ARG, "knn plan: which must be 0 (fit) or 1 (scoring)");
    if (n_items < 1 || n_items > 0x7fffffffLL || n_rows < 0) return fail(g_knn_err, TFR_ERR_ARG, "knn plan: n_rows >= 0 and 1 <= n_items < 2^31");
    if (int rc = check_k(g_knn_err, "knn plan", k)) return rc;
    KnnPlan p;
    if (!knn_plan(which, n_items, k, n_rows, &p))
        return fail(g_knn_err, TFR_ERR_ARG, "knn plan: %lld items need more than %lld / k slices", (long long)n_items, (long long)tfr::TOPK_MERGE_KEYS);
    if (slice_width) *slice_width = p.width;
    if (slices) *slices = p.slices;
    if (row_chunk) *row_chunk = p.chunk;
    if (lds_bytes) *lds_bytes = (int64_t)std::max(p.lds, tfr::topk_merge_lds(p.slices, k));
    if (look_ahead) *look_ahead = p.ahead;
    return TFR_OK;
}

int tfr_knn_destroy(tfr_knn* m) { return m ? tfr::destroy_handle(m, {m->ev0, m->ev1}) : TFR_OK; }

int tfr_knn_create(tfr_knn** out, int64_t n_users, int64_t n_items, int32_t K, int32_t metric, double shrink, int32_t device) {
    if (!out) return fail(g_knn_err, TFR_ERR_ARG, "out is null");
    *out = nullptr;
    if (int rc = tfr::check_counts(g_knn_err, n_users, n_items)) return rc;
    if (int rc = check_k(g_knn_err, "create", K)) return rc;
    if (metric < KNN_COSINE || metric > KNN_COUNT) return fail(g_knn_err, TFR_ERR_ARG, "metric must be 0 (cosine), 1 (jaccard) or 2 (count)");
    if (!(shrink >= 0.0) || !std::isfinite(shrink)) return fail(g_knn_err, TFR_ERR_ARG, "shrink must be non-negative and finite");
    if (metric == KNN_COUNT && shrink != 0.0) return fail(g_knn_err, TFR_ERR_ARG, "the count metric takes no shrink");
    KnnPlan p;
    if (!knn_plan(0, n_items, K, n_items, &p))
        return fail(g_knn_err, TFR_ERR_ARG, "%lld items at K %d need more than %lld / K slices", (long long)n_items, K, (long long)tfr::TOPK_MERGE_KEYS);
    tfr_knn* m = nullptr;
    if (int rc = tfr::create_handle(g_knn_err, "knn_create", &m, n_users, n_items, device)) return rc;
    m->K = K; m->metric = metric; m->shrink = shrink;
    hipError_t e = m->nb_items.reserve(n_items * K, m->stream);
    if (e == hipSuccess) e = m->nb_scores.reserve(n_items * K, m->stream);
    if (e == hipSuccess) e = hipEventCreate(&m->ev0);
    if (e == hipSuccess) e = hipEventCreate(&m->ev1);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP;
        tfr_knn_destroy(m);
        return fail(g_knn_err, code, "knn_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

// A load forgets the fitted neighbours (item_lists.h load_lists: `fitted`).
int tfr_knn_load(tfr_knn* m, const int64_t* indptr, const int32_t* items) {
    if (int rc = tfr::load_lists(g_knn_err, m, indptr, items, [] {})) return rc;
    std::vector<int64_t> len((size_t)m->n_items, 0);     // the CSR passed load_lists' checks: every id is inside
    for (int64_t e = 0; e < indptr[m->n_users]; ++e) len[(size_t)items[e]]++;
    m->max_item_users = *std::max_element(len.begin(), len.end());
    return TFR_OK;
}

int tfr_knn_fit(tfr_knn* m, float* elapsed_ms) {
    if (!m) return fail(g_knn_err, TFR_ERR_ARG, "null model");
    if (!m->loaded) return fail(g_knn_err, TFR_ERR_STATE, "no data: call tfr_knn_load first");
    KnnPlan p;
    if (!knn_plan(0, m->n_items, m->K, m->n_items, &p)) return fail(g_knn_err, TFR_ERR_ARG, "fit: no plan");
    LISTCHK(g_knn_err, hipSetDevice(m->device));
    m->fitted = false;
    KnnFitArgs a = {};
    a.shrink = m->shrink; a.metric = m->metric;
    return run_fit(m, p, a, p.cap == 256 ? k_knn_cooc<256> : k_knn_cooc<512>, elapsed_ms);
}

int tfr_knn_weighted_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t* slice_width, int32_t* slices, int64_t* row_chunk,
                          int64_t* lds_bytes, int32_t* look_ahead) {
    if (n_items < 1 || n_items > 0x7fffffffLL || n_rows < 0)
        return fail(g_knn_err, TFR_ERR_ARG, "knn weighted plan: n_rows >= 0 and 1 <= n_items < 2^31");
    if (int rc = check_k(g_knn_err, "knn weighted plan", k)) return rc;
    KnnPlan p;
    if (!knn_plan(2, n_items, k, n_rows, &p))
        return fail(g_knn_err, TFR_ERR_ARG, "knn weighted plan: %lld items need more than %lld / k slices", (long long)n_items,
                    (long long)tfr::TOPK_MERGE_KEYS);
    if (slice_width) *slice_width = p.width;
    if (slices) *slices = p.slices;
    if (row_chunk) *row_chunk = p.chunk;
    if (lds_bytes) *lds_bytes = (int64_t)std::max(p.lds, tfr::topk_merge_lds(p.slices, k));
    if (look_ahead) *look_ahead = p.ahead;
    return TFR_OK;
}

// Everything is checked on the host before any device work: a refused call leaves the lists as they were.
int tfr_knn_fit_weighted(tfr_knn* m, const uint64_t* user_w, const double* row_scale, const double* col_scale, int32_t shift,
                         float* elapsed_ms) {
    if (!m) return fail(g_knn_err, TFR_ERR_ARG, "null model");
    if (!user_w || !row_scale || !col_scale) return fail(g_knn_err, TFR_ERR_ARG, "fit_weighted: null user_w, row_scale or col_scale");
    if (shift < 0 || shift > 62) return fail(g_knn_err, TFR_ERR_ARG, "fit_weighted: shift must be in [0, 62] (got %d)", shift);
    double rmax = 0.0, cmax = 0.0;
    for (int64_t i = 0; i < m->n_items; ++i) {
        if (!(row_scale[i] >= 0.0) || !std::isfinite(row_scale[i]) || !(col_scale[i] >= 0.0) || !std::isfinite(col_scale[i]))
            return fail(g_knn_err, TFR_ERR_ARG, "fit_weighted: the scales of item %lld are not both finite and >= 0", (long long)i);
        rmax = std::max(rmax, row_scale[i]);
        cmax = std::max(cmax, col_scale[i]);
    }
    KnnPlan p;
    if (!knn_plan(2, m->n_items, m->K, m->n_items, &p))
        return fail(g_knn_err, TFR_ERR_ARG, "fit_weighted: %lld items at K %d need more than %lld / K slices of %d columns",
                    (long long)m->n_items, m->K, (long long)tfr::TOPK_MERGE_KEYS, KNN_W_WFIT);
    if (!m->loaded) return fail(g_knn_err, TFR_ERR_STATE, "no data: call tfr_knn_load first");
    uint64_t wmax = 0;
    for (int64_t u = 0; u < m->n_users; ++u) wmax = std::max(wmax, user_w[u]);
    // every sum stays below 2^63: max weight * longest item list <= 2^63 - 1, by a division
    if (m->max_item_users > 0 && wmax > 0x7fffffffffffffffULL / (uint64_t)m->max_item_users)
        return fail(g_knn_err, TFR_ERR_ARG, "fit_weighted: weight %llu times %lld users of one item reaches 2^63", (unsigned long long)wmax,
                    (long long)m->max_item_users);
    // and every similarity is a finite float32: the products grow with each factor, so the largest of each bounds them
    const double unit = ldexp(1.0, -shift);
    const double top = (double)(wmax * (uint64_t)m->max_item_users) * unit * rmax * cmax;
    if (!(top <= (double)FLT_MAX))
        return fail(g_knn_err, TFR_ERR_ARG, "fit_weighted: a similarity could reach %g, past float32", top);
    LISTCHK(g_knn_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    m->fitted = false;
    LISTCHK(g_knn_err, m->uw.reserve(m->n_users, s));
    LISTCHK(g_knn_err, m->row_scale.reserve(m->n_items, s));
    LISTCHK(g_knn_err, m->col_scale.reserve(m->n_items, s));
    LISTCHK(g_knn_err, hipMemcpyAsync(m->uw, user_w, (size_t)m->n_users * 8, hipMemcpyHostToDevice, s));
    LISTCHK(g_knn_err, hipMemcpyAsync(m->row_scale, row_scale, (size_t)m->n_items * 8, hipMemcpyHostToDevice, s));
    LISTCHK(g_knn_err, hipMemcpyAsync(m->col_scale, col_scale, (size_t)m->n_items * 8, hipMemcpyHostToDevice, s));
    KnnWFitArgs a = {};
    a.uw = m->uw; a.row_scale = m->row_scale; a.col_scale = m->col_scale; a.unit = unit;
    return run_fit(m, p, a, p.cap == 256 ? k_knn_cooc_w<256> : k_knn_cooc_w<512>, elapsed_ms);
}

int tfr_knn_get_neighbours(tfr_knn* m, int64_t row_lo, int64_t n_rows, int32_t* items_out, float* scores_out) {
    if (!m) return fail(g_knn_err, TFR_ERR_ARG, "null model");
    if (!m->fitted) return fail(g_knn_err, TFR_ERR_STATE, "no neighbours: call tfr_knn_fit or tfr_knn_set_neighbours first");
    if (int rc = window(g_knn_err, m, "get_neighbours", row_lo, n_rows)) return rc;
    if (n_rows == 0) return TFR_OK;
    LISTCHK(g_knn_err, hipSetDevice(m->device));
    const size_t off = (size_t)row_lo * m->K, cnt = (size_t)n_rows * m->K;
    if (items_out) LISTCHK(g_knn_err, hipMemcpyAsync(items_out, m->nb_items.get() + off, cnt * 4, hipMemcpyDeviceToHost, m->stream));
    if (scores_out) LISTCHK(g_knn_err, hipMemcpyAsync(scores_out, m->nb_scores.get() + off, cnt * 4, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_knn_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

// Rows [row_lo, row_lo + n_rows) of the neighbour lists from host arrays.  Checked before any device work.  The rows not
// named keep what they hold; on a handle without lists they are set empty first.
int tfr_knn_set_neighbours(tfr_knn* m, int64_t row_lo, int64_t n_rows, const int32_t* items, const float* scores) {
    if (!m) return fail(g_knn_err, TFR_ERR_ARG, "null model");
    if (int rc = window(g_knn_err, m, "set_neighbours", row_lo, n_rows)) return rc;
    if (n_rows > 0 && (!items || !scores)) return fail(g_knn_err, TFR_ERR_ARG, "set_neighbours: null items or scores");
    const int K = m->K;
    std::vector<int32_t> seen;
    for (int64_t r = 0; r < n_rows; ++r) {
        seen.clear();
        for (int c = 0; c < K; ++c) {
            const int32_t j = items[r * K + c];
            if (j == -1) continue;
            if (j < -1 || j >= m->n_items) return fail(g_knn_err, TFR_ERR_OOB, "set_neighbours: row %lld: id %d out of range", (long long)(row_lo + r), j);
            if (j == row_lo + r) return fail(g_knn_err, TFR_ERR_ARG, "set_neighbours: row %lld lists itself", (long long)(row_lo + r));
            if (!std::isfinite(scores[r * K + c]))
                return fail(g_knn_err, TFR_ERR_ARG, "set_neighbours: row %lld: the score of item %d is not finite", (long long)(row_lo + r), j);
            seen.push_back(j);
        }
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
            return fail(g_knn_err, TFR_ERR_ARG, "set_neighbours: row %lld repeats an item", (long long)(row_lo + r));
    }
    LISTCHK(g_knn_err, hipSetDevice(m->device));
    if (!m->fitted) {                                    // every row empty first: item -1 (every byte 0xff), score -inf
        const std::vector<float> pad((size_t)m->n_items * K, -INFINITY);
        LISTCHK(g_knn_err, hipMemsetAsync(m->nb_items, 0xff, pad.size() * 4, m->stream));
        LISTCHK(g_knn_err, hipMemcpy(m->nb_scores, pad.data(), pad.size() * 4, hipMemcpyHostToDevice));
    }
    if (n_rows > 0) {
        const size_t off = (size_t)row_lo * K, cnt = (size_t)n_rows * K;
        LISTCHK(g_knn_err, hipMemcpyAsync(m->nb_items.get() + off, items, cnt * 4, hipMemcpyHostToDevice, m->stream));
        LISTCHK(g_knn_err, hipMemcpyAsync(m->nb_scores.get() + off, scores, cnt * 4, hipMemcpyHostToDevice, m->stream));
    }
    LISTCHK(g_knn_err, hipStreamSynchronize(m->stream));
    m->fitted = true;
    return TFR_OK;
}

int tfr_knn_topk(tfr_knn* m, const int32_t* users, int64_t n, int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                 int32_t* items_out, float* scores_out) {
    return tfr::topk_users<KnnServe>(g_knn_err, m, users, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_knn_topk_lists(tfr_knn* m, const int64_t* list_indptr, const int32_t* list_items, int64_t n, int32_t k,
                       const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    return tfr::topk_lists<KnnServe>(g_knn_err, m, list_indptr, list_items, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_knn_rank_items(tfr_knn* m, const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
                       const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    return tfr::rank_users<KnnServe>(g_knn_err, m, users, n, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

}  // extern "C"
