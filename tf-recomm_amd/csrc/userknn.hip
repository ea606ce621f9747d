// userknn.hip - user-based nearest neighbours on gfx950 (tfr_uknn_*).
//   X: the binary user x item matrix.  d_u = items of user u, c_uv = items both u and v have.  sim(u, v) is knn_sim of
//   (c_uv, d_u, d_v).  The neighbours of u are the K users v != u, c_uv > 0 with the largest key (similarity descending, id
//   ascending).  score(u, j) = the float32 add chain from +0 over u's neighbour slots, slot 0 first, of sim(u, v) for the v
//   that have j.  No division by the sum of the similarities: a per-user constant moves no ranking.
//
// Fit: itemknn.hip's k_knn_cooc through knn_launch_cooc, with the user rows where it reads item lists and the other way round.
// k_uknn_score<R, MODE>: one wave per (query, slice of KNN_W_SCORE item columns) with a float32 accumulator of its own in
//   LDS, four waves per block, no block barrier.  Lane l loads neighbour slots l + 64 r of the query's row: the id, the
//   similarity, the bounds of that user's item row, and finds the part of the row inside the slice by two binary searches -
//   all K searches run side by side.  Then the wave walks the slots in order by __shfl; lanes stride over that neighbour's
//   part and do a plain LDS read-add-write.  One neighbour's items are distinct, so its adds never meet; a wave_lds_sync puts
//   neighbour t's adds before neighbour t + 1's: the chain has the stated order, without atomics.  The tail is score_tail.
// k_uknn_query_cooc<CAP>: k_knn_cooc's block per (query list, slice of KNN_W_FIT user columns): count_row over the list's
//   items with the model's item lists as the rows it walks; d_L is the list's length, d_v the resident row's; nobody is
//   left out as "self".  Queue, per-slice keys and merge as in the fit, into a [n, K] pair k_uknn_score reads by row q.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "tfrecomm.h"
#include "svd_kernels.h"
#include "userknn.h"

namespace {

using tfr::topk_key;
using tfr::wave_lds_sync;
using tfr::fail;
using tfr::check_k;

template <int R, int MODE>
__global__ __launch_bounds__(256) void k_uknn_score(UknnScoreArgs a) {
    __shared__ float acc[KNN_WAVES][KNN_W_SCORE];
    __shared__ uint64_t queue[KNN_WAVES][KNN_SCORE_CAP];
    static_assert(sizeof(acc) + sizeof(queue) == knn_score_lds(), "uknn_plan reports another LDS size");
    static_assert(KNN_SCORE_CAP >= KNN_KMAX + 64, "a queue must hold k plus one append");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * KNN_WAVES + wave;
    if (w >= a.n * a.slices) return;                     // waves never meet at a block barrier
    const int64_t qi = a.q_lo + w / a.slices;
    const int slice = (int)(w % a.slices);
    const int64_t row = a.users ? (int64_t)a.users[qi] : qi;
    const int64_t lo = (int64_t)slice * KNN_W_SCORE;
    const int width = (int)(a.n_items - lo < KNN_W_SCORE ? a.n_items - lo : KNN_W_SCORE);
    const int K = a.K;
    float* A = acc[wave];

    for (int t = lane; t < width; t += 64) A[t] = 0.f;
    unsigned long long st[R], en[R];
    float sv[R];
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int slot = lane + 64 * rr;
        st[rr] = 0; en[rr] = 0; sv[rr] = 0.f;
        const int32_t v = slot < K ? a.nb_users[row * K + slot] : -1;
        if (v >= 0) {
            sv[rr] = a.nb_scores[row * K + slot];
            const int64_t vlo = a.pu[v], vhi = a.pu[v + 1];
            const int64_t s0 = tfr::list_lower_bound(a.items, vlo, vhi, lo);
            st[rr] = (unsigned long long)s0;
            en[rr] = (unsigned long long)tfr::list_lower_bound(a.items, s0, vhi, lo + width);
        }
    }
    wave_lds_sync();
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int nb = K - 64 * rr < 64 ? K - 64 * rr : 64;
        for (int z = 0; z < nb; ++z) {
            const int64_t zs = (int64_t)__shfl(st[rr], z), ze = (int64_t)__shfl(en[rr], z);
            const float zv = __shfl(sv[rr], z);
            if (zs == ze) continue;                      // an empty slot, or a neighbour with nothing in the slice
            for (int64_t t = zs + lane; t < ze; t += 64) A[(int64_t)a.items[t] - lo] += zv;
            wave_lds_sync();                             // this neighbour's adds stand before the next one's reads
        }
    }
    tfr::score_tail<MODE, KNN_SCORE_CAP>(a, A, queue[wave], qi, w, lo, width, lane);
}

template <int CAP>
__global__ __launch_bounds__(256) void k_uknn_query_cooc(UknnQueryArgs a) {
    __shared__ uint32_t counts[KNN_W_FIT];
    __shared__ uint64_t queue[KNN_WAVES][CAP];
    __shared__ int32_t wcnt[KNN_WAVES];
    static_assert(sizeof(counts) + sizeof(queue) + sizeof(wcnt) == knn_fit_lds(CAP), "uknn_plan reports another LDS size");
    static_assert(CAP >= KNN_KMAX + 64 || CAP == 256, "a queue must hold K plus one append");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.y, K = a.K;
    const int64_t lo = (int64_t)slice * KNN_W_FIT;
    const int width = (int)(a.n_users - lo < KNN_W_FIT ? a.n_users - lo : KNN_W_FIT);
    uint64_t* q = queue[wave];

    for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const int64_t p0 = a.qptr[a.row_lo + r], p1 = a.qptr[a.row_lo + r + 1];
        for (int t = tid; t < width; t += 256) counts[t] = 0;
        __syncthreads();

        tfr::count_row<KNN_WAVES>(a, counts, p0, p1, lo, width, lane, wave);
        __syncthreads();

        int qn = 0;
        uint64_t thr = 0;
        for (int base = wave * 64; base < width; base += 64 * KNN_WAVES) {
            const int j = base + lane;
            const uint32_t c = j < width ? counts[j] : 0u;
            const bool ok = c > 0;
            uint64_t key = 0;
            if (ok) key = topk_key(knn_sim(a.metric, c, p1 - p0, a.deg[lo + j + 1] - a.deg[lo + j], a.shrink), lo + j);
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

thread_local tfr::ErrText g_uknn_err;

// a chunk's per-slice keys into rows [r0, r0 + n_rows) of a [*, K] pair
int merge_rows(tfr_uknn* m, const KnnPlan& p, int32_t* ids, float* scores, int64_t r0, int64_t n_rows) {
    tfr::TopkMergeArgs mg;
    memset(&mg, 0, sizeof(mg));
    mg.part = m->part; mg.items_out = ids + r0 * m->K; mg.scores_out = scores + r0 * m->K;
    mg.n_rows = n_rows; mg.k = m->K; mg.slices = p.slices;
    tfr::launch_topk_merge(mg, m->stream);
    LISTCHK(g_uknn_err, hipGetLastError());
    return TFR_OK;
}

// what the serving drivers of item_lists.h ask of a family
struct UknnServe {
    using Model = tfr_uknn;
    using Args = UknnScoreArgs;
    using Plan = KnnPlan;
    static constexpr auto plan = uknn_plan;
    static constexpr const char* load_fn = "tfr_uknn_load";
    static constexpr const char* not_fitted = "no neighbours: call tfr_uknn_fit or tfr_uknn_set_neighbours first";

    static Args args(const Model* m) {
        Args a = {};
        a.nb_users = m->serving_lists ? m->q_nb_users : m->nb_users;
        a.nb_scores = m->serving_lists ? m->q_nb_scores : m->nb_scores;
        a.pu = m->pu; a.items = m->items;
        a.K = m->K;
        return a;
    }

    template <int MODE>
    static void launch(const Args& a, hipStream_t s) {
        const dim3 g((unsigned)((a.n * a.slices + KNN_WAVES - 1) / KNN_WAVES));
        const int R = knn_rounds(a.K);
        void (*kernel)(UknnScoreArgs) = k_uknn_score<4, MODE>;
        if (R == 1) kernel = k_uknn_score<1, MODE>;
        if (R == 2) kernel = k_uknn_score<2, MODE>;
        hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, a);
    }

    // lists need the resident rows to search, not fitted lists
    static const char* lists_refuse(const Model* m) { return m->loaded ? nullptr : "no data: call tfr_uknn_load first"; }

    // the neighbours of the n staged lists among the resident users, into q_nb_*; the model's device is current
    static int lists_prepare(tfr::ErrText& err, Model* m, int64_t n) {
        KnnPlan p;
        if (!uknn_plan(2, m->n_users, m->K, n, &p)) return fail(err, TFR_ERR_ARG, "top-K of lists: no plan for the neighbour search");
        hipStream_t s = m->stream;
        LISTCHK(err, m->q_nb_users.reserve(n * m->K, s));
        LISTCHK(err, m->q_nb_scores.reserve(n * m->K, s));
        LISTCHK(err, m->part.reserve(p.chunk * p.slices * m->K, s));
        UknnQueryArgs a = {};
        a.qptr = m->q_ptr; a.iu = m->q_ids; a.pu = m->pi; a.items = m->iu; a.deg = m->pu; a.part = m->part;
        a.n_users = m->n_users; a.shrink = m->shrink; a.K = m->K; a.slices = p.slices; a.metric = m->metric;
        for (int64_t r0 = 0; r0 < n; r0 += p.chunk) {
            a.row_lo = r0;
            a.n_rows = n - r0 < p.chunk ? n - r0 : p.chunk;
            const dim3 g((unsigned)std::min<int64_t>(a.n_rows, KNN_GRID_ROWS), (unsigned)p.slices);
            hipLaunchKernelGGL(p.cap == 256 ? k_uknn_query_cooc<256> : k_uknn_query_cooc<512>, g, dim3(256), 0, s, a);
            LISTCHK(err, hipGetLastError());
            if (int rc = merge_rows(m, p, m->q_nb_users, m->q_nb_scores, r0, a.n_rows)) return rc;
        }
        return TFR_OK;
    }
};

// rows [row_lo, row_lo + n_rows) of the user x K lists
int user_window(const tfr_uknn* m, const char* who, int64_t row_lo, int64_t n_rows) {
    if (row_lo < 0 || n_rows < 0 || row_lo > m->n_users || n_rows > m->n_users - row_lo)
        return fail(g_uknn_err, TFR_ERR_ARG, "%s: rows [%lld, %lld + %lld) are not inside the %lld users", who, (long long)row_lo,
                    (long long)row_lo, (long long)n_rows, (long long)m->n_users);
    return TFR_OK;
}

}  // namespace

extern "C" {

const char* tfr_uknn_last_error(void) { return g_uknn_err.text; }

int tfr_uknn_plan(int64_t n_cols, int32_t k, int64_t n_rows, int32_t which, int32_t* slice_width, int32_t* slices, int64_t* row_chunk,
                  int64_t* lds_bytes, int32_t* look_ahead) {
    if (which < 0 || which > 2)
        return fail(g_uknn_err, TFR_ERR_ARG, "uknn plan: which must be 0 (fit), 1 (scoring) or 2 (neighbours of lists)");
    if (n_cols < 1 || n_cols > 0x7fffffffLL || n_rows < 0) return fail(g_uknn_err, TFR_ERR_ARG, "uknn plan: n_rows >= 0 and 1 <= n_cols < 2^31");
    if (int rc = check_k(g_uknn_err, "uknn plan", k)) return rc;
    KnnPlan p;
    if (!uknn_plan(which, n_cols, k, n_rows, &p))
        return fail(g_uknn_err, TFR_ERR_ARG, "uknn plan: %lld columns need more than %lld / k slices", (long long)n_cols, (long long)tfr::TOPK_MERGE_KEYS);
    if (slice_width) *slice_width = p.width;
    if (slices) *slices = p.slices;
    if (row_chunk) *row_chunk = p.chunk;
    if (lds_bytes) *lds_bytes = (int64_t)std::max(p.lds, tfr::topk_merge_lds(p.slices, k));
    if (look_ahead) *look_ahead = p.ahead;
    return TFR_OK;
}

int tfr_uknn_destroy(tfr_uknn* m) { return m ? tfr::destroy_handle(m, {m->ev0, m->ev1}) : TFR_OK; }

int tfr_uknn_create(tfr_uknn** out, int64_t n_users, int64_t n_items, int32_t K, int32_t metric, double shrink, int32_t device) {
    if (!out) return fail(g_uknn_err, TFR_ERR_ARG, "out is null");
    *out = nullptr;
    if (int rc = tfr::check_counts(g_uknn_err, n_users, n_items)) return rc;
    if (int rc = check_k(g_uknn_err, "create", K)) return rc;
    if (metric < KNN_COSINE || metric > KNN_COUNT) return fail(g_uknn_err, TFR_ERR_ARG, "metric must be 0 (cosine), 1 (jaccard) or 2 (count)");
    if (!(shrink >= 0.0) || !std::isfinite(shrink)) return fail(g_uknn_err, TFR_ERR_ARG, "shrink must be non-negative and finite");
    if (metric == KNN_COUNT && shrink != 0.0) return fail(g_uknn_err, TFR_ERR_ARG, "the count metric takes no shrink");
    KnnPlan p;
    if (!uknn_plan(0, n_users, K, n_users, &p))
        return fail(g_uknn_err, TFR_ERR_ARG, "%lld users at K %d need more than %lld / K slices", (long long)n_users, K, (long long)tfr::TOPK_MERGE_KEYS);
    tfr_uknn* m = nullptr;
    if (int rc = tfr::create_handle(g_uknn_err, "uknn_create", &m, n_users, n_items, device)) return rc;
    m->K = K; m->metric = metric; m->shrink = shrink;
    hipError_t e = m->nb_users.reserve(n_users * K, m->stream);
    if (e == hipSuccess) e = m->nb_scores.reserve(n_users * K, m->stream);
    if (e == hipSuccess) e = hipEventCreate(&m->ev0);
    if (e == hipSuccess) e = hipEventCreate(&m->ev1);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP;
        tfr_uknn_destroy(m);
        return fail(g_uknn_err, code, "uknn_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

// A load forgets the fitted neighbours (item_lists.h load_lists: `fitted`).
int tfr_uknn_load(tfr_uknn* m, const int64_t* indptr, const int32_t* items) {
    return tfr::load_lists(g_uknn_err, m, indptr, items, [] {});
}

// k_knn_cooc with the orientations swapped: a row is a user, its list the user's items, and the rows the list names are
// the item lists.  Per row chunk the kernel over (rows, slices), then the merge into the handle's lists; timed by events.
int tfr_uknn_fit(tfr_uknn* m, float* elapsed_ms) {
    if (!m) return fail(g_uknn_err, TFR_ERR_ARG, "null model");
    if (!m->loaded) return fail(g_uknn_err, TFR_ERR_STATE, "no data: call tfr_uknn_load first");
    KnnPlan p;
    if (!uknn_plan(0, m->n_users, m->K, m->n_users, &p)) return fail(g_uknn_err, TFR_ERR_ARG, "fit: no plan");
    LISTCHK(g_uknn_err, hipSetDevice(m->device));
    m->fitted = false;
    hipStream_t s = m->stream;
    LISTCHK(g_uknn_err, m->part.reserve(p.chunk * p.slices * m->K, s));
    (void)hipEventRecord(m->ev0, s);
    KnnFitArgs a = {};
    a.shrink = m->shrink; a.metric = m->metric;
    a.pi = m->pu; a.iu = m->items; a.pu = m->pi; a.items = m->iu; a.part = m->part;
    a.n_items = m->n_users; a.K = m->K; a.slices = p.slices;
    for (int64_t r0 = 0; r0 < m->n_users; r0 += p.chunk) {
        a.row_lo = r0;
        a.n_rows = m->n_users - r0 < p.chunk ? m->n_users - r0 : p.chunk;
        knn_launch_cooc(a, p.cap, dim3((unsigned)std::min<int64_t>(a.n_rows, KNN_GRID_ROWS), (unsigned)p.slices), s);
        LISTCHK(g_uknn_err, hipGetLastError());
        if (int rc = merge_rows(m, p, m->nb_users, m->nb_scores, r0, a.n_rows)) return rc;
    }
    (void)hipEventRecord(m->ev1, s);
    LISTCHK(g_uknn_err, hipStreamSynchronize(s));
    if (elapsed_ms) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, m->ev0, m->ev1) != hipSuccess) ms = 0.f;
        *elapsed_ms = ms;
    }
    m->fitted = true;
    return TFR_OK;
}

int tfr_uknn_get_neighbours(tfr_uknn* m, int64_t row_lo, int64_t n_rows, int32_t* users_out, float* scores_out) {
    if (!m) return fail(g_uknn_err, TFR_ERR_ARG, "null model");
    if (!m->fitted) return fail(g_uknn_err, TFR_ERR_STATE, "%s", UknnServe::not_fitted);
    if (int rc = user_window(m, "get_neighbours", row_lo, n_rows)) return rc;
    if (n_rows == 0) return TFR_OK;
    LISTCHK(g_uknn_err, hipSetDevice(m->device));
    const size_t off = (size_t)row_lo * m->K, cnt = (size_t)n_rows * m->K;
    if (users_out) LISTCHK(g_uknn_err, hipMemcpyAsync(users_out, m->nb_users.get() + off, cnt * 4, hipMemcpyDeviceToHost, m->stream));
    if (scores_out) LISTCHK(g_uknn_err, hipMemcpyAsync(scores_out, m->nb_scores.get() + off, cnt * 4, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_uknn_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

// Rows [row_lo, row_lo + n_rows) of the neighbour lists from host arrays.  Checked before any device work.  The rows not
// named keep what they hold; on a handle without lists they are set empty first.
int tfr_uknn_set_neighbours(tfr_uknn* m, int64_t row_lo, int64_t n_rows, const int32_t* users, const float* scores) {
    if (!m) return fail(g_uknn_err, TFR_ERR_ARG, "null model");
    if (int rc = user_window(m, "set_neighbours", row_lo, n_rows)) return rc;
    if (n_rows > 0 && (!users || !scores)) return fail(g_uknn_err, TFR_ERR_ARG, "set_neighbours: null users or scores");
    const int K = m->K;
    std::vector<int32_t> seen;
    for (int64_t r = 0; r < n_rows; ++r) {
        seen.clear();
        for (int c = 0; c < K; ++c) {
            const int32_t v = users[r * K + c];
            if (v == -1) continue;
            if (v < -1 || v >= m->n_users) return fail(g_uknn_err, TFR_ERR_OOB, "set_neighbours: row %lld: id %d out of range", (long long)(row_lo + r), v);
            if (v == row_lo + r) return fail(g_uknn_err, TFR_ERR_ARG, "set_neighbours: row %lld lists itself", (long long)(row_lo + r));
            if (!std::isfinite(scores[r * K + c]))
                return fail(g_uknn_err, TFR_ERR_ARG, "set_neighbours: row %lld: the score of user %d is not finite", (long long)(row_lo + r), v);
            seen.push_back(v);
        }
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
            return fail(g_uknn_err, TFR_ERR_ARG, "set_neighbours: row %lld repeats a user", (long long)(row_lo + r));
    }
    LISTCHK(g_uknn_err, hipSetDevice(m->device));
    if (!m->fitted) {                                    // every row empty first: user -1 (every byte 0xff), score -inf
        const std::vector<float> pad((size_t)m->n_users * K, -INFINITY);
        LISTCHK(g_uknn_err, hipMemsetAsync(m->nb_users, 0xff, pad.size() * 4, m->stream));
        LISTCHK(g_uknn_err, hipMemcpy(m->nb_scores, pad.data(), pad.size() * 4, hipMemcpyHostToDevice));
    }
    if (n_rows > 0) {
        const size_t off = (size_t)row_lo * K, cnt = (size_t)n_rows * K;
        LISTCHK(g_uknn_err, hipMemcpyAsync(m->nb_users.get() + off, users, cnt * 4, hipMemcpyHostToDevice, m->stream));
        LISTCHK(g_uknn_err, hipMemcpyAsync(m->nb_scores.get() + off, scores, cnt * 4, hipMemcpyHostToDevice, m->stream));
    }
    LISTCHK(g_uknn_err, hipStreamSynchronize(m->stream));
    m->fitted = true;
    return TFR_OK;
}

int tfr_uknn_topk(tfr_uknn* m, const int32_t* users, int64_t n, int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                  int32_t* items_out, float* scores_out) {
    return tfr::topk_users<UknnServe>(g_uknn_err, m, users, n, k, excl_indptr, excl_items, items_out, scores_out);
}

// The lists' neighbours are searched first (UknnServe::lists_prepare); while the call runs the scoring reads them, row q.
int tfr_uknn_topk_lists(tfr_uknn* m, const int64_t* list_indptr, const int32_t* list_items, int64_t n, int32_t k,
                        const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    KnnPlan p;                                           // the scoring's plan, before the neighbour search does device work
    if (m && n > 0 && k >= 1 && k <= KNN_KMAX && m->loaded && !uknn_plan(1, m->n_items, k, n, &p))
        return fail(g_uknn_err, TFR_ERR_ARG, "top-K of lists: no plan for k %d over %lld items (slices * k <= %lld)", k, (long long)m->n_items,
                    (long long)tfr::TOPK_MERGE_KEYS);
    if (m) m->serving_lists = true;
    const int rc =tfr::topk_lists<UknnServe>(g_uknn_err, m, list_indptr, list_items, n, k, excl_indptr, excl_items, items_out, scores_out);
    if (m) m->serving_lists = false;
    return rc;
}

int tfr_uknn_rank_items(tfr_uknn* m, const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
                        const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    return tfr::rank_users<UknnServe>(g_uknn_err, m, users, n, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

}  // extern "C"
