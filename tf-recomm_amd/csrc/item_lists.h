// item_lists.h - what the item x item models share (ItemKNN: itemknn.{h,hip}; EASE: ease.{h,hip}, §32; SLIM:
// slim.{h,hip}, §34, which serves through EASE's scoring launches; the layer itself: §33).  They start from one binary user x
// item CSR and its transpose, and serve the same way: a wave holds one (query, catalogue slice) row of float32 scores in LDS,
// and the same tail turns that row into top-K keys or ranks.
//
// Device side: the binary search and the co-occurrence count loop of the fit kernels (uint32 counts, and uint64 sums of user
// weights for ItemKNN's weighted fit, §35), the per-wave key queue, and the scoring tail.  They are templated on the calling kernel's own argument block and read the fields both blocks name alike.
// Host side: the handle's base (ItemListModel), the error text, the CSR / user / k / window checks, the staging of a host CSR,
// the load, the shared ends of create and destroy, and the three serving bodies behind tfr_{knn,ease}_{topk,topk_lists,
// rank_items}.  A family describes itself to the serving bodies with a struct F:
//     Model, Args, Plan        its handle (derived from ItemListModel), its scoring argument block and its plan
//     plan                     (which, n_items, k, n_rows, Plan*) -> bool; the bodies use Plan::slices and Plan::chunk
//     load_fn, not_fitted      what the state messages name
//     args(const Model*)       an argument block with the model's own fields set
//     launch<MODE>(Args, s)    the scoring launch of a mode (0 top-K, 1 target keys, 2 rank counts)
// and, only where the lists of unknown users need work of the family's own before they are scored (UserKNN, userknn.{h,hip},
// §36: their neighbours are searched among the resident users), the pair ListsHook finds:
//     lists_refuse(const Model*)          NULL, or why top-K of lists cannot run in this state (default: not fitted)
//     lists_prepare(err, Model*, n)       after the n lists are staged in q_ptr / q_ids, before the scoring (default: nothing)
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <new>
#include <type_traits>
#include <vector>
#include "tfrecomm.h"
#include "devbuf.h"
#include "score_tile.h"
#include "topk.h"

namespace tfr {

// ---- device ------------------------------------------------------------------------------------------------------------------

// first position in the increasing x[lo, hi) whose value is not below v
__device__ __forceinline__ int64_t list_lower_bound(const int32_t* x, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)x[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// counts[j - lo] += users that item list [p0, p1) of a.iu shares with column j, for the columns [lo, lo + width): each of
// the block's WAVES waves takes 64 users at a time, lane l finds the part of user l's row inside the slice, then the wave
// walks the 64 parts.  Integer LDS atomics: exact in any order.  The caller zeroes the counters before and bars after.
template <int WAVES, class Args>
__device__ __forceinline__ void count_row(const Args& a, uint32_t* counts, int64_t p0, int64_t p1, int64_t lo, int width, int lane,
                                          int wave) {
    for (int64_t b = p0 + wave * 64; b < p1; b += 64 * WAVES) {
        unsigned long long st = 0, en = 0;
        if (b + lane < p1) {
            const int32_t u = a.iu[b + lane];
            const int64_t ulo = a.pu[u], uhi = a.pu[u + 1];
            const int64_t s0 = list_lower_bound(a.items, ulo, uhi, lo);
            st = (unsigned long long)s0;
            en = (unsigned long long)list_lower_bound(a.items, s0, uhi, lo + width);
        }
        const int nb = (int)(p1 - b < 64 ? p1 - b : 64);
        for (int z = 0; z < nb; ++z) {
            const int64_t zs = (int64_t)__shfl(st, z), ze = (int64_t)__shfl(en, z);
            for (int64_t t = zs + lane; t < ze; t += 64) atomicAdd(&counts[(int64_t)a.items[t] - lo], 1u);
        }
    }
}

// The weighted sibling: sums[j - lo] += a.uw[u] over the users u that the item list shares with column j.  The lane that
// loads user l's row bounds loads its uint64 weight too, and the three travel together by __shfl; a user of weight 0 is
// not walked.  64-bit integer LDS atomics: the sums are exact in any order as long as none reaches 2^64.
template <int WAVES, class Args>
__device__ __forceinline__ void count_row(const Args& a, unsigned long long* sums, int64_t p0, int64_t p1, int64_t lo, int width,
                                          int lane, int wave) {
    for (int64_t b = p0 + wave * 64; b < p1; b += 64 * WAVES) {
        unsigned long long st = 0, en = 0, wt = 0;
        if (b + lane < p1) {
            const int32_t u = a.iu[b + lane];
            wt = a.uw[u];
            const int64_t ulo = a.pu[u], uhi = a.pu[u + 1];
            const int64_t s0 = list_lower_bound(a.items, ulo, uhi, lo);
            st = (unsigned long long)s0;
            en = (unsigned long long)list_lower_bound(a.items, s0, uhi, lo + width);
        }
        const int nb = (int)(p1 - b < 64 ? p1 - b : 64);
        for (int z = 0; z < nb; ++z) {
            const unsigned long long zw = __shfl(wt, z);
            if (zw == 0) continue;
            const int64_t zs = (int64_t)__shfl(st, z), ze = (int64_t)__shfl(en, z);
            for (int64_t t = zs + lane; t < ze; t += 64) atomicAdd(&sums[(int64_t)a.items[t] - lo], zw);
        }
    }
}

// The per-wave key queue: q is the wave's own LDS, cnt and thr are wave-uniform registers.
// sort the wave's queue, keep its k best, raise its threshold
template <int CAP>
__device__ __forceinline__ void queue_compact(uint64_t* q, int& cnt, uint64_t& thr, int k, int lane) {
    for (int t = cnt + lane; t < CAP; t += 64) q[t] = 0;
    wave_lds_sync();
    wave_sort_desc<CAP>(q, lane);
    cnt = cnt < k ? cnt : k;
    thr = cnt == k ? q[k - 1] : 0;
}

// each lane offers one key; needs cnt <= CAP - 64 on entry and leaves it so
template <int CAP>
__device__ __forceinline__ void queue_offer(uint64_t* q, int& cnt, uint64_t& thr, int k, int lane, bool ok, uint64_t key) {
    ok = ok && key > thr;
    const uint64_t mask = __ballot(ok);
    if (mask) {
        if (ok) q[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = key;
        cnt += __popcll(mask);
        if (cnt > CAP - 64) queue_compact<CAP>(q, cnt, thr, k, lane);
    }
}

// The tail of a scoring wave.  A: the wave's LDS row of scores for the columns [lo, lo + width) of query qi, complete and
// visible to the wave; q: its queue of CAP keys; w: its index among the launch's waves, (query of the chunk) * slices + slice.
// Excluded columns are overwritten with NaN, which no sum of finite scores gives.  MODE 0 (top-K): scan, keys, queue,
// part[w].  MODE 1 (ranking): the targets inside the slice get their key.  MODE 2: lane t counts the slots of the slice
// whose key beats target t's; the slices' counts meet in an integer atomic.
template <int MODE, int CAP, class Args>
__device__ __forceinline__ void score_tail(const Args& a, float* A, uint64_t* q, int64_t qi, int64_t w, int64_t lo, int width, int lane) {
    if (a.xptr) {
        const int64_t x0 = a.xptr[qi], x1 = a.xptr[qi + 1];
        for (int64_t t = x0 + lane; t < x1; t += 64) {
            const int64_t col = (int64_t)a.xids[t] - lo;
            if (col >= 0 && col < width) A[col] = __builtin_nanf("");
        }
        wave_lds_sync();
    }

    if (MODE == 0) {
        int qn = 0;
        uint64_t thr = 0;
        for (int base = 0; base < width; base += 64) {
            const int j = base + lane;
            const float v = j < width ? A[j] : __builtin_nanf("");
            const bool ok = !__builtin_isnan(v);
            queue_offer<CAP>(q, qn, thr, a.k, lane, ok, ok ? topk_key(v, lo + j) : 0);
        }
        if (qn > 0) queue_compact<CAP>(q, qn, thr, a.k, lane);
        uint64_t* dst = a.part + (size_t)w * a.k;
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

// ---- host: error text ------------------------------------------------------------------------------------------------------

// A family's last error.  Each family keeps a thread_local one of its own and hands it to the shared code by reference.
struct ErrText { char text[512] = ""; };

inline int fail(ErrText& err, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err.text, sizeof(err.text), fmt, ap);
    va_end(ap);
    return code;
}

#define LISTCHK(err, expr)                                                                                  \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return tfr::fail(err, e_ == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, \
                                               "%s: %s", #expr, hipGetErrorString(e_));                     \
    } while (0)

// ---- host: the handle's base -------------------------------------------------------------------------------------------------

struct ItemListModel {
    int64_t n_users = 0, n_items = 0;
    int device = 0;
    bool loaded = false, fitted = false;
    hipStream_t stream = nullptr;
    DevBuf<int64_t> pu, pi;                              // [n_users + 1], [n_items + 1]
    DevBuf<int32_t> items, iu;                           // the CSR as loaded and its transpose
    DevBuf<uint64_t> part, tkeys;
    // one call's staged inputs and outputs
    DevBuf<int32_t> q_users, q_ids, x_ids, t_ids, out_items, ranks;
    DevBuf<int64_t> q_ptr, x_ptr, t_ptr;
    DevBuf<float> out_scores;
};

// ---- host: checks and staging ------------------------------------------------------------------------------------------------

// a CSR of n rows over ids in [0, bound): indptr from `from0 ? 0 : anything >= 0` and non-decreasing, rows strictly
// increasing (`strict`) or non-decreasing.  TFR_OK, or the code with the message set.
inline int check_csr(ErrText& err, const char* who, const char* what, bool from0, bool strict, const int64_t* indptr, const int32_t* ids,
                     int64_t n, int64_t bound) {
    if (!indptr) return fail(err, TFR_ERR_ARG, "%s: null %s indptr", who, what);
    if (from0 ? indptr[0] != 0 : indptr[0] < 0) return fail(err, TFR_ERR_ARG, "%s: %s indptr must start at 0", who, what);
    for (int64_t r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) return fail(err, TFR_ERR_ARG, "%s: %s indptr decreases at row %lld", who, what, (long long)r);
    if (indptr[n] > indptr[0] && !ids) return fail(err, TFR_ERR_ARG, "%s: %s indptr without ids", who, what);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            if (ids[e] < 0 || ids[e] >= bound)
                return fail(err, TFR_ERR_OOB, "%s: %s row %lld: id %d out of range", who, what, (long long)r, ids[e]);
            if (e > indptr[r] && (strict ? ids[e] <= ids[e - 1] : ids[e] < ids[e - 1]))
                return fail(err, TFR_ERR_ARG, "%s: %s row %lld is not %s", who, what, (long long)r,
                            strict ? "strictly increasing" : "non-decreasing");
        }
    return TFR_OK;
}

inline int check_users(ErrText& err, const char* who, const ItemListModel* m, const int32_t* users, int64_t n) {
    if (!users) return fail(err, TFR_ERR_ARG, "%s: null users", who);
    for (int64_t q = 0; q < n; ++q)
        if (users[q] < 0 || users[q] >= m->n_users) return fail(err, TFR_ERR_OOB, "%s: user id %d out of range", who, users[q]);
    return TFR_OK;
}

inline int check_k(ErrText& err, const char* who, int32_t k) {
    return k < 1 || k > TOPK_KMAX ? fail(err, TFR_ERR_ARG, "%s: k must be in [1, %d] (got %d)", who, TOPK_KMAX, k) : TFR_OK;
}

// rows [row_lo, row_lo + n_rows) of an item x something matrix
inline int window(ErrText& err, const ItemListModel* m, const char* who, int64_t row_lo, int64_t n_rows) {
    if (row_lo < 0 || n_rows < 0 || row_lo > m->n_items || n_rows > m->n_items - row_lo)
        return fail(err, TFR_ERR_ARG, "%s: rows [%lld, %lld + %lld) are not inside the %lld items", who, (long long)row_lo,
                    (long long)row_lo, (long long)n_rows, (long long)m->n_items);
    return TFR_OK;
}

// a host CSR onto the device: indptr as it stands, the ids [0, indptr[n])
inline int stage_csr(ErrText& err, ItemListModel* m, DevBuf<int64_t>& dp, DevBuf<int32_t>& di, const int64_t* indptr, const int32_t* ids,
                     int64_t n) {
    LISTCHK(err, dp.reserve(n + 1, m->stream));
    LISTCHK(err, di.reserve(std::max<int64_t>(1, indptr[n]), m->stream));
    LISTCHK(err, hipMemcpyAsync(dp, indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, m->stream));
    if (indptr[n] > 0) LISTCHK(err, hipMemcpyAsync(di, ids, (size_t)indptr[n] * 4, hipMemcpyHostToDevice, m->stream));
    return TFR_OK;
}

// ---- host: create, destroy, load -----------------------------------------------------------------------------------------------

inline int check_counts(ErrText& err, int64_t n_users, int64_t n_items) {
    if (n_users < 1 || n_items < 1 || n_users > 0x7fffffffLL || n_items > 0x7fffffffLL)
        return fail(err, TFR_ERR_ARG, "need positive int32 user and item counts");
    return TFR_OK;
}

// The end of a create, after the family's own checks: the device, a handle of type M with the counts set, its stream.  On
// TFR_OK the device is current and *out is the handle; a family that fails later destroys it.  `who` names the create in
// the message of a stream that could not be made.
template <class M>
int create_handle(ErrText& err, const char* who, M** out, int64_t n_users, int64_t n_items, int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(err, TFR_ERR_HIP, "no HIP device available - this library has no CPU path");
    if (device < 0 || device >= ndev) return fail(err, TFR_ERR_ARG, "device %d not in [0,%d)", device, ndev);
    LISTCHK(err, hipSetDevice(device));
    M* m = new (std::nothrow) M();
    if (!m) return fail(err, TFR_ERR_NOMEM, "host allocation failed");
    m->n_users = n_users; m->n_items = n_items; m->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete m;
        return fail(err, e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

// m is not null.  The buffers are freed with the model's device current, after its stream has drained.
template <class M>
int destroy_handle(M* m, std::initializer_list<hipEvent_t> events) {
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (hipEvent_t e : events)
        if (e) (void)hipEventDestroy(e);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return TFR_OK;
}

// The user CSR.  Everything is checked and the transpose built on the host before any device work, so a refused load
// leaves the model as it was.  Past that the model forgets what it was fitted to - `loaded`, `fitted`, and what the
// family's `forget` clears - before the first copy.
// `item_ptr`, where given, receives the item lists' indptr [n_items + 1] on TFR_OK (a family that plans from it).
template <class Forget>
int load_lists(ErrText& err, ItemListModel* m, const int64_t* indptr, const int32_t* items, Forget forget,
               std::vector<int64_t>* item_ptr = nullptr) {
    if (!m) return fail(err, TFR_ERR_ARG, "null model");
    const int64_t nu = m->n_users, ni = m->n_items;
    if (int rc = check_csr(err, "load", "user", true, true, indptr, items, nu, ni)) return rc;
    const int64_t nnz = indptr[nu];
    // the item-major orientation: users ascend inside each item's list because the rows are walked in order
    std::vector<int64_t> pi((size_t)ni + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) pi[(size_t)items[e] + 1]++;
    for (int64_t i = 0; i < ni; ++i) pi[(size_t)i + 1] += pi[(size_t)i];
    std::vector<int64_t> cur(pi.begin(), pi.end() - 1);
    std::vector<int32_t> iu((size_t)nnz);
    for (int64_t u = 0; u < nu; ++u)
        for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) iu[(size_t)cur[(size_t)items[e]]++] = (int32_t)u;

    LISTCHK(err, hipSetDevice(m->device));
    LISTCHK(err, hipStreamSynchronize(m->stream));
    m->loaded = false;
    m->fitted = false;
    forget();
    const int64_t cap = std::max<int64_t>(1, nnz);
    LISTCHK(err, m->pu.reserve(nu + 1, m->stream));
    LISTCHK(err, m->pi.reserve(ni + 1, m->stream));
    LISTCHK(err, m->items.reserve(cap, m->stream));
    LISTCHK(err, m->iu.reserve(cap, m->stream));
    LISTCHK(err, hipMemcpy(m->pu, indptr, (size_t)(nu + 1) * 8, hipMemcpyHostToDevice));
    LISTCHK(err, hipMemcpy(m->pi, pi.data(), pi.size() * 8, hipMemcpyHostToDevice));
    if (nnz) {
        LISTCHK(err, hipMemcpy(m->items, items, (size_t)nnz * 4, hipMemcpyHostToDevice));
        LISTCHK(err, hipMemcpy(m->iu, iu.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
    }
    if (item_ptr) item_ptr->swap(pi);
    m->loaded = true;
    return TFR_OK;
}

// ---- host: serving -------------------------------------------------------------------------------------------------------------

// the query side of an argument block: the resident rows named by staged users, or staged lists
struct ListQuery { const int32_t* users; const int64_t* ptr; const int32_t* ids; };

template <class F>
typename F::Args score_args(const typename F::Model* m, const ListQuery& q) {
    typename F::Args a = F::args(m);
    a.users = q.users; a.ptr = q.ptr; a.ids = q.ids;
    a.n_items = m->n_items;
    return a;
}

// top-K of n queries whose lists are on the device; the exclusion CSR is the host's, already checked
template <class F>
int topk_run(ErrText& err, typename F::Model* m, const char* who, const ListQuery& q, int64_t n, int32_t k, const int64_t* xip,
             const int32_t* xit, int32_t* items_out, float* scores_out) {
    typename F::Plan p;
    if (!F::plan(1, m->n_items, k, n, &p))
        return fail(err, TFR_ERR_ARG, "%s: no plan for k %d over %lld items (slices * k <= %lld)", who, k, (long long)m->n_items,
                    (long long)TOPK_MERGE_KEYS);
    hipStream_t s = m->stream;
    if (xip) if (int rc = stage_csr(err, m, m->x_ptr, m->x_ids, xip, xit, n)) return rc;
    LISTCHK(err, m->out_items.reserve(n * k, s));
    if (scores_out) LISTCHK(err, m->out_scores.reserve(n * k, s));
    LISTCHK(err, m->part.reserve(p.chunk * p.slices * k, s));
    typename F::Args a = score_args<F>(m, q);
    if (xip) { a.xptr = m->x_ptr; a.xids = m->x_ids; }
    a.part = m->part; a.k = k; a.slices = p.slices;
    for (int64_t c0 = 0; c0 < n; c0 += p.chunk) {
        a.q_lo = c0;
        a.n = n - c0 < p.chunk ? n - c0 : p.chunk;
        F::template launch<0>(a, s);
        LISTCHK(err, hipGetLastError());
        TopkMergeArgs g;
        memset(&g, 0, sizeof(g));
        g.part = m->part; g.items_out = m->out_items.get() + c0 * k;
        g.scores_out = scores_out ? m->out_scores.get() + c0 * k : nullptr;
        g.n_rows = a.n; g.k = k; g.slices = p.slices;
        launch_topk_merge(g, s);
        LISTCHK(err, hipGetLastError());
    }
    LISTCHK(err, hipMemcpyAsync(items_out, m->out_items, (size_t)n * k * 4, hipMemcpyDeviceToHost, s));
    if (scores_out) LISTCHK(err, hipMemcpyAsync(scores_out, m->out_scores, (size_t)n * k * 4, hipMemcpyDeviceToHost, s));
    LISTCHK(err, hipStreamSynchronize(s));
    return TFR_OK;
}

// the body of tfr_*_topk: resident users
template <class F>
int topk_users(ErrText& err, typename F::Model* m, const int32_t* users, int64_t n, int32_t k, const int64_t* excl_indptr,
               const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    if (!m) return fail(err, TFR_ERR_ARG, "null model");
    if (n < 0) return fail(err, TFR_ERR_ARG, "top-K: negative n");
    if (int rc = check_k(err, "top-K", k)) return rc;
    if (!m->loaded) return fail(err, TFR_ERR_STATE, "top-K: no data: call %s first", F::load_fn);
    if (!m->fitted) return fail(err, TFR_ERR_STATE, "top-K: %s", F::not_fitted);
    if (n == 0) return TFR_OK;
    if (!items_out) return fail(err, TFR_ERR_ARG, "top-K: null items_out");
    if (int rc = check_users(err, "top-K", m, users, n)) return rc;
    if (excl_indptr) if (int rc = check_csr(err, "top-K", "exclusion", false, false, excl_indptr, excl_items, n, m->n_items)) return rc;
    LISTCHK(err, hipSetDevice(m->device));
    LISTCHK(err, m->q_users.reserve(n, m->stream));
    LISTCHK(err, hipMemcpyAsync(m->q_users, users, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    return topk_run<F>(err, m, "top-K", ListQuery{m->q_users, m->pu, m->items}, n, k, excl_indptr, excl_items, items_out, scores_out);
}

// what top-K of lists asks of the state, and what runs between the staging of the lists and their scoring: a fitted model
// and nothing, unless the family names lists_refuse and lists_prepare
template <class F, class = void>
struct ListsHook {
    static const char* refuse(const typename F::Model* m) { return m->fitted ? nullptr : F::not_fitted; }
    static int prepare(ErrText&, typename F::Model*, int64_t) { return TFR_OK; }
};
template <class F>
struct ListsHook<F, std::void_t<decltype(&F::lists_prepare)>> {
    static const char* refuse(const typename F::Model* m) { return F::lists_refuse(m); }
    static int prepare(ErrText& err, typename F::Model* m, int64_t n) { return F::lists_prepare(err, m, n); }
};

// the body of tfr_*_topk_lists: users known by their lists alone; needs no load
template <class F>
int topk_lists(ErrText& err, typename F::Model* m, const int64_t* list_indptr, const int32_t* list_items, int64_t n, int32_t k,
               const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    if (!m) return fail(err, TFR_ERR_ARG, "null model");
    if (n < 0) return fail(err, TFR_ERR_ARG, "top-K of lists: negative n");
    if (int rc = check_k(err, "top-K of lists", k)) return rc;
    if (const char* why = ListsHook<F>::refuse(m)) return fail(err, TFR_ERR_STATE, "top-K of lists: %s", why);
    if (n == 0) return TFR_OK;
    if (!items_out) return fail(err, TFR_ERR_ARG, "top-K of lists: null items_out");
    if (int rc = check_csr(err, "top-K of lists", "list", true, true, list_indptr, list_items, n, m->n_items)) return rc;
    if (excl_indptr)
        if (int rc = check_csr(err, "top-K of lists", "exclusion", false, false, excl_indptr, excl_items, n, m->n_items)) return rc;
    LISTCHK(err, hipSetDevice(m->device));
    if (int rc = stage_csr(err, m, m->q_ptr, m->q_ids, list_indptr, list_items, n)) return rc;
    if (int rc = ListsHook<F>::prepare(err, m, n)) return rc;
    return topk_run<F>(err, m, "top-K of lists", ListQuery{nullptr, m->q_ptr, m->q_ids}, n, k, excl_indptr, excl_items, items_out, scores_out);
}

// the body of tfr_*_rank_items: the targets' keys, then per target the count of keys above its own
template <class F>
int rank_users(ErrText& err, typename F::Model* m, const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
               const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    if (!m) return fail(err, TFR_ERR_ARG, "null model");
    if (n < 0) return fail(err, TFR_ERR_ARG, "rank: negative n");
    if (!m->loaded) return fail(err, TFR_ERR_STATE, "rank: no data: call %s first", F::load_fn);
    if (!m->fitted) return fail(err, TFR_ERR_STATE, "rank: %s", F::not_fitted);
    if (n == 0) return TFR_OK;
    if (int rc = check_users(err, "rank", m, users, n)) return rc;
    if (int rc = check_csr(err, "rank", "target", false, true, tgt_indptr, tgt_items, n, m->n_items)) return rc;
    if (excl_indptr) if (int rc = check_csr(err, "rank", "exclusion", false, false, excl_indptr, excl_items, n, m->n_items)) return rc;
    const int64_t t0 = tgt_indptr[0], n_tgt = tgt_indptr[n] - t0;
    if (n_tgt == 0) return TFR_OK;
    if (!ranks_out) return fail(err, TFR_ERR_ARG, "rank: null ranks_out");
    typename F::Plan p;                                  // the ranking merges nothing: only the slicing of the plan is used
    if (!F::plan(1, m->n_items, 1, n, &p)) return fail(err, TFR_ERR_ARG, "rank: no plan");
    LISTCHK(err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    LISTCHK(err, m->q_users.reserve(n, s));
    LISTCHK(err, hipMemcpyAsync(m->q_users, users, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (int rc = stage_csr(err, m, m->t_ptr, m->t_ids, tgt_indptr, tgt_items, n)) return rc;
    if (excl_indptr) if (int rc = stage_csr(err, m, m->x_ptr, m->x_ids, excl_indptr, excl_items, n)) return rc;
    LISTCHK(err, m->tkeys.reserve(tgt_indptr[n], s));
    LISTCHK(err, m->ranks.reserve(tgt_indptr[n], s));
    typename F::Args a = score_args<F>(m, ListQuery{m->q_users, m->pu, m->items});
    if (excl_indptr) { a.xptr = m->x_ptr; a.xids = m->x_ids; }
    a.tptr = m->t_ptr; a.tids = m->t_ids; a.tkeys = m->tkeys; a.ranks = m->ranks;
    a.q_lo = 0; a.n = n; a.k = 1; a.slices = p.slices;
    F::template launch<1>(a, s);
    LISTCHK(err, hipGetLastError());
    F::template launch<2>(a, s);
    LISTCHK(err, hipGetLastError());
    LISTCHK(err, hipMemcpyAsync(ranks_out, m->ranks.get() + t0, (size_t)n_tgt * 4, hipMemcpyDeviceToHost, s));
    LISTCHK(err, hipStreamSynchronize(s));
    return TFR_OK;
}

}  // namespace tfr
