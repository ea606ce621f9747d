// api.hip - the C-ABI of include/tfrecomm.h over the kernels in svd_kernels.hip.
// Host-side orchestration of one minibatch (svd_train_val.py:66-72):
//   K1 forward+loss+g  ->  key sorts (user ids, item ids)  ->  item-side segmented reduce
//   -> user-side segmented reduce (+ fused lazy Adam / SGD)  ->  item apply  ->  finalize
// or, in TF1 Adam mode, both reduces to scratch followed by the dense sweeps.
#include <hip/hip_runtime.h>
#include <utility>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <math.h>
#include <new>
#include <chrono>
#include <vector>
#include <algorithm>
#include "tfrecomm.h"
#include "svd_kernels.h"
#include "topk.h"
#include "neighbours.h"
#include "rank.h"
#include "finetune.h"
#include "bf16_rows.h"
#include "fm_bf16.h"
#include "devbuf.h"

using namespace tfr;

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, "%s: %s",   \
                        #expr, hipGetErrorString(e_));                                       \
    } while (0)

struct ProfEvent { hipEvent_t a, b; int kid; };

// an id buffer of the resident-store steps, with the store records of its leading n_recs ids beside it: left there by the
// stream that filled the ids (in stream order before their chunk's event), so that the small-table step's sorts read one
// record per id instead of ids -> store.  Reallocating or rewriting the ids clears n_recs.
struct IdBuf {
    DevBuf<int64_t> ids;
    DevBuf<int4> recs;
    int64_t n_recs = 0;
};

struct BprState;                                        // bpr_api.inc.h

struct tfr_model {
    int64_t U = 0, I = 0;
    int32_t D = 0, G = 0, VEC = 0;
    int bits_u = 1, bits_i = 1;
    tfr_opts o;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // tables: index TFR_MU..TFR_Q; slots m, v
    DevBuf<float> w[5], m[5], v[5];
    int64_t n[5] = {0, 0, 0, 0, 0};
    uint32_t frozen = 0;
    int64_t step = 0;
    float b1p = 0.f, b2p = 0.f;
    // batch workspace
    int64_t cap = 0;
    DevBuf<int32_t> d_u, d_i;
    DevBuf<float> d_r, d_logits, d_g;
    DevBuf<int32_t> ks_u, ps_u, ks_i, ps_i;
    DevBuf<int32_t> ks2_u, ps2_u, ks2_i, ps2_i;   // rsort ping-pong
    DevBuf<int32_t> lrank_u, lrank_i, hist_u, hist_i;   // csort
    DevBuf<int32_t> offs_u, offs_i, binbase_u, binbase_i;
    DevBuf<int32_t> blocktot_u, blocktot_i;
    // two-table form of the fused big-table step (RedArgs::sel): the alternate item table, the per-row "which table" word,
    // the per-entry {partner row | old table} words of the current batch; q_dirty = some row may live in q_alt
    DevBuf<float> q_alt; DevBuf<int32_t> q_sel, osel; bool q_dirty = false;
    DevBuf<float> gq, gp, gbq, gbp;
    DevBuf<int32_t> map_u, map_i;
    DevBuf<float> dg_p, dg_q, dg_bu, dg_bi;   // tf1: dense per-row gradients
    DevBuf<float> partials;
    DevBuf<float> scalars;            // {loss, reg, sum_g, -}
    DevBuf<float> step_out;           // per-step {loss, reg, sum_g} ring for multi-step calls
    DevBuf<int32_t> d_err;
    DevBuf<unsigned long long> d_auc;   // {2 x rank sum of the positives, number of positives}
    const float* last_r = nullptr; int64_t last_B = 0;     // rates of the last host-fed training batch whose logits were kept
    // host-fed calls (tfr_train_step / tfr_forward): one pinned staging buffer each way, so a step is one
    // H2D copy, the kernels and one D2H copy instead of five pageable transfers
    DevBuf<int32_t> d_in; HostBuf<int32_t> h_in; HostBuf<float> h_out;
    HostBuf<int32_t> h_err;                                  // pinned landing place of the device error flag
    // look-ahead of the small-table step: the next batch's tile sort, published by the previous launch
    DevBuf<int4> srt[2][2];                                      // [parity][side] sorted records {u, i, r, pos}
    const int64_t* pf_ids = nullptr; int64_t pf_B = 0; int pf_par = 0; bool pf_valid = false;
    const int64_t* dp_next_ids = nullptr;                        // tfr_dp_hint_next: batch of the next tfr_dp_local_grads
    DevBuf<unsigned long long> tile_dbg;                         // TFR_TILE_DEBUG=1: per-block stamps of k_tile_step
    // big-table look-ahead: the next batch is gathered and sorted on a second stream into the alternate
    // set of batch buffers while this step's bandwidth-bound kernels run
    struct SortSet { DevBuf<int32_t> d_u, d_i; DevBuf<float> d_r; DevBuf<int32_t> ks_u, ps_u, ks_i, ps_i; } alt;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_sorted[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr}, ev_first = nullptr;
    // tfr_draw_ids_dev / tfr_join_draws / tfr_join_draw: one event per issued draw (ring; draws complete in issue order)
    static const int DRAW_RING = 8;
    hipEvent_t draw_evs[DRAW_RING] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t draw_count = 0, draw_joined = 0;
    // wide form of the id draw (rng.hip), allocated with the generator state; rng_ws points into the three buffers
    DevBuf<uint32_t> rng_raw; DevBuf<int32_t> rng_counts, rng_hdr;
    MtScratch rng_ws = {nullptr, nullptr, nullptr, 0};
    hipEvent_t ev_mid = nullptr; bool ev_mid_on = false;   // recorded between the item-side and the user-side kernel of a big-table step
    // resident store
    DevBuf<int4> store;               // {user, item, rate bits, -} per rating
    int64_t N = 0;
    IdBuf ids;                        // staged / drawn ids of the resident-store steps
    int64_t n_ids = 0;
    // device id draw (rng.hip): NumPy's MT19937 state {key[624], pos}; draws run on their own stream, ahead
    // of the steps that consume them; one event per drawn chunk
    DevBuf<uint32_t> d_rng;
    bool rng_set = false;
    // run-ahead between calls: after a drawn call the generator goes on into the alternate id buffer, so the next
    // call with the same batch size starts on ids that are already there; anything else that looks at the generator
    // first puts it back to the snapshot taken where the consumed ids end
    IdBuf ids_alt;
    DevBuf<uint32_t> d_rng_snap;
    bool spec_valid = false; int64_t spec_B = 0, spec_N = 0, spec_steps = 0;
    hipEvent_t spec_ev = nullptr;
    hipStream_t stream3 = nullptr;
    std::vector<hipEvent_t> chunk_ev;
    hipEvent_t ev_ids_free = nullptr;
    // host-drawn ids, one step at a time, without a host sync: pinned ring + device ring
    static const int HRING = 4;
    HostBuf<int64_t> h_ring; DevBuf<int64_t> d_ring; int64_t ring_cap = 0; int ring_pos = 0;
    hipEvent_t ring_ev[HRING] = {nullptr, nullptr, nullptr, nullptr};
    // row-sharded step: the routed local batch (tfr_shard_route)
    // Two sets, so that a caller can route (and pre-sort) batch s+1 on a side stream while step s still reads its own:
    // tfr_shard_select picks the set the shard calls fill and consume.
    struct RouteSet {
        DevBuf<int32_t> mine, u, it, slot, counts;
        DevBuf<float> r;
        int64_t B = 0, slots = 0;
        int32_t world = 0;
        // sorted orders: of the routed samples by local user row / by request slot (forward + reduce), made by tfr_shard_presort
        // ahead of time or by the step itself; of the requests received as an owner (apply_items)
        DevBuf<int32_t> ks_u, ps_u, ks_i, ps_i;
        DevBuf<int32_t> akeys, aks, aps;
        bool sorted_fwd = false; const int32_t* sorted_req = nullptr; int64_t sorted_req_n = 0;
        const int32_t *fks_u = nullptr, *fps_u = nullptr, *fks_i = nullptr, *fps_i = nullptr;   // where the forward's sorted columns are
    } rt[2];
    int rt_sel = 0;
    // resident validation set (svd_train_val.py:33-38: the whole set is one batch)
    DevBuf<int32_t> ev_u, ev_i;
    DevBuf<float> ev_r;
    int64_t ev_n = 0;
    // top-K (tfr_topk*): the (row, item slice) key lists of one user chunk, the host entries' staged chunk inputs / outputs,
    // and the device entry's exclusion-check word
    DevBuf<uint64_t> tk_part;
    DevBuf<int32_t> tk_users;
    DevBuf<int64_t> tk_indptr;
    DevBuf<int32_t> tk_excl;
    DevBuf<int32_t> tk_items;
    DevBuf<float> tk_scores;
    DevBuf<int32_t> tk_bad;
    // nearest neighbours (tfr_neighbours*): the inverse row norms of item_features [0] and user_features [1], each with the
    // step counter and the table generation it was built at.  tab_gen counts what changes a table without a step (set_table,
    // init, set_step, set_frozen, a voided step); tab_exposed: tfr_table_devptr handed a table out, writes are unseen from then
    struct RnCache { DevBuf<float> rn; int64_t step = -1; uint64_t gen = 0; bool valid = false; } nb_rn[2];
    uint64_t tab_gen = 0;
    bool tab_exposed = false;
    // held-out ranking (tfr_rank_items*): one piece chunk's staged pieces, targets and exclusions, and its per-piece state
    DevBuf<RankPiece> rk_pieces;
    DevBuf<int32_t> rk_tgt, rk_excl, rk_ranks;
    DevBuf<uint64_t> rk_keys;
    DevBuf<int32_t> rk_order, rk_bins, rk_nr;
    // batched fine-tuning (tfr_finetune_users): one device buffer for a call's schedule and outputs
    DevBuf<char> ft_buf;
    // bf16 snapshot (tfr_bf16_*): P and Q as padded bf16 rows, mu and the biases as they were at the same moment
    // gen counts the snapshots made and dropped; rn: the inverse row norms of the snapshot's Q [0] and P [1]
    // (tfr_bf16_neighbours*), each valid for the snapshot generation it was built at - steps and tfr_set_table do not enter
    struct Bf16Snap {
        DevBuf<uint16_t> p, q; DevBuf<float> bu, bi, mu; bool valid = false;
        uint64_t gen = 0;
        struct Rn { DevBuf<float> rn; uint64_t gen = 0; bool valid = false; } rn[2];
        void drop() {
            p.reset(); q.reset(); bu.reset(); bi.reset(); mu.reset(); valid = false;
            for (Rn& r : rn) { r.rn.reset(); r.valid = false; }
            gen += 1;
        }
    } bf;
    // BPR steps (tfr_bpr_*): the positives, the sampler's settings and the step's buffers; created by the first BPR call
    BprState* bpr = nullptr;
    // WARP trainers (tfr_warp_*) bound to this model: tfr_destroy refuses while one is alive
    int32_t warp_live = 0;
    // profiling
    bool prof = false;
    std::vector<ProfEvent> events;
    double prof_ms[TFR_K_COUNT];
    int64_t prof_n[TFR_K_COUNT];
    float prof_overhead_ms = 0.f;     // elapsed time of an empty event pair on this stream
};

// ---------------------------------------------------------------------------------------
static int bits_for(int64_t rows) {
    int b = 1;
    while (((int64_t)1 << b) < rows && b < 31) ++b;
    return b;
}

// reserve n elements in each buffer of a group (stops at the first failure)
template <typename... Bufs>
static hipError_t reserve_each(int64_t n, hipStream_t s, Bufs&... b) {
    hipError_t e = hipSuccess;
    (void)((e = b.reserve(n, s), e == hipSuccess) && ...);
    return e;
}

// the growth policy of the batch-sized buffers: powers of two from 1024
static int64_t pow2_cap(int64_t n) {
    int64_t c = 1024;
    while (c < n) c <<= 1;
    return c;
}

struct Prof {
    tfr_model* m;
    int kid;
    hipEvent_t a = nullptr, b = nullptr;
    Prof(tfr_model* m_, int kid_) : m(m_), kid(kid_) {
        if (m->prof) {
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
            (void)hipEventRecord(a, m->stream);
        }
    }
    ~Prof() {
        if (a && b) {
            (void)hipEventRecord(b, m->stream);
            m->events.push_back({a, b, kid});
        }
    }
};

static int drain_profile(tfr_model* m) {
    if (m->events.empty()) return TFR_OK;
    HIPCHK(hipStreamSynchronize(m->stream));
    for (auto& e : m->events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            ms -= m->prof_overhead_ms;                   // what an empty start/stop pair measures
            if (ms < 0.f) ms = 0.f;
            m->prof_ms[e.kid] += ms;
            m->prof_n[e.kid] += 1;
        }
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    m->events.clear();
    return TFR_OK;
}

// Adam in TF1 mode: the reduce leaves every touched row's sum in scratch, a dense sweep moves every row
static bool tf1_mode(const tfr_model* m) { return m->o.optimizer == TFR_OPT_ADAM && m->o.adam_mode == TFR_ADAM_TF1; }

// small tables: the bins of both id columns fit the counting sort's LDS (bits_u / bits_i are fixed at tfr_create)
static bool small_tables(const tfr_model* m) { return (1 << std::max(m->bits_u, m->bits_i)) <= CSORT_MAX_BINS; }
// a batch of B entries is sorted by the counting sort (otherwise by the radix sort)
static bool csort_path(const tfr_model* m, int64_t B) { return small_tables(m) && csort_eligible(B, m->bits_u, m->bits_i); }

// The reduce's gradient scratch, as ensure_capacity lays it out in cap*D-float parts.  TF1 mode: gq holds the item side's rows,
// gp the user side's.  Otherwise gq = [item side | user side | per-entry copies of the pre-update item rows]; only the pieces of
// runs cut by a block boundary land in the two sides' parts, and the fused user side reads the copies.
static float* user_grad_rows(const tfr_model* m) { return tf1_mode(m) ? m->gp.get() : m->gq + (size_t)m->cap * m->D; }
static float* item_copy_rows(const tfr_model* m) { return m->gq + 2 * (size_t)m->cap * m->D; }
static float* grad_rows(const tfr_model* m, int side) { return side == TFR_P ? user_grad_rows(m) : m->gq.get(); }
static float* grad_bias(const tfr_model* m, int side) { return side == TFR_P ? m->gbp.get() : m->gbq.get(); }

// tfr_last_batch_auc reads the kept batch where the step left it: the logits in d_logits, the rates in d_in (staged batches)
// or d_r.  Whatever overwrites, swaps or reallocates one of them, and every training call, forgets the batch first, so that
// the call refuses (TFR_ERR_STATE) where it would otherwise rank unrelated numbers or read freed memory.
static void forget_kept_batch(tfr_model* m) { m->last_r = nullptr; m->last_B = 0; }

static int ensure_capacity(tfr_model* m, int64_t B) {
    if (B <= m->cap) return TFR_OK;
    forget_kept_batch(m);                                // d_logits and d_r are reallocated
    const int64_t cap = pow2_cap(B);
    if (cap > (int64_t)1 << 30) return fail(TFR_ERR_ARG, "batch %lld too large", (long long)B);
    hipStream_t s = m->stream;
    m->cap = 0;
    m->pf_valid = false;
    HIPCHK(reserve_each(cap, s, m->d_u, m->d_i, m->d_r));
    HIPCHK(m->d_logits.reserve(cap + 4, s));          // + {loss, reg, sum g, error flag} behind the logits
    HIPCHK(reserve_each(cap, s, m->d_g, m->ks_u, m->ps_u, m->ks_i, m->ps_i, m->ks2_u, m->ps2_u, m->ks2_i, m->ps2_i));
    const bool tf1_ws = tf1_mode(m);
    // the layout user_grad_rows / item_copy_rows read
    HIPCHK(m->gq.reserve(cap * m->D * (tf1_ws ? 1 : 3), s));
    HIPCHK(reserve_each(cap, s, m->gbq, m->srt[0][0], m->srt[0][1], m->srt[1][0], m->srt[1][1], m->gbp));
    if (tf1_ws) HIPCHK(m->gp.reserve(cap * m->D, s));
    {   // per-block {loss, reg, sum g}: the forward launches <= 8192 blocks, the reduce with the
        // forward fused in one block per 1024/G sorted entries
        const int64_t nb = (cap + 1024 / m->G - 1) / (1024 / m->G);
        HIPCHK(m->partials.reserve((nb > 8192 ? nb : 8192) * 4, s));
    }
    {
        const int64_t ntiles = (cap + CSORT_TILE - 1) / CSORT_TILE;
        const bool small = small_tables(m);
        const int64_t hu = std::max((small ? ((int64_t)1 << m->bits_u) : 256) * ntiles, 256 * ntiles);
        const int64_t hi = std::max((small ? ((int64_t)1 << m->bits_i) : 256) * ntiles, 256 * ntiles);
        HIPCHK(reserve_each(cap, s, m->osel, m->lrank_u, m->lrank_i));
        HIPCHK(m->hist_u.reserve(hu, s));
        HIPCHK(m->hist_i.reserve(hi, s));
        HIPCHK(m->offs_u.reserve(hu, s));
        HIPCHK(m->offs_i.reserve(hi, s));
        HIPCHK(m->binbase_u.reserve(small ? (int64_t)1 << m->bits_u : 1, s));
        HIPCHK(m->binbase_i.reserve(small ? (int64_t)1 << m->bits_i : 1, s));
        HIPCHK(reserve_each(64 + 256 * ntiles / 4096, s, m->blocktot_u, m->blocktot_i));
    }
    m->cap = cap;
    return TFR_OK;
}

static int cancel_run_ahead(tfr_model* m);

// clear the device error flag e (just read back) and name its cause
static int device_error(tfr_model* m, int32_t e) {
    HIPCHK(hipMemsetAsync(m->d_err, 0, sizeof(int32_t), m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (e & 1) return fail(TFR_ERR_OOB, "user/item id out of range [0,%lld) / [0,%lld)",
                           (long long)m->U, (long long)m->I);
    if (e == 8) return fail(TFR_ERR_OOB, "row-sharded step: another rank voided the step (capacity exceeded or id out of range there) - "
                                         "it was void on every rank; that rank's sync names the cause");
    if (e == 16) return fail(TFR_ERR_ARG, "top-K exclusion CSR: a row is not non-decreasing (or indptr is)");
    if (e & 4) return fail(TFR_ERR_OOB, "row-sharded step: more local samples or distinct items per owner than the fixed capacities "
                                        "(sample_cap / slot_cap) hold - the step was void; raise the slack");
    return fail(TFR_ERR_OOB, "store index out of range [0,%lld)", (long long)m->N);
}

// read + clear the device error flag (stream must be idle or this call synchronises)
static int check_device_error(tfr_model* m) {
    // the flag lands in pinned memory: a pageable destination turns the 4-byte copy into a staged, blocking one
    HIPCHK(m->h_err.reserve(16, m->stream));
    *m->h_err = 0;
    HIPCHK(hipMemcpyAsync(m->h_err, m->d_err, sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    const int32_t e = *m->h_err;
    return e ? device_error(m, e) : TFR_OK;
}

#define MODEL_ENTER(m)                                                \
    if (!(m)) return fail(TFR_ERR_ARG, "null model");                 \
    HIPCHK(hipSetDevice((m)->device));

// TFR_CALL_TRACE=1: host-side timestamps (us since the call's entry) of a multi-step call's phases on stderr
struct CallTrace {
    bool on; std::chrono::steady_clock::time_point t0; const char* name;
    explicit CallTrace(const char* n) : name(n) {
        static const bool en = env_default_off("TFR_CALL_TRACE");
        on = en;
        if (on) t0 = std::chrono::steady_clock::now();
    }
    void mark(const char* what) const {
        if (on) fprintf(stderr, "[%s] %-28s %8.1f us\n", name, what,
                        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// ---------------------------------------------------------------------------------------
extern "C" {

void tfr_default_opts(tfr_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->loss = TFR_LOSS_MSE;
    o->optimizer = TFR_OPT_ADAM;
    o->adam_mode = TFR_ADAM_TF1;
    o->lr = 1e-3f;
    o->reg = 0.05f;
    o->beta1 = 0.9f;
    o->beta2 = 0.999f;
    o->eps = 1e-8f;
}

int tfr_version(void) { return TFR_ABI_VERSION; }

const char* tfr_last_error(void) { return g_err; }

int tfr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- measurement yardstick: what a plain float4 read+write copy reaches on this device ---------------------------
// (MI355X_MICROARCH.md quotes 6.29 TB/s for exactly this shape of kernel; bench.py prints both)
// the copy form that is fastest on this part (tools/probes/copy_bw.hip: one 16-byte element per thread, short-lived workgroups in
// address order, streaming loads and stores - 6.2-6.5 TB/s where a grid-stride loop over the same bytes gives 4.8)
typedef float copy_f4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_copy_f4(const copy_f4* __restrict__ src, copy_f4* __restrict__ dst, int64_t n4) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n4) __builtin_nontemporal_store(__builtin_nontemporal_load(&src[k]), &dst[k]);
}

int tfr_device_copy_rate(int32_t device, int64_t bytes, int32_t reps, double* best_gbs, double* mean_gbs) {
    if (bytes < (1 << 20) || reps < 1 || reps > 1000 || !best_gbs) return fail(TFR_ERR_ARG, "tfr_device_copy_rate: bad argument");
    HIPCHK(hipSetDevice(device));
    const int64_t n4 = bytes / 16;
    DevBuf<copy_f4> a, b;                                // freed on return, with `device` current
    if (reserve_each(n4, nullptr, a, b) != hipSuccess) return fail(TFR_ERR_NOMEM, "tfr_device_copy_rate: out of memory");
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    (void)hipMemsetAsync(a, 1, n4 * 16, st);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    const unsigned grid = (unsigned)((n4 + 255) / 256);
    double best = 0.0, sum = 0.0;
    for (int r = -2; r < reps; ++r) {
        (void)hipEventRecord(e0, st);
        k_copy_f4<<<grid, 256, 0, st>>>(a, b, n4);
        (void)hipEventRecord(e1, st);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (r < 0 || ms <= 0.f) continue;
        const double g = 2.0 * (double)(n4 * 16) / (ms * 1e-3) / 1e9;
        sum += g;
        if (g > best) best = g;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(st);
    *best_gbs = best;
    if (mean_gbs) *mean_gbs = sum / reps;
    return TFR_OK;
}

static void bpr_release(tfr_model* m);

int tfr_destroy(tfr_model* m) {
    if (!m) return TFR_OK;
    if (m->warp_live > 0)
        return fail(TFR_ERR_STATE, "tfr_destroy: %d WARP trainer(s) are bound to this model (tfr_warp_destroy them first)", m->warp_live);
    (void)hipSetDevice(m->device);                       // the buffers are freed with the model's device current
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->stream2) (void)hipStreamSynchronize(m->stream2);
    if (m->stream3) (void)hipStreamSynchronize(m->stream3);
    for (auto& e : m->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto e : m->chunk_ev) (void)hipEventDestroy(e);
    if (m->ev_ids_free) (void)hipEventDestroy(m->ev_ids_free);
    if (m->spec_ev) (void)hipEventDestroy(m->spec_ev);
    for (int z = 0; z < tfr_model::HRING; ++z) if (m->ring_ev[z]) (void)hipEventDestroy(m->ring_ev[z]);
    for (int z = 0; z < 2; ++z) { if (m->ev_sorted[z]) (void)hipEventDestroy(m->ev_sorted[z]); if (m->ev_free[z]) (void)hipEventDestroy(m->ev_free[z]); }
    if (m->ev_first) (void)hipEventDestroy(m->ev_first);
    if (m->ev_mid) (void)hipEventDestroy(m->ev_mid);
    for (auto& e : m->draw_evs) if (e) (void)hipEventDestroy(e);
    if (m->stream2) (void)hipStreamDestroy(m->stream2);
    if (m->stream3) (void)hipStreamDestroy(m->stream3);
    bpr_release(m);
    if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    delete m;
    return TFR_OK;
}

// the tables (zeroed), their optimiser slots and the per-model scratch
static int alloc_model(tfr_model* m) {
    hipStream_t s = m->stream;
    const int64_t U = m->U, I = m->I, D = m->D;
    const bool adam = m->o.optimizer == TFR_OPT_ADAM;
    for (int t = 0; t < 5; ++t) {
        HIPCHK(m->w[t].reserve(m->n[t], s));
        HIPCHK(hipMemsetAsync(m->w[t], 0, (size_t)m->n[t] * 4, s));
        if (adam) {
            HIPCHK(reserve_each(m->n[t], s, m->m[t], m->v[t]));
            HIPCHK(hipMemsetAsync(m->m[t], 0, (size_t)m->n[t] * 4, s));
            HIPCHK(hipMemsetAsync(m->v[t], 0, (size_t)m->n[t] * 4, s));
        }
    }
    if (adam && m->o.adam_mode == TFR_ADAM_TF1) {
        HIPCHK(m->map_u.reserve(U, s));
        HIPCHK(m->map_i.reserve(I, s));
        HIPCHK(hipMemsetAsync(m->map_u, 0, (size_t)U * 4, s));
        HIPCHK(hipMemsetAsync(m->map_i, 0, (size_t)I * 4, s));
        // dense per-row gradient buffers for the TF1 sweep, while they stay small (<= 256 MB)
        if ((size_t)(U + I) * (D + 1) * 4 <= ((size_t)256 << 20)) {
            HIPCHK(m->dg_p.reserve(U * D, s));
            HIPCHK(m->dg_q.reserve(I * D, s));
            HIPCHK(m->dg_bu.reserve(U, s));
            HIPCHK(m->dg_bi.reserve(I, s));
            HIPCHK(hipMemsetAsync(m->dg_p, 0, (size_t)U * D * 4, s));
            HIPCHK(hipMemsetAsync(m->dg_q, 0, (size_t)I * D * 4, s));
            HIPCHK(hipMemsetAsync(m->dg_bu, 0, (size_t)U * 4, s));
            HIPCHK(hipMemsetAsync(m->dg_bi, 0, (size_t)I * 4, s));
        }
    }
    HIPCHK(m->scalars.reserve(4, s));
    HIPCHK(m->d_err.reserve(1, s));
    HIPCHK(hipMemsetAsync(m->scalars, 0, 16, s));
    HIPCHK(hipMemsetAsync(m->d_err, 0, 4, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFR_OK;
}

int tfr_create(tfr_model** out, int64_t U, int64_t I, int32_t D, const tfr_opts* opts) {
    if (!out) return fail(TFR_ERR_ARG, "out is null");
    *out = nullptr;
    if (!opts) return fail(TFR_ERR_ARG, "opts is null");
    if (U < 1 || I < 1 || U > 0x7fffffffLL || I > 0x7fffffffLL)
        return fail(TFR_ERR_ARG, "user_num/item_num must be in [1, 2^31)");
    int G, VEC;
    if (!geometry(D, &G, &VEC))
        return fail(TFR_ERR_ARG, "unsupported dim %d (need dim %% 4 == 0 and dim <= 256, or dim <= 64)", D);
    if (opts->loss != TFR_LOSS_MSE && opts->loss != TFR_LOSS_NLL) return fail(TFR_ERR_ARG, "bad loss");
    if (opts->optimizer != TFR_OPT_ADAM && opts->optimizer != TFR_OPT_SGD) return fail(TFR_ERR_ARG, "bad optimizer");
    if (opts->adam_mode != TFR_ADAM_TF1 && opts->adam_mode != TFR_ADAM_LAZY) return fail(TFR_ERR_ARG, "bad adam_mode");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(TFR_ERR_HIP, "no HIP device available (%s) - this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (opts->device < 0 || opts->device >= ndev) return fail(TFR_ERR_ARG, "device %d not in [0,%d)", opts->device, ndev);
    HIPCHK(hipSetDevice(opts->device));
    tfr_model* m = new (std::nothrow) tfr_model();
    if (!m) return fail(TFR_ERR_NOMEM, "host allocation failed");
    m->U = U; m->I = I; m->D = D; m->G = G; m->VEC = VEC;
    m->o = *opts;
    m->device = opts->device;
    m->bits_u = bits_for(U);
    m->bits_i = bits_for(I);
    m->n[TFR_MU] = 1; m->n[TFR_BU] = U; m->n[TFR_BI] = I; m->n[TFR_P] = U * D; m->n[TFR_Q] = I * D;
    m->b1p = opts->beta1;
    m->b2p = opts->beta2;
    memset(m->prof_ms, 0, sizeof(m->prof_ms));
    memset(m->prof_n, 0, sizeof(m->prof_n));
    int rc = TFR_OK;
    if (hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking) != hipSuccess) {
        rc = fail(TFR_ERR_HIP, "hipStreamCreate failed");
    } else {
        m->stream = m->own_stream;
        rc = alloc_model(m);
    }
    if (rc) {
        char keep[512];
        strncpy(keep, g_err, sizeof(keep));
        tfr_destroy(m);
        strncpy(g_err, keep, sizeof(g_err));
        return rc;
    }
    *out = m;
    return TFR_OK;
}

// ---- variables -------------------------------------------------------------------------
// two-table form: every row that lives in the alternate item table goes back to the main one.  Called by everything that
// looks at item_features other than the fused big-table step itself (forward / eval, get / set, the other step paths).
static int settle_q(tfr_model* m) {
    if (!m->q_dirty) return TFR_OK;
    launch_settle_alt(m->w[TFR_Q], m->q_alt, m->q_sel, m->I, m->D, m->stream);
    HIPCHK(hipGetLastError());
    m->q_dirty = false;
    return TFR_OK;
}

static int table_ptr(tfr_model* m, int32_t which, float** p, int64_t* n) {
    const int t = which & 7;
    if (t > TFR_Q || (which & ~(7 | TFR_SLOT_M | TFR_SLOT_V)) || ((which & TFR_SLOT_M) && (which & TFR_SLOT_V)))
        return fail(TFR_ERR_ARG, "bad table id %d", which);
    if (t == TFR_Q && settle_q(m)) return TFR_ERR_HIP;
    float* q = (which & TFR_SLOT_M) ? m->m[t] : (which & TFR_SLOT_V) ? m->v[t] : m->w[t];
    if (!q) return fail(TFR_ERR_STATE, "table %d has no such slot (optimizer is not Adam)", which);
    *p = q;
    *n = m->n[t];
    return TFR_OK;
}

int tfr_set_table(tfr_model* m, int32_t which, const float* host, int64_t n) {
    MODEL_ENTER(m);
    float* p; int64_t cnt;
    int rc = table_ptr(m, which, &p, &cnt);
    if (rc) return rc;
    if (!host || n != cnt) return fail(TFR_ERR_ARG, "table %d expects %lld floats, got %lld", which, (long long)cnt, (long long)n);
    m->tab_gen += 1;
    HIPCHK(hipMemcpyAsync(p, host, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_get_table(tfr_model* m, int32_t which, float* host, int64_t n) {
    MODEL_ENTER(m);
    float* p; int64_t cnt;
    int rc = table_ptr(m, which, &p, &cnt);
    if (rc) return rc;
    if (!host || n != cnt) return fail(TFR_ERR_ARG, "table %d holds %lld floats, asked %lld", which, (long long)cnt, (long long)n);
    HIPCHK(hipMemcpyAsync(host, p, (size_t)n * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_table_devptr(tfr_model* m, int32_t which, void** ptr, int64_t* n) {
    MODEL_ENTER(m);
    float* p; int64_t cnt;
    int rc = table_ptr(m, which, &p, &cnt);
    if (rc) return rc;
    if (ptr) *ptr = p;
    if (n) *n = cnt;
    m->tab_exposed = true;
    return TFR_OK;
}

int tfr_scalars_devptr(tfr_model* m, void** ptr) {
    MODEL_ENTER(m);
    if (ptr) *ptr = m->scalars;
    return TFR_OK;
}

int tfr_set_frozen(tfr_model* m, uint32_t mask) {
    MODEL_ENTER(m);
    if (mask >> 5) return fail(TFR_ERR_ARG, "frozen mask has bits beyond the 5 tables");
    m->frozen = mask;
    m->tab_gen += 1;
    return TFR_OK;
}

int tfr_get_step(tfr_model* m, int64_t* step, float* b1p, float* b2p) {
    MODEL_ENTER(m);
    if (step) *step = m->step;
    if (b1p) *b1p = m->b1p;
    if (b2p) *b2p = m->b2p;
    return TFR_OK;
}

int tfr_set_step(tfr_model* m, int64_t step, float b1p, float b2p) {
    MODEL_ENTER(m);
    if (step < 0) return fail(TFR_ERR_ARG, "negative step");
    m->step = step;
    m->b1p = b1p;
    m->b2p = b2p;
    m->tab_gen += 1;
    return TFR_OK;
}

int tfr_set_hyper(tfr_model* m, float lr, float reg) {
    MODEL_ENTER(m);
    m->o.lr = lr;
    m->o.reg = reg;
    return TFR_OK;
}

int tfr_set_stream(tfr_model* m, void* s) {
    MODEL_ENTER(m);
    HIPCHK(hipStreamSynchronize(m->stream));
    m->stream = s ? (hipStream_t)s : m->own_stream;
    m->draw_joined = 0;                                  // joins were made on the old stream
    return TFR_OK;
}

// the same without draining the old stream: for a caller that alternates between two streams and orders them itself (events)
int tfr_switch_stream(tfr_model* m, void* s) {
    MODEL_ENTER(m);
    m->stream = s ? (hipStream_t)s : m->own_stream;
    m->draw_joined = 0;                                  // joins were made on the old stream
    return TFR_OK;
}

int tfr_get_stream(tfr_model* m, void** s) {
    MODEL_ENTER(m);
    if (s) *s = (void*)m->stream;
    return TFR_OK;
}

int tfr_sync(tfr_model* m) {
    MODEL_ENTER(m);
    CallTrace tr("sync");
    const int rc = check_device_error(m);
    tr.mark("main stream drained");
    return rc;
}

int tfr_profile(tfr_model* m, int32_t enable) {
    MODEL_ENTER(m);
    int rc = drain_profile(m);
    if (rc) return rc;
    if (enable) {
        memset(m->prof_ms, 0, sizeof(m->prof_ms));
        memset(m->prof_n, 0, sizeof(m->prof_n));
        // calibrate: median-of-9 elapsed time of back-to-back event pairs with nothing in between
        float v[9];
        int n = 0;
        for (int k = 0; k < 9; ++k) {
            hipEvent_t e0, e1;
            if (hipEventCreate(&e0) != hipSuccess) break;
            if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); break; }
            (void)hipEventRecord(e0, m->stream);
            (void)hipEventRecord(e1, m->stream);
            float ms = 0.f;
            if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) v[n++] = ms;
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
        }
        for (int x = 1; x < n; ++x) for (int y = x; y > 0 && v[y] < v[y - 1]; --y) { float t = v[y]; v[y] = v[y - 1]; v[y - 1] = t; }
        m->prof_overhead_ms = n ? v[n / 2] : 0.f;
    }
    m->prof = enable != 0;
    return TFR_OK;
}

int tfr_profile_read(tfr_model* m, int32_t kernel, double* total_ms, int64_t* launches) {
    MODEL_ENTER(m);
    if (kernel < 0 || kernel >= TFR_K_COUNT) return fail(TFR_ERR_ARG, "bad kernel id");
    int rc = drain_profile(m);
    if (rc) return rc;
    if (total_ms) *total_ms = m->prof_ms[kernel];
    if (launches) *launches = m->prof_n[kernel];
    return TFR_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// A training update's view of the model, written once for every step path.
// One side of the factorisation: side = TFR_P (users: P, user_bias) or TFR_Q (items: Q, item_bias).  The side's tables,
// their Adam slots and frozen bits go into the fields every update struct names alike; `w` is where the rows are written.
template <typename A>
static void bind_side_tables(A& a, float*& w, const tfr_model* m, int side) {
    const int b = side == TFR_P ? TFR_BU : TFR_BI;
    w = m->w[side]; a.m = m->m[side]; a.v = m->v[side];
    a.bias_w = m->w[b]; a.bias_m = m->m[b]; a.bias_v = m->v[b];
    a.frozen_rows = (m->frozen >> side) & 1; a.frozen_bias = (m->frozen >> b) & 1;
}
static void bind_side(RedArgs& a, const tfr_model* m, int side) { bind_side_tables(a, a.own_w, m, side); }
static void bind_side(ApplyArgs& a, const tfr_model* m, int side) { bind_side_tables(a, a.w, m, side); }
template <typename A>                    // DenseArgs, TileDenseArgs: the sweeps also cover every row of the side
static void bind_side(A& a, const tfr_model* m, int side) {
    bind_side_tables(a, a.w, m, side);
    a.rows = side == TFR_P ? m->U : m->I;
}

// the optimiser at the model's current step
struct OptStep { bool adam, tf1; float alpha, b1, b2, eps, lr; };
static OptStep opt_step(const tfr_model* m) {
    const tfr_opts& o = m->o;
    const bool adam = o.optimizer == TFR_OPT_ADAM;
    // lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), float32 like the TF graph [TF1-lib]
    return {adam, adam && o.adam_mode == TFR_ADAM_TF1, adam ? o.lr * sqrtf(1.f - m->b2p) / (1.f - m->b1p) : 0.f,
            o.beta1, o.beta2, o.eps, o.lr};
}
template <typename A>
static void set_hyper(A& a, const OptStep& k) { a.alpha = k.alpha; a.b1 = k.b1; a.b2 = k.b2; a.eps = k.eps; a.lr = k.lr; }

// the optimiser as the kernels' mode arguments: the reduce's (scratch in TF1 mode, else the update fused in) and the
// applies' (also the `opt` field of FinArgs / DenseArgs / TileDenseArgs)
static int reduce_mode(const OptStep& k) { return k.tf1 ? RMODE_SCRATCH : k.adam ? RMODE_ADAM : RMODE_SGD; }
static int apply_mode(const OptStep& k) { return k.adam ? 0 : 1; }
// launch_apply_rows: write the reduced rows (and biases) out to w / bias_w instead of updating a table
static const int APPLY_EMIT_ROWS = 2;

// K4 with the bias_global update; partials and nblk are the caller's
static FinArgs mu_fin(const tfr_model* m, const OptStep& k, bool update_mu, float* out) {
    FinArgs f;
    memset(&f, 0, sizeof(f));
    f.scalars = m->scalars; f.out = out; f.err = m->d_err;
    f.mu = m->w[TFR_MU]; f.mu_m = m->m[TFR_MU]; f.mu_v = m->v[TFR_MU];
    f.update_mu = update_mu ? 1 : 0; f.opt = apply_mode(k);
    set_hyper(f, k);
    return f;
}

// K4 without the bias_global update: the local {loss, reg, sum g} into out (data-parallel and row-sharded steps, where
// bias_global waits for the all-reduce); nblk is the caller's
static FinArgs local_fin(const tfr_model* m, float* out) {
    FinArgs f;
    memset(&f, 0, sizeof(f));
    f.partials = m->partials; f.scalars = m->scalars; f.out = out; f.err = m->d_err;
    f.mu = m->w[TFR_MU];
    return f;
}

// ---- the phases of a training step: one builder per argument struct -----------------------------------------------
// Each sets what every caller sets alike; what a path does differently stays an assignment at its call site.

// one side of the segmented reduce over the sorted order ks / ps of B entries: `own` is the side's table, the sums go to
// the side's scratch
static RedArgs reduce_side(const tfr_model* m, int side, const int32_t* ks, const int32_t* ps, int64_t B) {
    RedArgs r;
    memset(&r, 0, sizeof(r));
    r.side = side == TFR_Q ? 1 : 0; r.ks = ks; r.ps = ps;
    r.own = m->w[side]; r.own_bias = m->w[side == TFR_P ? TFR_BU : TFR_BI];
    r.grad_rows = grad_rows(m, side); r.grad_bias = grad_bias(m, side);
    r.err = m->d_err; r.B = B; r.D = m->D;
    return r;
}
// ... of a rating batch: the partner rows are the other table's, by the other id column; g comes from the forward
static RedArgs rating_side(const tfr_model* m, int side, const int32_t* ks, const int32_t* ps, const int32_t* other, int64_t B) {
    RedArgs r = reduce_side(m, side, ks, ps, B);
    r.other = other; r.partner = m->w[side == TFR_P ? TFR_Q : TFR_P]; r.g = m->d_g;
    r.item_abs = m->o.item_abs; r.reg_bias = m->o.reg_bias; r.lam = m->o.reg;
    return r;
}

// k_apply_rows on the runs of one side that the reduce cut into several pieces (the whole runs are done)
static ApplyArgs apply_split(const tfr_model* m, int side, const int32_t* ks, int64_t B) {
    ApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.ks = ks; a.grad_rows = grad_rows(m, side); a.grad_bias = grad_bias(m, side);
    a.err = m->d_err; a.B = B; a.D = m->D; a.only_split = 1;
    return a;
}

// the dense sweep of one side (every row moves); with ks, the touched rows' sums come from the reduce's scratch, found
// through the side's row -> slot map
static DenseArgs dense_side(const tfr_model* m, const OptStep& k, int side, const int32_t* ks = nullptr, int64_t B = 0) {
    DenseArgs d;
    memset(&d, 0, sizeof(d));
    bind_side(d, m, side);
    set_hyper(d, k);
    d.err = m->d_err; d.D = m->D; d.opt = apply_mode(k);
    if (ks) {
        d.map = side == TFR_P ? m->map_u : m->map_i;
        d.ks = ks; d.B = B; d.grad_rows = grad_rows(m, side); d.grad_bias = grad_bias(m, side);
    }
    return d;
}

// k_dense_tiles over both sides' per-tile piece sums of a B-entry batch (tile tables of parity par), K4 `f` riding along;
// a[0] items, a[1] users
static TileDenseLaunch tile_dense(const tfr_model* m, int64_t B, int par, const FinArgs& f) {
    TileDenseLaunch L;
    memset(&L, 0, sizeof(L));
    for (int j = 0; j < 2; ++j) {
        const int side = j == 0 ? TFR_Q : TFR_P;
        TileDenseArgs& d = L.a[j];
        d.tab = j == 0 ? (par ? m->offs_i : m->hist_i) : (par ? m->offs_u : m->hist_u);
        d.nbins = 1 << (j == 0 ? m->bits_i : m->bits_u);
        d.ntiles = (int32_t)((B + CSORT_TILE - 1) / CSORT_TILE);
        d.grad_rows = grad_rows(m, side); d.grad_bias = grad_bias(m, side);
        d.rows = side == TFR_P ? m->U : m->I;
        d.err = m->d_err; d.D = m->D;
    }
    L.f = f;
    return L;
}

// after a step's applies: the beta-power accumulators advance [TF1-lib], then the step count
static void advance_step(tfr_model* m) {
    if (m->o.optimizer == TFR_OPT_ADAM) {
        m->b1p *= m->o.beta1;
        m->b2p *= m->o.beta2;
    }
    m->step += 1;
}

// the forward's tables, batch and outputs; with d_store_ids the batch is gathered from the resident store
static FwdArgs fwd_args(const tfr_model* m, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                        float* d_logits, float* d_g, const int64_t* d_store_ids) {
    FwdArgs a;
    memset(&a, 0, sizeof(a));
    a.P = m->w[TFR_P]; a.Q = m->w[TFR_Q]; a.bu = m->w[TFR_BU]; a.bi = m->w[TFR_BI]; a.mu = m->w[TFR_MU];
    a.u = du; a.it = di; a.r = dr;
    a.logits = d_logits; a.g = d_g; a.partials = m->partials; a.err = m->d_err;
    a.B = B; a.U = m->U; a.I = m->I; a.N = m->N;
    if (d_store_ids) { a.ids = d_store_ids; a.store = m->store; }
    a.D = m->D; a.loss = m->o.loss; a.item_abs = m->o.item_abs; a.reg_bias = m->o.reg_bias;
    return a;
}

// which rows a forward scores from: the float32 tables, or their bf16 snapshot (bf16_rows.h)
enum FwdRows { ROWS_F32, ROWS_BF16 };

// TFR_BF16_PNT=0|1: A/B override of the non-temporal user rows (unset: the float32 forward's rule on the snapshot's bytes).
// Read at every launch, so that one process can alternate the two (tools/bench_bf16_forward.py --pnt-ab).
static bool bf16_pnt(int64_t U, int D) {
    if (env_default_off("TFR_BF16_PNT")) return true;
    if (!env_default_on("TFR_BF16_PNT")) return false;
    return stream_user_rows(U, (size_t)bf16_row_stride(D) * 2);
}

// what a forward launches for a shape: lanes per rating, ratings in flight per lane group, blocks, and whether the user
// rows go by non-temporal loads.  run_forward launches by it and tfr_forward_plan reports it.
struct FwdPlan { int G, unr, grid; bool pnt; };
static FwdPlan forward_plan(int D, int G_f32, int64_t U, int mode, FwdRows rows, int64_t B) {
    FwdPlan p;
    p.G = rows == ROWS_F32 ? G_f32 : bf16_geometry(D);
    p.unr = rows == ROWS_F32 ? 4 : bf16_unroll(p.G);
    p.grid = forward_grid(B, p.G, mode, p.unr);
    p.pnt = rows == ROWS_F32 ? forward_pnt(mode, U, D) : bf16_pnt(U, D);     // float32: launch_forward asks forward_pnt itself
    return p;
}

// forward on device-resident ids; from the snapshot: MODE_INFER or MODE_EVAL
static int run_forward(tfr_model* m, int mode, const int32_t* du, const int32_t* di, const float* dr,
                       int64_t B, float* d_logits, float* d_g, int* nblk_out,
                       const int64_t* d_store_ids = nullptr, FwdRows rows = ROWS_F32) {
    if (rows == ROWS_F32) { const int rcq = settle_q(m); if (rcq) return rcq; }
    const FwdPlan fp = forward_plan(m->D, m->G, m->U, mode, rows, B);
    const int G = fp.G, grid = fp.grid;
    if (nblk_out) *nblk_out = grid;
    if (rows == ROWS_F32) {
        FwdArgs a = fwd_args(m, du, di, dr, B, d_logits, d_g, d_store_ids);
        if (d_store_ids) { a.u_out = m->d_u; a.it_out = m->d_i; }     // the gathered ids, for the backward
        { static const bool lr = env_default_off("TFR_LDS_REDUCE"); a.lds_reduce = lr; }
        Prof p(m, TFR_K_FORWARD);
        launch_forward(a, mode, G, m->VEC, grid, m->stream);
    } else {
        Bf16FwdArgs a;
        memset(&a, 0, sizeof(a));
        a.P = m->bf.p; a.Q = m->bf.q; a.bu = m->bf.bu; a.bi = m->bf.bi; a.mu = m->bf.mu;
        a.u = du; a.it = di; a.r = dr;
        a.logits = d_logits; a.partials = m->partials; a.err = m->d_err;
        a.B = B; a.U = m->U; a.I = m->I;
        a.DP = bf16_row_stride(m->D); a.loss = m->o.loss; a.item_abs = m->o.item_abs;
        Prof p(m, TFR_K_FORWARD);
        launch_forward_bf16(a, mode, G, grid, fp.pnt, m->stream);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// which pass a radix sort of B keys takes: the 4096-key tiles from TFR_RSORT_WIDE_MIN keys up unless TFR_RSORT_WIDE=0
// (radix_sort_columns launches by it, tfr_kernel_plan reports it)
static bool rsort_wide_taken(int64_t B) { return switch_rsort_wide() && rsortw_eligible(B); }

// hand-written LSD radix sort of one or two key columns: column c = (keys[c], bits[c]) ->
// sorted keys in ks_out[c], original positions in ps_out[c].  ceil(maxbits/8) passes, 3 launches each.
static int radix_sort_columns(tfr_model* m, int ncols, const int32_t* const* keys, const int* bits,
                              int32_t* const* ks_out, int32_t* const* ps_out, int64_t B,
                              const int64_t* limits = nullptr, const int64_t* store_ids = nullptr) {
    m->pf_valid = false;                                 // the sort scratch doubles as the published tables of the tile step
    int maxbits = bits[0];
    if (ncols > 1 && bits[1] > maxbits) maxbits = bits[1];
    const int passes = (maxbits + 7) / 8;
    int32_t* tmpk[2] = {m->ks2_u, m->ks2_i};
    int32_t* tmpv[2] = {m->ps2_u, m->ps2_i};
    RSortArgs r;
    memset(&r, 0, sizeof(r));
    r.B = B;
    r.ntiles = (int32_t)((B + CSORT_TILE - 1) / CSORT_TILE);
    r.lrank[0] = m->lrank_u; r.lrank[1] = m->lrank_i;
    r.hist[0] = m->hist_u; r.hist[1] = m->hist_i;
    r.offs[0] = m->offs_u; r.offs[1] = m->offs_i;
    r.blocktot[0] = m->blocktot_u; r.blocktot[1] = m->blocktot_i;
    r.chunk = 4096;                                      // entries per scan block (k_rsort_scan)
    for (int p = 0; p < passes; ++p) {
        const bool to_final = ((passes - 1 - p) % 2) == 0;      // last pass lands in ks_out / ps_out
        for (int c = 0; c < ncols; ++c) {
            if (p == 0) { r.keys_in[c] = keys[c]; r.vals_in[c] = nullptr; }
            else { r.keys_in[c] = r.keys_out[c]; r.vals_in[c] = r.vals_out[c]; }
        }
        for (int c = 0; c < ncols; ++c) {
            r.keys_out[c] = to_final ? ks_out[c] : tmpk[c];
            r.vals_out[c] = to_final ? ps_out[c] : tmpv[c];
        }
        r.shift = 8 * p;
        r.ids = nullptr;
        if (p == 0 && store_ids) {                               // the first pass gathers the batch from the resident store itself
            r.ids = store_ids; r.store = m->store; r.N = m->N;
            r.u_out = m->d_u; r.i_out = m->d_i; r.r_out = m->d_r;
        }
        r.err = (p == 0 && limits) ? m->d_err : nullptr;         // ids outside the tables void the step
        if (limits) for (int c = 0; c < ncols; ++c) r.limit[c] = (int32_t)limits[c];
        if (rsort_wide_taken(B)) launch_rsortw_pass(r, ncols, m->stream);   // from 65536 keys: 4096-key tiles, LDS-staged scatter
        else launch_rsort_pass(r, ncols, m->stream);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// the radix sort of n keys of du (and, with di, of di) by the model's own key widths into ks_u/ps_u (ks_i/ps_i);
// checked: ids outside (U, I) void the step
static int sort_model_columns(tfr_model* m, const int32_t* du, const int32_t* di, int64_t n, bool checked,
                              const int64_t* store_ids = nullptr) {
    const int32_t* keys[2] = {du, di};
    const int bits[2] = {m->bits_u, m->bits_i};
    int32_t* ks[2] = {m->ks_u, m->ks_i};
    int32_t* ps[2] = {m->ps_u, m->ps_i};
    const int64_t limits[2] = {m->U, m->I};
    return radix_sort_columns(m, di ? 2 : 1, keys, bits, ks, ps, n, checked ? limits : nullptr, store_ids);
}

// stable sort of batch positions by user id and by item id
static int sort_columns(tfr_model* m, const int32_t* du, const int32_t* di, int64_t B,
                        const FinArgs* fin = nullptr, bool* fin_done = nullptr, bool validate = false,
                        const int64_t* store_ids = nullptr) {
    Prof p(m, TFR_K_SORT);
    m->pf_valid = false;                                 // the sort scratch doubles as the published tables of the tile step
    if (csort_path(m, B)) {
        CSortArgs c;
        c.keys[0] = du; c.keys[1] = di;
        c.ks[0] = m->ks_u; c.ks[1] = m->ks_i; c.ps[0] = m->ps_u; c.ps[1] = m->ps_i;
        c.lrank[0] = m->lrank_u; c.lrank[1] = m->lrank_i; c.hist[0] = m->hist_u; c.hist[1] = m->hist_i;
        c.offs[0] = m->offs_u; c.offs[1] = m->offs_i; c.binbase[0] = m->binbase_u; c.binbase[1] = m->binbase_i;
        c.blocktot[0] = m->blocktot_u; c.blocktot[1] = m->blocktot_i;
        c.nbins[0] = 1 << m->bits_u; c.nbins[1] = 1 << m->bits_i;
        c.ntiles = (int32_t)((B + CSORT_TILE - 1) / CSORT_TILE);
        c.B = B;
        launch_csort(c, fin, m->stream);
        if (fin && fin_done) *fin_done = true;
        HIPCHK(hipGetLastError());
        return TFR_OK;
    }
    return sort_model_columns(m, du, di, B, validate, store_ids);
}

// big tables with a touched-rows optimiser: the forward is computed inside the item-side reduce,
// which needs the sorted order first - so the step starts with (gather +) sort
static bool fwd_in_reduce(const tfr_model* m, int64_t B) {
    return B > 0 && !tf1_mode(m) && !csort_path(m, B);
}

static int gather_batch(tfr_model* m, const int64_t* d_ids, int64_t lo, int64_t B);

// forward (+ fused store gather) and the stable sort of both id columns for one minibatch; K4
// (`f`) rides in the csort scan launch when that path is taken (fin_done).  du/di are updated
// to where the batch ids live afterwards.
static bool tiles_eligible(const tfr_model* m, int64_t B) {
    return B > 0 && csort_path(m, B) && (B + CSORT_TILE - 1) / CSORT_TILE <= 16;
}

static int front_and_sort(tfr_model* m, const int32_t*& du, const int32_t*& di, const float*& dr, int64_t B,
                          float* d_logits, const int64_t* d_store_ids, FinArgs& f, int& nblk, bool& fin_done,
                          bool tiles = false, bool sort_only = false) {
    m->pf_valid = false;                                 // the sort scratch doubles as the published tables of the tile step
    hipStream_t s = m->stream;
    int rc;
    if (sort_only) {
        const bool radix = !csort_path(m, B);
        static const bool fuse = env_default_on("TFR_FUSE_GATHER");   // TFR_FUSE_GATHER=0: A/B switch (separate k_gather_triples launch)
        if (d_store_ids && radix && fuse) {                      // the radix sort's first pass gathers the batch itself (one launch less)
            du = m->d_u; di = m->d_i; dr = m->d_r;
            return sort_columns(m, du, di, B, nullptr, nullptr, true, d_store_ids);
        }
        if (d_store_ids) {
            if ((rc = gather_batch(m, d_store_ids, 0, B))) return rc;
            du = m->d_u; di = m->d_i; dr = m->d_r;
        }
        return sort_columns(m, du, di, B, nullptr, nullptr, true);       // + id range check
    }
    if (d_store_ids && B >= 32768) {
        // big batches are bandwidth-bound: a separate gather keeps the forward's dependent chain
        // at ids -> rows; small batches are launch-bound and gather inside the forward instead
        if ((rc = gather_batch(m, d_store_ids, 0, B))) return rc;
        d_store_ids = nullptr;
        du = m->d_u; di = m->d_i; dr = m->d_r;
    }
    if (csort_path(m, B)) {
        // small tables: forward and the counting sort's rank pass share one launch, then
        // scan (+K4) and scatter
        FrontArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.f = fwd_args(m, du, di, dr, B, d_logits, m->d_g, d_store_ids);     // with store ids the rank blocks publish them
        CSortArgs& c = fa.c;
        c.keys[0] = d_store_ids ? m->d_u : du; c.keys[1] = d_store_ids ? m->d_i : di;
        c.ks[0] = m->ks_u; c.ks[1] = m->ks_i; c.ps[0] = m->ps_u; c.ps[1] = m->ps_i;
        c.lrank[0] = m->lrank_u; c.lrank[1] = m->lrank_i; c.hist[0] = m->hist_u; c.hist[1] = m->hist_i;
        c.offs[0] = m->offs_u; c.offs[1] = m->offs_i; c.binbase[0] = m->binbase_u; c.binbase[1] = m->binbase_i;
        c.blocktot[0] = m->blocktot_u; c.blocktot[1] = m->blocktot_i;
        c.nbins[0] = 1 << m->bits_u; c.nbins[1] = 1 << m->bits_i;
        c.ntiles = (int32_t)((B + CSORT_TILE - 1) / CSORT_TILE);
        c.B = B;
        fa.key_out[0] = m->d_u; fa.key_out[1] = m->d_i;
        fa.nfwd = front_forward_blocks(B, m->G);
        fa.tile_local = tiles ? 1 : 0;
        nblk = fa.nfwd;
        {
            Prof p(m, TFR_K_FORWARD);
            launch_front(fa, m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
        if (d_store_ids) { du = m->d_u; di = m->d_i; }
        f.nblk = nblk;
        if (tiles) return TFR_OK;      // tile-local order is final; K4 rides in the sweep launch
        {
            Prof p(m, TFR_K_SORT);
            launch_csort_tail(c, &f, s);
        }
        HIPCHK(hipGetLastError());
        fin_done = true;
    } else {
        rc = run_forward(m, MODE_TRAIN, du, di, dr, B, d_logits, m->d_g, &nblk, d_store_ids);
        if (rc) return rc;
        if (d_store_ids) { du = m->d_u; di = m->d_i; }
        f.nblk = nblk;
        if ((rc = sort_columns(m, du, di, B, &f, &fin_done))) return rc;
    }
    return TFR_OK;
}

// K1+K2+K3 of the small-table step in one launch (k_tile_step).  Look-ahead (multi-step calls on the
// resident store): was this batch's tile sort published by the previous launch?  Is there a next
// batch to sort in this one?  The packed tables and the sorted records are double-buffered by step
// parity (hist_* / offs_* serve as the two tables).  *par_out = which table set k_dense_tiles reads.
// ---- store records beside the id buffers (IdBuf) ---------------------------------------------------------
static bool recs_on() {                                  // TFR_RECS=0: A/B switch
    static const bool on = env_default_on("TFR_RECS");
    return on;
}
static void recs_forget(tfr_model* m) { m->ids.n_recs = 0; m->ids_alt.n_recs = 0; }      // the store changed
// does [p, p + n) overlap the id buffer b?
static bool ids_overlap(const IdBuf& b, const int64_t* p, int64_t n) {
    const int64_t* base = b.ids;
    return base && p < base + b.ids.capacity() && base < p + n;
}
// after a run of ids [off, off + count) of b was written on stream `st`: gather their records behind it.  Without room
// for the records (allocation failed) the step reads ids -> store as without them.
static void recs_follow(tfr_model* m, IdBuf& b, int64_t off, int64_t count, hipStream_t st) {
    if (!recs_on()) return;
    if (b.recs.capacity() < b.ids.capacity()) {          // the old records' readers: the id buffer they went with was freed after a sync
        b.n_recs = 0;
        b.recs.reset();
        if (b.recs.reserve(b.ids.capacity(), st) != hipSuccess) { (void)hipGetLastError(); return; }
    }
    if (off > b.n_recs) { b.n_recs = 0; return; }        // a gap: nothing before `off` is known to have records
    launch_gather_recs(b.ids + off, m->store, b.recs + off, count, m->N, st);
    b.n_recs = off + count;
}
// the records of ids [p, p + B) when p points into one of the model's id buffers and they are all there
static const int4* recs_for(tfr_model* m, const int64_t* p, int64_t B) {
    if (!p || !recs_on()) return nullptr;
    for (const IdBuf* b : {&m->ids, &m->ids_alt})
        if (ids_overlap(*b, p, 1) && (p - b->ids.get()) + B <= b->n_recs) return b->recs + (p - b->ids.get());
    return nullptr;
}

static int tile_step_launch(tfr_model* m, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                            float* d_logits, const int64_t* d_store_ids, const int64_t* next_store_ids,
                            int* par_out, int* nblk_out) {
    const tfr_opts& o = m->o;
    TileStepArgs ts;
    memset(&ts, 0, sizeof(ts));
    ts.P = m->w[TFR_P]; ts.Q = m->w[TFR_Q]; ts.bu = m->w[TFR_BU]; ts.bi = m->w[TFR_BI]; ts.mu = m->w[TFR_MU];
    ts.u = du; ts.it = di; ts.r = dr;
    if (d_store_ids) { ts.ids = d_store_ids; ts.store = m->store; ts.recs = recs_for(m, d_store_ids, B); }
    ts.logits = d_logits; ts.partials = m->partials; ts.err = m->d_err;
    const bool presorted = m->pf_valid && d_store_ids && m->pf_ids == d_store_ids && m->pf_B == B;
    const int par = presorted ? m->pf_par : 0;
    int32_t* tabs[2][2] = {{m->hist_u, m->hist_i}, {m->offs_u, m->offs_i}};
    ts.tab[0] = tabs[par][0]; ts.tab[1] = tabs[par][1];
    if (presorted) { ts.srt[0] = m->srt[par][0]; ts.srt[1] = m->srt[par][1]; }
    m->pf_valid = false;
    if (next_store_ids && d_store_ids) {
        ts.store = m->store;
        ts.next_ids = next_store_ids; ts.next_B = B; ts.next_ntiles = (int32_t)((B + CSORT_TILE - 1) / CSORT_TILE);
        ts.next_recs = recs_for(m, next_store_ids, B);
        ts.next_tab[0] = tabs[par ^ 1][0]; ts.next_tab[1] = tabs[par ^ 1][1];
        ts.next_srt[0] = m->srt[par ^ 1][0]; ts.next_srt[1] = m->srt[par ^ 1][1];
        m->pf_valid = true; m->pf_ids = next_store_ids; m->pf_B = B; m->pf_par = par ^ 1;
    }
    ts.grad_rows[0] = grad_rows(m, TFR_P); ts.grad_rows[1] = grad_rows(m, TFR_Q);
    ts.grad_bias[0] = grad_bias(m, TFR_P); ts.grad_bias[1] = grad_bias(m, TFR_Q);
    ts.B = B; ts.U = m->U; ts.I = m->I; ts.N = m->N;
    ts.D = m->D; ts.loss = o.loss; ts.item_abs = o.item_abs; ts.reg_bias = o.reg_bias;
    ts.ntiles = (int32_t)((B + CSORT_TILE - 1) / CSORT_TILE);
    ts.nbins[0] = 1 << m->bits_u; ts.nbins[1] = 1 << m->bits_i;
    ts.lam = o.reg;
    *par_out = par;
    *nblk_out = ts.ntiles * m->G;            // one {loss, reg, sum g} slot per piece
    static const bool dbg_on = env_default_off("TFR_TILE_DEBUG");   // TFR_TILE_DEBUG=1: per-block start / end stamps of every launch on stderr (synchronises)
    if (dbg_on && m->tile_dbg.reserve(2048 * 8, m->stream) != hipSuccess) (void)hipGetLastError();
    unsigned long long* d_dbg = m->tile_dbg;
    if (d_dbg && 2 * (ts.next_ntiles + ts.ntiles * m->G) <= 2048) { (void)hipMemsetAsync(d_dbg, 0, 2048 * 64, m->stream); ts.dbg = d_dbg; }
    {
        Prof p(m, TFR_K_REDUCE_ITEM);
        launch_tile_step(ts, m->G, m->VEC, m->stream);
    }
    HIPCHK(hipGetLastError());
    if (ts.dbg) {
        std::vector<unsigned long long> h(2048 * 8);
        (void)hipStreamSynchronize(m->stream);
        (void)hipMemcpy(h.data(), d_dbg, h.size() * 8, hipMemcpyDeviceToHost);
        unsigned long long t0 = ~0ull, t1 = 0;
        for (size_t k = 0; k < h.size(); k += 8) if (h[k]) { if (h[k] < t0) t0 = h[k]; if (h[k + 1] > t1) t1 = h[k + 1]; }
        const int nsort = ts.next_ids ? 2 * ts.next_ntiles : 0;
        const int64_t epb = 1024 / m->G, epg = tile_step_epg(ts.ntiles, m->G, m->VEC);
        const size_t nblk_u = (size_t)((B + epb * epg - 1) / (epb * epg));   // grid: sort blocks, user side, item side
        double ahead_end = 0, ahead_dur = 0, comp_end = 0, comp_dur = 0, ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, phl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int longest_y = -1; size_t longest_k = 0;
        int nblocks = 0, ncomp = 0;
        for (size_t k = 0; k < h.size() / 8; ++k) {
            const unsigned long long* b = &h[8 * k];
            if (!b[0]) continue;
            ++nblocks;
            const double st = (b[0] - t0) / 100.0, en = (b[1] - t0) / 100.0;
            const bool ah = (int)k < nsort;
            if (ah) { if (en > ahead_end) ahead_end = en; if (en - st > ahead_dur) ahead_dur = en - st; }
            else {
                if (en > comp_end) comp_end = en;
                if (en - st > comp_dur) {
                    comp_dur = en - st; longest_y = k < nsort + nblk_u ? 0 : 1; longest_k = k - nsort - (longest_y ? nblk_u : 0);
                    if (b[2] && b[6]) { for (int q = 2; q <= 6; ++q) phl[q] = (b[q] - b[0]) / 100.0; phl[7] = en - st; }
                }
                if (b[2] && b[6]) { ++ncomp; for (int q = 2; q <= 6; ++q) ph[q] += (b[q] - b[0]) / 100.0; ph[7] += en - st; }
            }
        }
        fprintf(stderr, "[k_tile_step] %d blocks (%d look-ahead): span %.2f us; look-ahead blocks end by %.2f (longest %.2f), step blocks end by "
                        "%.2f (longest %.2f); mean step block, us since its start: records %.2f, rows+contributions %.2f, wave sums staged %.2f, "
                        "partials %.2f, wave rounds %.2f, end %.2f\n", nblocks, nsort, (t1 - t0) / 100.0, ahead_end, ahead_dur, comp_end, comp_dur,
                ph[2] / (ncomp ? ncomp : 1), ph[3] / (ncomp ? ncomp : 1), ph[4] / (ncomp ? ncomp : 1), ph[5] / (ncomp ? ncomp : 1),
                ph[6] / (ncomp ? ncomp : 1), ph[7] / (ncomp ? ncomp : 1));
        fprintf(stderr, "[k_tile_step] longest step block: side %d, block %zu of its side: records %.2f, rows+contributions %.2f, wave sums staged %.2f, "
                        "partials %.2f, wave rounds %.2f, end %.2f\n", longest_y, longest_k, phl[2], phl[3], phl[4], phl[5], phl[6], phl[7]);
    }
    return TFR_OK;
}

// The three paths of a training step after its forward and sort (front_and_sort); `f` is the step's K4, nblk included.

// small tables: per-tile sorted order -> piece sums per tile -> one sweep that combines a row's per-tile partials, applies
// the optimiser to both tables and runs K4.  one_launch: gather + tile-local sort + forward + per-tile reduce of both sides
// in one launch (k_tile_step); otherwise the reduce follows front_and_sort's forward and sort
static int step_small_tiles(tfr_model* m, const OptStep& k, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                            float* d_logits, const int64_t* d_store_ids, const int64_t* next_store_ids, bool one_launch,
                            FinArgs f) {
    hipStream_t s = m->stream;
    int par = 0;
    if (one_launch) {
        int nblk = 0, rc;
        if ((rc = tile_step_launch(m, du, di, dr, B, d_logits, d_store_ids, next_store_ids, &par, &nblk))) return rc;
        f.nblk = nblk;
    } else {
        RedPair pr;
        pr.a[0] = rating_side(m, TFR_Q, m->ks_i, m->ps_i, du, B);
        pr.a[1] = rating_side(m, TFR_P, m->ks_u, m->ps_u, di, B);
        pr.a[0].tile = pr.a[1].tile = CSORT_TILE;
        Prof p(m, TFR_K_REDUCE_ITEM);
        launch_seg_reduce(pr, 2, RMODE_SCRATCH, m->G, m->VEC, s);
    }
    HIPCHK(hipGetLastError());
    TileDenseLaunch L = tile_dense(m, B, par, f);
    for (int j = 0; j < 2; ++j) {
        TileDenseArgs& d = L.a[j];
        bind_side(d, m, j == 0 ? TFR_Q : TFR_P);
        set_hyper(d, k);
        d.opt = apply_mode(k); d.skip_untouched = k.tf1 ? 0 : 1;
    }
    {
        Prof p(m, TFR_K_APPLY);
        launch_dense_tiles(L, false, true, m->G, m->VEC, s);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// big tables, Adam in TF1 mode: both sides' sums into scratch in one launch (both only read the tables), then the dense
// sweeps - every row of every unfrozen table moves.  B = 0: the sweeps alone
static int step_big_tf1(tfr_model* m, const OptStep& k, const int32_t* du, const int32_t* di, int64_t B) {
    hipStream_t s = m->stream;
    if (B > 0) {
        RedPair pr = {{rating_side(m, TFR_Q, m->ks_i, m->ps_i, du, B), rating_side(m, TFR_P, m->ks_u, m->ps_u, di, B)}};
        RedArgs& ri = pr.a[0];
        RedArgs& ru = pr.a[1];
        bind_side(ru, m, TFR_P);
        set_hyper(ri, k); set_hyper(ru, k);
        ri.map = m->map_i; ru.map = m->map_u;
        if (m->dg_p) {
            ri.dense_rows = m->dg_q; ri.dense_bias = m->dg_bi;
            ru.dense_rows = m->dg_p; ru.dense_bias = m->dg_bu;
        }
        {
            Prof p(m, TFR_K_REDUCE_ITEM);
            launch_seg_reduce(pr, 2, reduce_mode(k), m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
    }
    Prof p(m, TFR_K_APPLY);
    DensePair dp;
    memset(&dp, 0, sizeof(dp));
    dp.a[0] = dense_side(m, k, TFR_P, m->ks_u, B);
    dp.a[0].dense_grad = m->dg_p; dp.a[0].dense_gbias = m->dg_bu;
    dp.a[1] = dense_side(m, k, TFR_Q, m->ks_i, B);
    dp.a[1].dense_grad = m->dg_q; dp.a[1].dense_gbias = m->dg_bi;
    // the sweep also consumes (clears) the row->slot maps, so it always runs on both tables
    launch_adam_dense(dp, 2, m->G, m->VEC, s);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// big tables, lazy Adam / SGD: both sides fused (reduce + update in place).  The item side goes first; the user side then
// updates P and reads the pre-update Q rows - from the table the item side did not write (dual) or from the per-entry copy
// the item side leaves.  fwd_fused: K1 runs inside the item side.  Pieces of runs cut by a block boundary are parked in
// the sides' scratch and finished by k_apply_rows, which also carries K4 unless the sort did (fin_done)
static int step_big_fused(tfr_model* m, const OptStep& k, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                          float* d_logits, bool fwd_fused, bool dual, FinArgs f, bool fin_done) {
    hipStream_t s = m->stream;
    RedArgs ri = rating_side(m, TFR_Q, m->ks_i, m->ps_i, du, B);
    RedArgs ru = rating_side(m, TFR_P, m->ks_u, m->ps_u, di, B);
    bind_side(ri, m, TFR_Q); bind_side(ru, m, TFR_P);
    set_hyper(ri, k); set_hyper(ru, k);
    // big tables: every row of this step is touched once and cannot stay cached - non-temporal loads / stores for the
    // rows, default policy only for reading back the pre-update copies (A/B, TFR_NT=<bits>:
    // 523-548 us/step with 0, 498 with 23; bits in svd_kernels.h RedArgs::nt)
    { static const int nt = (int)env_int("TFR_NT", 23); ri.nt = ru.nt = fwd_fused ? nt : 0; }
    if (dual) {
        // the updated item row goes to the table the row is NOT in, so the user side still finds the pre-update row where
        // it was: no copy written (4D per rating) and none read
        ri.own_alt = m->q_alt; ri.own_w_alt = m->q_alt; ri.sel = m->q_sel; ri.osel_out = m->osel;
        ru.osel_in = m->osel; ru.partner_alt = m->q_alt;
        m->q_dirty = true;
    } else {
        ri.own_copy_out = item_copy_rows(m);
        ru.partner_by_pos = item_copy_rows(m);
    }
    if (fwd_fused) {           // K1 inside the item side: logits, g, per-block {loss, reg, sum g}
        ri.partner_bias = m->w[TFR_BU]; ri.mu = m->w[TFR_MU]; ri.r = dr; ri.loss = m->o.loss;
        ri.g_out = m->d_g; ri.logits_out = d_logits; ri.partials = m->partials;
        { static const bool st = env_default_on("TFR_STAGE_SUM"); ri.stage_sum = st; }
        const int epb = 1024 / m->G;
        f.nblk = (int)((B + epb - 1) / epb);
    }
    RedPair pr;
    pr.a[0] = ri;
    {
        Prof p(m, TFR_K_REDUCE_ITEM);
        launch_seg_reduce(pr, 1, reduce_mode(k), m->G, m->VEC, s, fwd_fused);
    }
    HIPCHK(hipGetLastError());
    if (m->ev_mid_on) HIPCHK(hipEventRecord(m->ev_mid, s));
    pr.a[0] = ru;
    {
        Prof p(m, TFR_K_REDUCE_USER);
        launch_seg_reduce(pr, 1, reduce_mode(k), m->G, m->VEC, s);
    }
    HIPCHK(hipGetLastError());
    ApplyPair app;
    app.a[0] = apply_split(m, TFR_Q, m->ks_i, B);
    app.a[1] = apply_split(m, TFR_P, m->ks_u, B);
    bind_side(app.a[0], m, TFR_Q); bind_side(app.a[1], m, TFR_P);
    set_hyper(app.a[0], k); set_hyper(app.a[1], k);
    if (dual) { app.a[0].w_alt = m->q_alt; app.a[0].sel = m->q_sel; }
    if (!fin_done) { app.f = f; app.with_fin = 1; }     // K4 rides in the same launch (one launch and ~6 us fewer per big-table step)
    {
        Prof p(m, TFR_K_APPLY);
        launch_apply_rows(app, 2, apply_mode(k), m->G, m->VEC, s);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// one minibatch on device-resident (u, i, r) - or, with d_store_ids, on rows of the resident
// store gathered inside the forward kernel; out3 = optional device {loss, reg, sum_g} slot
static int run_train_step(tfr_model* m, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                          float* d_logits, float* out3, const int64_t* d_store_ids = nullptr,
                          const int64_t* next_store_ids = nullptr, bool presorted_big = false, bool out_err = false) {
    const OptStep k = opt_step(m);
    int nblk = 0, rc;
    hipStream_t s = m->stream;
    bool fin_done = false;
    forget_kept_batch(m);                                // (tfr_train_step / tfr_train_steps_repeat keep theirs after this)
    FinArgs f = mu_fin(m, k, !((m->frozen >> TFR_MU) & 1), out3);
    f.partials = m->partials; f.out_err = out_err ? 1 : 0;
    const bool tiles = tiles_eligible(m, B);
    const bool fwd_fused = fwd_in_reduce(m, B);
    bool dual = false, one_launch = false;
    if (B > 0) {
        // two-table form of the fused big-table step (no per-entry copy of the pre-update item rows): TFR_DUALQ=0 restores the copy
        dual = fwd_fused && switch_dualq();
        if (dual && !(m->q_alt && m->q_sel)) {           // both tables or neither
            hipError_t e = m->q_alt.reserve(m->n[TFR_Q], s);
            if (e == hipSuccess) e = m->q_sel.reserve(m->I, s);
            if (e == hipSuccess) e = hipMemsetAsync(m->q_sel, 0, (size_t)m->I * 4, s);
            if (e != hipSuccess) {
                m->q_alt.reset();
                m->q_sel.reset();
                return fail(e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, "two-table step: %s", hipGetErrorString(e));
            }
        }
        if (!dual && (rc = settle_q(m))) return rc;
        one_launch = tiles && !switch_tile_split();
        if (!one_launch && !(presorted_big && fwd_fused))     // presorted_big: gathered + sorted ahead, on the second stream
            if ((rc = front_and_sort(m, du, di, dr, B, d_logits, d_store_ids, f, nblk, fin_done, tiles, fwd_fused))) return rc;
    }
    if (tiles) {
        if ((rc = step_small_tiles(m, k, du, di, dr, B, d_logits, d_store_ids, next_store_ids, one_launch, f))) return rc;
        fin_done = true;
    } else if (k.tf1) {
        if ((rc = step_big_tf1(m, k, du, di, B))) return rc;
    } else if (B > 0) {
        if ((rc = step_big_fused(m, k, du, di, dr, B, d_logits, fwd_fused, dual, f, fin_done))) return rc;
        fin_done = true;
    }
    if (!fin_done) {
        f.nblk = nblk;
        Prof p(m, TFR_K_FINALIZE);
        launch_finalize(f, s);
    }
    HIPCHK(hipGetLastError());
    advance_step(m);
    return TFR_OK;
}

// the step counter and the beta powers as an entry point found them: what a voided step is rolled back to
struct StepMark { int64_t step; float b1p, b2p; };
static StepMark mark_step(const tfr_model* m) { return {m->step, m->b1p, m->b2p}; }

static void rollback_step(tfr_model* m, const StepMark& k) {
    m->step = k.step;
    m->b1p = k.b1p;
    m->b2p = k.b2p;
    m->tab_gen += 1;                                     // the voided step may have run: the counter no longer tells
}

// pinned staging for host-fed batches up to 1M ratings (larger ones take the plain copies)
static const int64_t STAGE_MAX = 1 << 20;
static int ensure_staging(tfr_model* m, int64_t B) {
    const int64_t cap = pow2_cap(B);
    forget_kept_batch(m);                                // d_in is about to be rewritten, perhaps reallocated
    HIPCHK(m->d_in.reserve(3 * cap, m->stream));
    HIPCHK(m->h_in.reserve(3 * cap, m->stream));
    HIPCHK(m->h_out.reserve(cap + 4, m->stream));
    return TFR_OK;
}

static int check_batch(const void* u, const void* i, int64_t B) {
    if (B < 0) return fail(TFR_ERR_ARG, "negative batch");
    if (B > 0 && (!u || !i)) return fail(TFR_ERR_ARG, "null id pointer");
    return TFR_OK;
}

// a host batch's three columns into d_u / d_i / d_r (the workspace holds B: ensure_capacity)
static int upload_triples(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t B) {
    forget_kept_batch(m);
    HIPCHK(hipMemcpyAsync(m->d_u, u, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->d_i, i, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->d_r, r, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    return TFR_OK;
}

// `call`: the entry that makes the snapshot of this handle (an FM handle's is tfr_fm_bf16_snapshot)
static int bf16_need_snapshot(const tfr_model* m, const char* call = "tfr_bf16_snapshot") {
    return m->bf.valid ? TFR_OK : fail(TFR_ERR_STATE, "no bf16 snapshot: call %s first", call);
}

// ---- forward ---------------------------------------------------------------------------
// the bodies of tfr_forward_dev / tfr_forward and of their snapshot twins, which differ in `rows` and in the snapshot test
static int forward_dev(tfr_model* m, FwdRows rows, const int32_t* du, const int32_t* di, int64_t B, float* d_logits) {
    int rc = check_batch(du, di, B);
    if (rc) return rc;
    if (rows == ROWS_BF16 && (rc = bf16_need_snapshot(m))) return rc;
    if (B == 0) return TFR_OK;
    if (!d_logits) return fail(TFR_ERR_ARG, "null logits pointer");
    if ((rc = ensure_capacity(m, 1))) return rc;
    return run_forward(m, MODE_INFER, du, di, nullptr, B, d_logits, nullptr, nullptr, nullptr, rows);
}

static int forward_host(tfr_model* m, FwdRows rows, const int32_t* u, const int32_t* i, int64_t B, float* logits_out) {
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (rows == ROWS_BF16 && (rc = bf16_need_snapshot(m))) return rc;
    if (B == 0) return TFR_OK;
    if (!logits_out) return fail(TFR_ERR_ARG, "null logits pointer");
    if ((rc = ensure_capacity(m, B))) return rc;
    forget_kept_batch(m);                                // the logits land in d_logits
    if (B <= STAGE_MAX) {                                // pinned staging: one copy in, one out (+ the error flag)
        if ((rc = ensure_staging(m, B))) return rc;
        memcpy(m->h_in, u, (size_t)B * 4);
        memcpy(m->h_in + B, i, (size_t)B * 4);
        HIPCHK(hipMemcpyAsync(m->d_in, m->h_in, (size_t)2 * B * 4, hipMemcpyHostToDevice, m->stream));
        if ((rc = run_forward(m, MODE_INFER, m->d_in, m->d_in + B, nullptr, B, m->d_logits, nullptr, nullptr, nullptr, rows))) return rc;
        HIPCHK(hipMemcpyAsync(m->h_out, m->d_logits, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
        if ((rc = check_device_error(m))) return rc;
        memcpy(logits_out, m->h_out, (size_t)B * 4);
        return TFR_OK;
    }
    HIPCHK(hipMemcpyAsync(m->d_u, u, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->d_i, i, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    if ((rc = run_forward(m, MODE_INFER, m->d_u, m->d_i, nullptr, B, m->d_logits, nullptr, nullptr, nullptr, rows))) return rc;
    HIPCHK(hipMemcpyAsync(logits_out, m->d_logits, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    return check_device_error(m);
}

extern "C" {

int tfr_forward_dev(tfr_model* m, const int32_t* du, const int32_t* di, int64_t B, float* d_logits) {
    MODEL_ENTER(m);
    return forward_dev(m, ROWS_F32, du, di, B, d_logits);
}

int tfr_forward(tfr_model* m, const int32_t* u, const int32_t* i, int64_t B, float* logits_out) {
    MODEL_ENTER(m);
    return forward_host(m, ROWS_F32, u, i, B, logits_out);
}

// rank-sum AUC of n device scores against device labels (> 0.5 = positive); NaN when a class is empty
static int auc_device(tfr_model* m, const float* d_score, const float* d_label, int64_t n, double* auc_out) {
    int rc;
    if ((rc = ensure_capacity(m, n))) return rc;
    HIPCHK(m->d_auc.reserve(2, m->stream));
    hipStream_t s = m->stream;
    HIPCHK(hipMemsetAsync(m->d_auc, 0, 16, s));
    launch_auc_keys(d_score, m->d_i, n, s);              // d_i: batch-sized int scratch
    HIPCHK(hipGetLastError());
    const int32_t* keys[2] = {m->d_i, nullptr};
    const int bits[2] = {32, 0};
    int32_t* ks[2] = {m->ks_i, nullptr};
    int32_t* ps[2] = {m->ps_i, nullptr};
    if ((rc = radix_sort_columns(m, 1, keys, bits, ks, ps, n))) return rc;
    launch_auc_ranksum(m->ks_i, m->ps_i, d_label, n, m->d_auc, s);
    HIPCHK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, m->d_auc, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double np = (double)h[1], nn = (double)n - np;
    if (auc_out) *auc_out = (np > 0 && nn > 0) ? (0.5 * (double)h[0] - 0.5 * np * (np + 1.0)) / (np * nn) : NAN;
    return TFR_OK;
}

// the AUC needs the kept logits, which only the float32 rows' forward writes
static int eval_device(tfr_model* m, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                       double* sse_out, int64_t* neq_out, double* nll_out = nullptr, double* auc_out = nullptr,
                       FwdRows rows = ROWS_F32) {
    int nblk = 0, rc;
    if (auc_out && (rc = ensure_capacity(m, B))) return rc;
    if (auc_out) forget_kept_batch(m);                   // the logits land in d_logits
    if ((rc = run_forward(m, MODE_EVAL, du, di, dr, B, auc_out ? m->d_logits : nullptr, nullptr, &nblk, nullptr, rows))) return rc;
    std::vector<float> part((size_t)nblk * 4);
    HIPCHK(hipMemcpyAsync(part.data(), m->partials, part.size() * 4, hipMemcpyDeviceToHost, m->stream));
    if ((rc = check_device_error(m))) return rc;
    double sse = 0.0, nll = 0.0;
    int64_t neq = 0;
    for (int b = 0; b < nblk; ++b) {
        sse += (double)part[(size_t)b * 4 + 0];
        neq += (int64_t)llround((double)part[(size_t)b * 4 + 1]);
        nll += (double)part[(size_t)b * 4 + 2];
    }
    if (sse_out) *sse_out = sse;
    if (neq_out) *neq_out = neq;
    if (nll_out) *nll_out = nll;
    if (auc_out) return auc_device(m, m->d_logits, dr, B, auc_out);
    return TFR_OK;
}

int tfr_eval(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t B,
             double* sse_out, int64_t* neq_out) {
    MODEL_ENTER(m);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (sse_out) *sse_out = 0.0;
    if (neq_out) *neq_out = 0;
    if (B == 0) return TFR_OK;
    if (!r) return fail(TFR_ERR_ARG, "null rate pointer");
    if ((rc = ensure_capacity(m, B))) return rc;
    if ((rc = upload_triples(m, u, i, r, B))) return rc;
    return eval_device(m, m->d_u, m->d_i, m->d_r, B, sse_out, neq_out);
}

// ---- bf16 snapshot (bf16_rows.h) -------------------------------------------------------
int tfr_bf16_row_stride(int32_t dim) { return dim < 1 ? 0 : bf16_row_stride(dim); }

int tfr_bf16_snapshot(tfr_model* m) {
    MODEL_ENTER(m);
    int rc = settle_q(m);                                // item rows may live in the two-table step's second table
    if (rc) return rc;
    hipStream_t s = m->stream;
    const int64_t DP = bf16_row_stride(m->D);
    tfr_model::Bf16Snap& b = m->bf;
    b.valid = false;
    b.gen += 1;                                          // the inverse norms of the earlier snapshot are stale from here
    hipError_t e = b.p.reserve(m->U * DP, s);
    if (e == hipSuccess) e = b.q.reserve(m->I * DP, s);
    if (e == hipSuccess) e = b.bu.reserve(m->U, s);
    if (e == hipSuccess) e = b.bi.reserve(m->I, s);
    if (e == hipSuccess) e = b.mu.reserve(1, s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);                   // a refresh: earlier scoring calls may still read the buffers
        b.drop();
        return fail(e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, "tfr_bf16_snapshot: %s", hipGetErrorString(e));
    }
    launch_rows_to_bf16(m->w[TFR_P], b.p, m->U, m->D, s);
    launch_rows_to_bf16(m->w[TFR_Q], b.q, m->I, m->D, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b.bu, m->w[TFR_BU], (size_t)m->U * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(b.bi, m->w[TFR_BI], (size_t)m->I * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(b.mu, m->w[TFR_MU], 4, hipMemcpyDeviceToDevice, s));
    b.valid = true;
    return TFR_OK;
}

int tfr_bf16_drop(tfr_model* m) {
    MODEL_ENTER(m);
    if (m->bf.valid) HIPCHK(hipStreamSynchronize(m->stream));
    m->bf.drop();
    return TFR_OK;
}

int tfr_bf16_forward_dev(tfr_model* m, const int32_t* du, const int32_t* di, int64_t B, float* d_logits) {
    MODEL_ENTER(m);
    return forward_dev(m, ROWS_BF16, du, di, B, d_logits);
}

int tfr_bf16_forward(tfr_model* m, const int32_t* u, const int32_t* i, int64_t B, float* logits_out) {
    MODEL_ENTER(m);
    return forward_host(m, ROWS_BF16, u, i, B, logits_out);
}

int tfr_bf16_eval(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t B,
                  double* sse_out, int64_t* neq_out, double* nll_out) {
    MODEL_ENTER(m);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (sse_out) *sse_out = 0.0;
    if (neq_out) *neq_out = 0;
    if (nll_out) *nll_out = 0.0;
    if ((rc = bf16_need_snapshot(m))) return rc;
    if (B == 0) return TFR_OK;
    if (!r) return fail(TFR_ERR_ARG, "null rate pointer");
    if ((rc = ensure_capacity(m, B))) return rc;
    if ((rc = upload_triples(m, u, i, r, B))) return rc;
    return eval_device(m, m->d_u, m->d_i, m->d_r, B, sse_out, neq_out, nll_out, nullptr, ROWS_BF16);
}

int tfr_bf16_get_rows(tfr_model* m, int32_t which, uint16_t* host, int64_t n) {
    MODEL_ENTER(m);
    if (which != TFR_P && which != TFR_Q) return fail(TFR_ERR_ARG, "tfr_bf16_get_rows: which must be TFR_P or TFR_Q, got %d", which);
    int rc = bf16_need_snapshot(m);
    if (rc) return rc;
    const int64_t cnt = (which == TFR_P ? m->U : m->I) * bf16_row_stride(m->D);
    if (!host || n != cnt) return fail(TFR_ERR_ARG, "bf16 rows of table %d hold %lld elements, asked %lld", which, (long long)cnt, (long long)n);
    HIPCHK(hipMemcpyAsync(host, which == TFR_P ? m->bf.p.get() : m->bf.q.get(), (size_t)n * 2, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_upload_eval_triples(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t N) {
    MODEL_ENTER(m);
    if (N < 1 || !u || !i || !r) return fail(TFR_ERR_ARG, "upload_eval_triples: need n >= 1 and non-null columns");
    HIPCHK(hipStreamSynchronize(m->stream));
    m->ev_n = 0;
    HIPCHK(reserve_each(N, m->stream, m->ev_u, m->ev_i, m->ev_r));
    HIPCHK(hipMemcpyAsync(m->ev_u, u, (size_t)N * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->ev_i, i, (size_t)N * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->ev_r, r, (size_t)N * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->ev_n = N;
    return ensure_capacity(m, 1);
}

/* the fork's epoch line on the device (svd_train_val.py:94-98,170-178): accuracy count, summed sigmoid
 * cross-entropy and AUC of the given batch / the resident validation set */
int tfr_eval_binary(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t B,
                    int64_t* neq_out, double* nll_sum_out, double* auc_out) {
    MODEL_ENTER(m);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (neq_out) *neq_out = 0;
    if (nll_sum_out) *nll_sum_out = 0.0;
    if (auc_out) *auc_out = NAN;
    if (B == 0) return TFR_OK;
    if (!r) return fail(TFR_ERR_ARG, "null rate pointer");
    if (m->o.loss != TFR_LOSS_NLL) return fail(TFR_ERR_STATE, "eval_binary needs the binary-outcome model (loss = nll)");
    if ((rc = ensure_capacity(m, B))) return rc;
    if ((rc = upload_triples(m, u, i, r, B))) return rc;
    // (the AUC reuses d_i as key scratch - after the forward, in stream order, has read the ids)
    return eval_device(m, m->d_u, m->d_i, m->d_r, B, nullptr, neq_out, nll_sum_out, auc_out);
}

int tfr_eval_binary_resident(tfr_model* m, int64_t* neq_out, double* nll_sum_out, double* auc_out, int64_t* n_out) {
    MODEL_ENTER(m);
    if (!m->ev_n) return fail(TFR_ERR_STATE, "no resident validation set: call tfr_upload_eval_triples first");
    if (m->o.loss != TFR_LOSS_NLL) return fail(TFR_ERR_STATE, "eval_binary needs the binary-outcome model (loss = nll)");
    if (n_out) *n_out = m->ev_n;
    return eval_device(m, m->ev_u, m->ev_i, m->ev_r, m->ev_n, nullptr, neq_out, nll_sum_out, auc_out);
}

/* AUC of arbitrary device scores / labels (label > 0.5 = positive): roc_auc_score on the device */
int tfr_auc_dev(tfr_model* m, const float* d_score, const float* d_label, int64_t n, double* auc_out) {
    MODEL_ENTER(m);
    if (n < 1 || !d_score || !d_label || !auc_out) return fail(TFR_ERR_ARG, "auc_dev: bad arguments");
    return auc_device(m, d_score, d_label, n, auc_out);
}

int tfr_eval_resident(tfr_model* m, double* sse_out, int64_t* neq_out, int64_t* n_out) {
    MODEL_ENTER(m);
    if (!m->ev_n) return fail(TFR_ERR_STATE, "no resident validation set: call tfr_upload_eval_triples first");
    if (n_out) *n_out = m->ev_n;
    return eval_device(m, m->ev_u, m->ev_i, m->ev_r, m->ev_n, sse_out, neq_out);
}

// ---- one minibatch ---------------------------------------------------------------------
int tfr_train_step_dev(tfr_model* m, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                       float* d_logits) {
    MODEL_ENTER(m);
    int rc = check_batch(du, di, B);
    if (rc) return rc;
    if (B > 0 && !dr) return fail(TFR_ERR_ARG, "null rate pointer");
    if ((rc = ensure_capacity(m, B > 0 ? B : 1))) return rc;
    return run_train_step(m, du, di, dr, B, d_logits, nullptr);
}

int tfr_train_step(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t B,
                   float* logits_out, float* loss_out, float* reg_out) {
    MODEL_ENTER(m);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (B > 0 && !r) return fail(TFR_ERR_ARG, "null rate pointer");
    if ((rc = ensure_capacity(m, B > 0 ? B : 1))) return rc;
    const StepMark mark = mark_step(m);
    float sc[4] = {0.f, 0.f, 0.f, 0.f};
    forget_kept_batch(m);
    if (B > 0 && B <= STAGE_MAX) {
        // one pinned H2D copy in, the kernels, one D2H copy out: [logits | loss, reg, sum g, error flag]
        if ((rc = ensure_staging(m, B))) return rc;
        memcpy(m->h_in, u, (size_t)B * 4);
        memcpy(m->h_in + B, i, (size_t)B * 4);
        memcpy(m->h_in + 2 * B, r, (size_t)B * 4);
        HIPCHK(hipMemcpyAsync(m->d_in, m->h_in, (size_t)3 * B * 4, hipMemcpyHostToDevice, m->stream));
        const int64_t nl = logits_out ? B : 0;
        float* out4 = m->d_logits + nl;
        if ((rc = run_train_step(m, m->d_in, m->d_in + B, reinterpret_cast<const float*>(m->d_in + 2 * B), B,
                                 logits_out ? m->d_logits : nullptr, out4, nullptr, nullptr, false, true))) return rc;
        HIPCHK(hipMemcpyAsync(m->h_out, m->d_logits, (size_t)(nl + 4) * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        const int32_t e = (int32_t)m->h_out[nl + 3];
        if (e) {                                         // a bad batch never advances the step
            rollback_step(m, mark);
            return device_error(m, e);
        }
        if (logits_out) memcpy(logits_out, m->h_out, (size_t)B * 4);
        sc[0] = m->h_out[nl]; sc[1] = m->h_out[nl + 1];
        m->last_r = logits_out ? reinterpret_cast<const float*>(m->d_in + 2 * B) : nullptr; m->last_B = B;
    } else {
        if (B > 0 && (rc = upload_triples(m, u, i, r, B))) return rc;
        if ((rc = run_train_step(m, m->d_u, m->d_i, m->d_r, B, logits_out ? m->d_logits : nullptr, nullptr))) return rc;
        if (logits_out && B > 0)
            HIPCHK(hipMemcpyAsync(logits_out, m->d_logits, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(sc, m->scalars, 16, hipMemcpyDeviceToHost, m->stream));
        // synchronous entry point: always validate so a bad batch never advances the step
        if ((rc = check_device_error(m))) {
            rollback_step(m, mark);
            return rc;
        }
        if (logits_out && B > 0) { m->last_r = m->d_r; m->last_B = B; }
    }
    if (loss_out) *loss_out = sc[0];
    if (reg_out) *reg_out = sc[1];
    return TFR_OK;
}

int tfr_train_steps_repeat(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t B, int32_t nsteps,
                           float* logits_out, float* loss_out) {
    MODEL_ENTER(m);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (B < 1 || !r) return fail(TFR_ERR_ARG, "train_steps_repeat: need a batch of at least one rating");
    if (nsteps < 0) return fail(TFR_ERR_ARG, "bad nsteps");
    if (nsteps == 0) return TFR_OK;
    if ((rc = ensure_capacity(m, B))) return rc;
    if (loss_out) HIPCHK(m->step_out.reserve((int64_t)nsteps * 4, m->stream));
    const StepMark mark = mark_step(m);
    if ((rc = upload_triples(m, u, i, r, B))) return rc;
    for (int32_t s = 0; s < nsteps; ++s) {
        const bool last = s + 1 == nsteps;
        if ((rc = run_train_step(m, m->d_u, m->d_i, m->d_r, B, (last && logits_out) ? m->d_logits : nullptr,
                                 loss_out ? m->step_out + (size_t)s * 4 : nullptr))) {
            (void)hipStreamSynchronize(m->stream);
            rollback_step(m, mark);
            return rc;
        }
    }
    std::vector<float> tmp;
    if (loss_out) {
        tmp.resize((size_t)nsteps * 4);
        HIPCHK(hipMemcpyAsync(tmp.data(), m->step_out, tmp.size() * 4, hipMemcpyDeviceToHost, m->stream));
    }
    if (logits_out) HIPCHK(hipMemcpyAsync(logits_out, m->d_logits, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    if ((rc = check_device_error(m))) {                    // a bad id voids every step of the call
        rollback_step(m, mark);
        return rc;
    }
    for (int32_t s = 0; loss_out && s < nsteps; ++s) loss_out[s] = tmp[(size_t)s * 4];
    if (logits_out) { m->last_r = m->d_r; m->last_B = B; }
    return TFR_OK;
}

/* roc_auc_score(rates, sigmoid(logits)) of the batch the last tfr_train_step / tfr_train_steps_repeat ran on (its pre-update
 * logits, the ones the caller was handed): svd_train_val.py:97, without sklearn on the host.  Needs that call to have asked
 * for logits, and nothing since to have trained or used the batch workspace (forget_kept_batch): TFR_ERR_STATE otherwise. */
int tfr_last_batch_auc(tfr_model* m, double* auc_out) {
    MODEL_ENTER(m);
    if (!auc_out) return fail(TFR_ERR_ARG, "null output");
    if (!m->last_r || m->last_B < 1) return fail(TFR_ERR_STATE, "no kept batch: tfr_last_batch_auc follows a tfr_train_step / tfr_train_steps_repeat that returned logits, "
                                                                "with no training, forward or evaluation call in between");
    return auc_device(m, m->d_logits, m->last_r, m->last_B, auc_out);
}

// ---- resident store --------------------------------------------------------------------
// pack three columns (host or device) into the 16-byte-record store, in chunks
static int build_store(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t N, bool on_device) {
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->spec_valid) { int rc0 = cancel_run_ahead(m); if (rc0) return rc0; }     // ids drawn ahead were for the old store size
    m->N = 0; m->pf_valid = false;
    recs_forget(m);
    HIPCHK(m->store.reserve(N, m->stream));
    if (on_device) {
        launch_pack_triples(u, i, r, m->store, N, m->stream);
        HIPCHK(hipGetLastError());
    } else {
        const int64_t chunk = (int64_t)1 << 24;
        DevBuf<int32_t> tu, ti;
        DevBuf<float> tr;
        HIPCHK(reserve_each(N < chunk ? N : chunk, m->stream, tu, ti, tr));
        hipError_t e = hipSuccess;
        for (int64_t off = 0; off < N && e == hipSuccess; off += chunk) {
            const int64_t n = (N - off < chunk) ? N - off : chunk;
            e = hipMemcpyAsync(tu, u + off, (size_t)n * 4, hipMemcpyHostToDevice, m->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(ti, i + off, (size_t)n * 4, hipMemcpyHostToDevice, m->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(tr, r + off, (size_t)n * 4, hipMemcpyHostToDevice, m->stream);
            if (e == hipSuccess) {
                launch_pack_triples(tu, ti, tr, m->store + off, n, m->stream);
                e = hipStreamSynchronize(m->stream);
            }
        }
        if (e != hipSuccess) return fail(TFR_ERR_HIP, "upload_triples: %s", hipGetErrorString(e));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    m->N = N;
    return TFR_OK;
}

int tfr_upload_triples(tfr_model* m, const int32_t* u, const int32_t* i, const float* r, int64_t N) {
    MODEL_ENTER(m);
    if (N < 1 || !u || !i || !r) return fail(TFR_ERR_ARG, "upload_triples: need n >= 1 and non-null columns");
    return build_store(m, u, i, r, N, false);
}

int tfr_set_triples_dev(tfr_model* m, const int32_t* du, const int32_t* di, const float* dr, int64_t N) {
    MODEL_ENTER(m);
    if (N < 1 || !du || !di || !dr) return fail(TFR_ERR_ARG, "set_triples_dev: need n >= 1 and non-null columns");
    return build_store(m, du, di, dr, N, true);
}

int tfr_init_tables(tfr_model* m, uint64_t seed, float fstd, float bstd) {
    MODEL_ENTER(m);
    hipStream_t s = m->stream;
    if (m->q_dirty) {                                    // fresh tables: every row lives in the main table again
        HIPCHK(hipMemsetAsync(m->q_sel, 0, (size_t)m->I * 4, s));
        m->q_dirty = false;
    }
    launch_init_trunc_normal(m->w[TFR_P], m->n[TFR_P], fstd, seed * 4 + 0, s);
    launch_init_trunc_normal(m->w[TFR_Q], m->n[TFR_Q], fstd, seed * 4 + 1, s);
    launch_init_trunc_normal(m->w[TFR_BU], m->n[TFR_BU], bstd, seed * 4 + 2, s);
    launch_init_trunc_normal(m->w[TFR_BI], m->n[TFR_BI], bstd, seed * 4 + 3, s);
    launch_init_uniform_scalar(m->w[TFR_MU], -1.7320508f, 1.7320508f, seed, s);
    HIPCHK(hipGetLastError());
    for (int t = 0; t < 5; ++t) {
        if (m->m[t]) HIPCHK(hipMemsetAsync(m->m[t], 0, (size_t)m->n[t] * 4, s));
        if (m->v[t]) HIPCHK(hipMemsetAsync(m->v[t], 0, (size_t)m->n[t] * 4, s));
    }
    m->step = 0;
    m->b1p = m->o.beta1;
    m->b2p = m->o.beta2;
    m->tab_gen += 1;
    HIPCHK(hipStreamSynchronize(s));
    return TFR_OK;
}

static const int64_t IDS_MIN_CAP = (int64_t)1 << 24;   // 128 MB: a 900-step call at batch 10000 fits without reallocating
// room for n staged ids (contents undefined afterwards); the stream must be idle
static int ensure_ids(tfr_model* m, int64_t n) {
    m->n_ids = 0; m->pf_valid = false;
    m->ids.n_recs = 0;
    // allocations are slow: never size for a short call only
    HIPCHK(m->ids.ids.reserve(n < IDS_MIN_CAP ? IDS_MIN_CAP : n, m->stream3 ? m->stream3 : m->stream));
    return TFR_OK;
}

int tfr_stage_ids(tfr_model* m, const int64_t* ids, int64_t n) {
    MODEL_ENTER(m);
    if (n < 1 || !ids) return fail(TFR_ERR_ARG, "stage_ids: need n >= 1 and non-null ids");
    HIPCHK(hipStreamSynchronize(m->stream));
    int rc;
    if ((rc = ensure_ids(m, n))) return rc;
    HIPCHK(hipMemcpyAsync(m->ids.ids, ids, (size_t)n * 8, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->n_ids = n;
    return TFR_OK;
}

static int gather_batch(tfr_model* m, const int64_t* d_ids, int64_t lo, int64_t B) {
    GatherArgs g;
    g.ids = d_ids; g.lo = lo; g.B = B; g.N = m->N;
    g.store = m->store;
    g.u = m->d_u; g.it = m->d_i; g.r = m->d_r; g.err = m->d_err;
    forget_kept_batch(m);
    {
        Prof p(m, TFR_K_GATHER);
        launch_gather(g, m->stream);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

static void swap_sortset(tfr_model* m) {
    std::swap(m->d_u, m->alt.d_u); std::swap(m->d_i, m->alt.d_i); std::swap(m->d_r, m->alt.d_r);
    std::swap(m->ks_u, m->alt.ks_u); std::swap(m->ps_u, m->alt.ps_u);
    std::swap(m->ks_i, m->alt.ks_i); std::swap(m->ps_i, m->alt.ps_i);
}

static int ensure_lookahead(tfr_model* m) {
    tfr_model::SortSet& A = m->alt;
    HIPCHK(reserve_each(m->cap, m->stream, A.d_u, A.d_i, A.d_r, A.ks_u, A.ps_u, A.ks_i, A.ps_i));
    if (!m->stream2) {
        // (tried, one gpurun call each, C3 step: a high-priority look-ahead stream - no change; the look-ahead stream
        // confined to 8 / 16 / 32 / 64 CUs by hipExtStreamCreateWithCUMask - 1070 / 717 / 584 / 487 us against 497-504)
        HIPCHK(hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking));
        for (int z = 0; z < 2; ++z) {
            HIPCHK(hipEventCreateWithFlags(&m->ev_sorted[z], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&m->ev_free[z], hipEventDisableTiming));
        }
        HIPCHK(hipEventCreateWithFlags(&m->ev_first, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&m->ev_mid, hipEventDisableTiming));
    }
    return TFR_OK;
}

// Big tables, touched-rows optimiser: gather + radix sort (+ id range check) of batch s+1 do not depend
// on the tables, are a few small latency-bound launches, and would otherwise head every step; they run
// on a second stream into the alternate buffer set while step s's HBM-bound kernels own the CUs.
// mask of legacy randint's rejection loop: smallest 2^k - 1 >= rng
static uint32_t mask_for(uint32_t rng) {
    uint32_t mk = rng;
    mk |= mk >> 1; mk |= mk >> 2; mk |= mk >> 4; mk |= mk >> 8; mk |= mk >> 16;
    return mk;
}

// Steps whose ids are drawn on the side stream (tfr_train_steps_drawn).  The draws are cut into chunks of whole steps -
// small ones first, so the first steps start after two batches' worth of draws, then doubling while the generator's
// lead over the steps allows it - and a chunk is ENQUEUED when the step loop needs it (need) or one at a time after a step's
// own launches (feed): the host never spends a stretch feeding the draw stream while the main stream sits empty (a 20-step
// call: the first step used to start 36 us into the call, behind six draw launches).
// need(step, stream) makes `stream` wait for the chunk that holds that step's ids.  NULL = ids staged by the host.
static int enqueue_run_ahead(tfr_model* m, int64_t B, int64_t nsteps, uint32_t rng);

struct IdsReady {
    tfr_model* m = nullptr;
    int64_t B = 0, nsteps = 0;
    uint32_t rng = 0;
    bool ahead_done = false;
    std::vector<int64_t> first;                            // first[c] = first step of chunk c; first[nchunks] = nsteps
    int enq = 0;                                           // chunks enqueued so far
    int waited[2] = {-1, -1};                              // highest chunk waited for: [0] main stream, [1] stream2
    int64_t pre = 0;                                       // pre: steps whose ids the previous call drew ahead (chunk 0, event spec_ev)
    int chunk_of(int64_t step) const {
        int c = 0;
        while (c + 1 < (int)first.size() - 1 && first[c + 1] <= step) ++c;
        return c;
    }
    void plan(int64_t cap_steps, int64_t pre_steps) {
        first.clear();
        pre = pre_steps;
        int64_t s = 0, n = pre ? pre : (nsteps < 2 ? nsteps : 2), done = 0;
        enq = pre ? 1 : 0;
        while (s < nsteps) {
            first.push_back(s);
            s += n; done += n;
            // next size: 1 while little has been drawn, then roughly half of what is already behind (the generator is at
            // most ~1.5x faster than a small-table step, so its lead grows by about a third of a step per step)
            n = done / 3;
            if (n < 1) n = 1;
            if (n > cap_steps) n = cap_steps;
            if (s + n > nsteps) n = nsteps - s;
        }
        first.push_back(nsteps);
    }
    // every chunk that starts at or before `step`, and at most `extra` more
    int enqueue_through(int64_t step, int extra = 0) {
        const int nch = (int)first.size() - 1;
        while (enq < nch && (first[enq] <= step || extra-- > 0)) {
            const int c = enq++;
            while ((int)m->chunk_ev.size() <= c) {
                hipEvent_t e;
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(TFR_ERR_HIP, "hipEventCreate failed");
                m->chunk_ev.push_back(e);
            }
            const int64_t s0 = first[c], s1 = first[c + 1];
            hipEvent_t pa = nullptr, pb = nullptr;
            if (m->prof && hipEventCreate(&pa) == hipSuccess && hipEventCreate(&pb) == hipSuccess) (void)hipEventRecord(pa, m->stream3);
            if (rng != 0) {
                launch_mt_draw(m->d_rng, m->ids.ids + s0 * B, (s1 - s0) * B, rng, mask_for(rng), m->stream3, nullptr, &m->rng_ws);
                recs_follow(m, m->ids, s0 * B, (s1 - s0) * B, m->stream3);
            }
            if (pa && pb) { (void)hipEventRecord(pb, m->stream3); m->events.push_back({pa, pb, TFR_K_DRAW}); }
            if (hipGetLastError() != hipSuccess || hipEventRecord(m->chunk_ev[c], m->stream3) != hipSuccess)
                return fail(TFR_ERR_HIP, "draw launch failed");
        }
        return TFR_OK;
    }
    // after a step's launches: one more chunk for the draw stream (never before them - with ids drawn ahead by the previous
    // call the first step must not queue behind draw launches it does not need; one per step keeps the host ahead of a
    // 20-us step and the generator busy from the start, so the run-ahead draw at the end of the call fits inside it)
    int feed(int64_t step) { return enqueue_through(step, 1); }
    int run_ahead() {
        if (ahead_done) return TFR_OK;
        ahead_done = true;
        return enqueue_run_ahead(m, B, nsteps, rng);
    }
    int need(int64_t step, hipStream_t st, int which) {
        if (step >= nsteps) step = nsteps - 1;
        int rc = enqueue_through(step);
        if (rc) return rc;
        const int c = chunk_of(step);
        if (c > waited[which]) {                           // chunks complete in order on the draw stream
            if (hipStreamWaitEvent(st, (c == 0 && pre) ? m->spec_ev : m->chunk_ev[c], 0) != hipSuccess)
                return fail(TFR_ERR_HIP, "hipStreamWaitEvent failed");
            waited[which] = c;                             // (skipping the wait when hipEventQuery says "done": no gain, A/B)
        }
        return TFR_OK;
    }
};

static int staged_steps_lookahead(tfr_model* m, int64_t first_step, int64_t B, int32_t nsteps, float* loss_out, IdsReady* ready) {
    int rc;
    if ((rc = ensure_lookahead(m))) return rc;
    hipStream_t main_s = m->stream;
    FinArgs fdummy;
    memset(&fdummy, 0, sizeof(fdummy));
    int nb0 = 0;
    bool fd0 = false;
    auto sort_batch = [&](int64_t step) -> int {           // into the buffer set the model currently points at
        const int32_t* du = m->d_u; const int32_t* di = m->d_i; const float* dr = m->d_r;
        if (ready) { const int e = ready->need(first_step + step, m->stream, m->stream == main_s ? 0 : 1); if (e) return e; }
        return front_and_sort(m, du, di, dr, B, nullptr, m->ids.ids + (first_step + step) * B, fdummy, nb0, fd0, false, true);
    };
    if ((rc = sort_batch(0))) return rc;
    HIPCHK(hipEventRecord(m->ev_first, main_s));
    // the next batch's sort chain starts beside the user-side kernel of this step (after the item-side one, which runs the
    // forward and suffers more from company): three A/B pairs in one gpurun call, 494/519/537 -> 489/512/523 us per step.
    // TFR_SORT_LATE=0: start it beside the item-side kernel (the round-1 order), kept for A/B
    static const bool late = env_default_on("TFR_SORT_LATE");
    if (late) {
        m->ev_mid_on = true;
        for (int32_t s = 0; s < nsteps && !rc; ++s) {
            const int z = s & 1;
            if (s > 0) HIPCHK(hipStreamWaitEvent(main_s, m->ev_sorted[z], 0));
            if ((rc = run_train_step(m, m->d_u, m->d_i, m->d_r, B, nullptr, loss_out ? m->step_out + (size_t)s * 4 : nullptr,
                                     m->ids.ids + (first_step + s) * B, nullptr, true)))
                break;
            HIPCHK(hipEventRecord(m->ev_free[z], main_s));
            if (ready && (rc = ready->feed(first_step + s))) break;
            if (s + 1 < nsteps) {
                swap_sortset(m);                           // the next step's set: free since step s-1, which the main stream has passed
                HIPCHK(hipStreamWaitEvent(m->stream2, m->ev_mid, 0));
                m->stream = m->stream2;
                rc = sort_batch(s + 1);
                m->stream = main_s;
                if (!rc) rc = hipEventRecord(m->ev_sorted[z ^ 1], m->stream2) == hipSuccess ? TFR_OK : fail(TFR_ERR_HIP, "event record");
            }
        }
        m->ev_mid_on = false;
        HIPCHK(hipStreamSynchronize(m->stream2));
        return rc;
    }
    for (int32_t s = 0; s < nsteps; ++s) {
        const int z = s & 1;
        if (s + 1 < nsteps) {
            swap_sortset(m);                               // the other set: target of the look-ahead sort
            if (s == 0) HIPCHK(hipStreamWaitEvent(m->stream2, m->ev_first, 0));      // sort scratch is shared
            else HIPCHK(hipStreamWaitEvent(m->stream2, m->ev_free[z ^ 1], 0));       // step s-1 has finished with this set
            m->stream = m->stream2;
            rc = sort_batch(s + 1);
            m->stream = main_s;
            if (!rc) rc = hipEventRecord(m->ev_sorted[z ^ 1], m->stream2) == hipSuccess ? TFR_OK : fail(TFR_ERR_HIP, "event record");
            swap_sortset(m);
            if (rc) return rc;
        }
        if (s > 0) HIPCHK(hipStreamWaitEvent(main_s, m->ev_sorted[z], 0));
        if ((rc = run_train_step(m, m->d_u, m->d_i, m->d_r, B, nullptr, loss_out ? m->step_out + (size_t)s * 4 : nullptr,
                                 m->ids.ids + (first_step + s) * B, nullptr, true)))
            return rc;
        HIPCHK(hipEventRecord(m->ev_free[z], main_s));
        if (ready && (rc = ready->feed(first_step + s))) return rc;
        if (s + 1 < nsteps) swap_sortset(m);               // the next step's batch lives in the other set
    }
    HIPCHK(hipStreamSynchronize(m->stream2));              // nothing of ours is left in flight on the side stream
    return TFR_OK;
}

static int staged_steps(tfr_model* m, int64_t first_step, int64_t B, int32_t nsteps, float* loss_out, IdsReady* ready = nullptr) {
    int rc;
    if ((rc = ensure_capacity(m, B))) return rc;
    if (loss_out) HIPCHK(m->step_out.reserve((int64_t)nsteps * 4, m->stream));
    const StepMark mark = mark_step(m);
    static const bool no_ahead = env_default_off("TFR_NO_LOOKAHEAD");   // TFR_NO_LOOKAHEAD=1: A/B switch
    if (nsteps > 1 && fwd_in_reduce(m, B) && !m->prof && !no_ahead) {
        if ((rc = staged_steps_lookahead(m, first_step, B, nsteps, loss_out, ready))) {
            (void)hipStreamSynchronize(m->stream2);
            return rc;
        }
    } else {
    for (int32_t s = 0; s < nsteps; ++s) {
        if (ready && (rc = ready->need(first_step + s + ((first_step + s + 2) * B <= m->n_ids ? 1 : 0), m->stream, 0))) return rc;
        // look ahead past the end of this call too when more staged batches follow: the
        // next call then starts presorted (the sort is free, hidden in this launch)
        const int64_t* nxt = (first_step + s + 2) * B <= m->n_ids ? m->ids.ids + (first_step + s + 1) * B : nullptr;
        if ((rc = run_train_step(m, m->d_u, m->d_i, m->d_r, B, nullptr,
                                 loss_out ? m->step_out + (size_t)s * 4 : nullptr,
                                 m->ids.ids + (first_step + s) * B, nxt))) {
            m->pf_valid = false;
            return rc;
        }
        if (ready && (rc = ready->feed(first_step + s))) return rc;
    }
    }
    if (loss_out) {
        std::vector<float> tmp((size_t)nsteps * 4);
        HIPCHK(hipMemcpyAsync(tmp.data(), m->step_out, tmp.size() * 4, hipMemcpyDeviceToHost, m->stream));
        if ((rc = check_device_error(m))) {
            rollback_step(m, mark);
            m->pf_valid = false;
            return rc;
        }
        for (int32_t s = 0; s < nsteps; ++s) loss_out[s] = tmp[(size_t)s * 4];
    }
    return TFR_OK;
}

int tfr_train_steps_staged(tfr_model* m, int64_t first_step, int64_t B, int32_t nsteps, float* loss_out) {
    MODEL_ENTER(m);
    if (!m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples first");
    if (!m->ids.ids) return fail(TFR_ERR_STATE, "no staged ids: call tfr_stage_ids first");
    if (B < 1 || nsteps < 0 || first_step < 0) return fail(TFR_ERR_ARG, "bad batch/nsteps/first_step");
    if ((first_step + nsteps) * B > m->n_ids)
        return fail(TFR_ERR_ARG, "steps [%lld,%lld) x batch %lld exceed the %lld staged ids", (long long)first_step,
                    (long long)(first_step + nsteps), (long long)B, (long long)m->n_ids);
    CallTrace tr("steps_staged");
    const int rc = staged_steps(m, first_step, B, nsteps, loss_out);
    tr.mark("all steps enqueued");
    return rc;
}

int tfr_train_steps_resident(tfr_model* m, const int64_t* ids, int64_t B, int32_t nsteps, float* loss_out) {
    MODEL_ENTER(m);
    if (!m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples first");
    if (B < 1 || nsteps < 0 || !ids) return fail(TFR_ERR_ARG, "bad batch/nsteps/ids");
    if (nsteps == 0) return TFR_OK;
    int rc = tfr_stage_ids(m, ids, B * nsteps);
    if (rc) return rc;
    return staged_steps(m, 0, B, nsteps, loss_out);
}

// ---- device id draw (rng.hip) ------------------------------------------------------------
static int ensure_rng(tfr_model* m) {
    HIPCHK(reserve_each(625, m->stream, m->d_rng, m->d_rng_snap));
    // scratch of the wide draw; TFR_RNG_WIDE=0 keeps every draw on the one-workgroup kernel (A/B)
    if (env_default_on("TFR_RNG_WIDE")) {
        HIPCHK(m->rng_raw.reserve(MT_WIDE_BLOCKS * 624, m->stream));
        HIPCHK(m->rng_counts.reserve(MT_WIDE_BLOCKS, m->stream));
        HIPCHK(m->rng_hdr.reserve(4, m->stream));
        m->rng_ws = {m->rng_raw, m->rng_counts, m->rng_hdr, MT_WIDE_BLOCKS};
    }
    if (!m->stream3) {
        HIPCHK(hipStreamCreateWithFlags(&m->stream3, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&m->ev_ids_free, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&m->spec_ev, hipEventDisableTiming));
    }
    return TFR_OK;
}

// forget the ids drawn ahead for a call that is not coming: the generator returns to where the consumed ids end
static int cancel_run_ahead(tfr_model* m) {
    if (m->spec_valid) {
        m->spec_valid = false;
        HIPCHK(hipMemcpyAsync(m->d_rng, m->d_rng_snap, 625 * 4, hipMemcpyDeviceToDevice, m->stream3));
    }
    return TFR_OK;
}

int tfr_rng_set_state(tfr_model* m, const uint32_t* key, int32_t pos) {
    MODEL_ENTER(m);
    if (!key || pos < 0 || pos > 624) return fail(TFR_ERR_ARG, "rng_set_state: need key[624] and pos in [0, 624]");
    int rc;
    if ((rc = ensure_rng(m))) return rc;
    m->spec_valid = false;                                 // the new state replaces whatever was drawn ahead
    HIPCHK(hipStreamSynchronize(m->stream3));
    uint32_t h[625];
    memcpy(h, key, 624 * 4);
    h[624] = (uint32_t)pos;
    HIPCHK(hipMemcpy(m->d_rng, h, sizeof(h), hipMemcpyHostToDevice));
    m->rng_set = true;
    return TFR_OK;
}

int tfr_rng_seed(tfr_model* m, uint32_t seed) {
    // init_genrand of MT19937 = what np.random.seed(int) does [NumPy-lib: _legacy_seeding -> mt19937_seed]
    uint32_t key[624];
    key[0] = seed;
    for (int i = 1; i < 624; ++i) key[i] = 1812433253u * (key[i - 1] ^ (key[i - 1] >> 30)) + (uint32_t)i;
    return tfr_rng_set_state(m, key, 624);
}

int tfr_rng_get_state(tfr_model* m, uint32_t* key, int32_t* pos) {
    MODEL_ENTER(m);
    if (!m->rng_set) return fail(TFR_ERR_STATE, "no generator state: call tfr_rng_seed / tfr_rng_set_state first");
    int rc;
    if ((rc = cancel_run_ahead(m))) return rc;
    HIPCHK(hipStreamSynchronize(m->stream3));
    uint32_t h[625];
    HIPCHK(hipMemcpy(h, m->d_rng, sizeof(h), hipMemcpyDeviceToHost));
    if (key) memcpy(key, h, 624 * 4);
    if (pos) *pos = (int32_t)h[624];
    return TFR_OK;
}

static int check_high(int64_t high) {
    if (high < 1 || high > ((int64_t)1 << 32))
        return fail(TFR_ERR_ARG, "randint(0, high): high must be in [1, 2^32] (NumPy draws 64-bit words beyond that)");
    return TFR_OK;
}

int tfr_draw_ids(tfr_model* m, int64_t high, int64_t count, int64_t* ids_out) {
    MODEL_ENTER(m);
    int rc;
    if ((rc = check_high(high))) return rc;
    if (count < 0 || (count > 0 && !ids_out)) return fail(TFR_ERR_ARG, "draw_ids: bad count / null output");
    if (!m->rng_set) return fail(TFR_ERR_STATE, "no generator state: call tfr_rng_seed / tfr_rng_set_state first");
    if (count == 0) return TFR_OK;
    if (high == 1) { memset(ids_out, 0, (size_t)count * 8); return TFR_OK; }    // rng == 0: no draw is consumed
    if ((rc = cancel_run_ahead(m))) return rc;
    DevBuf<int64_t> d;
    HIPCHK(d.reserve(count, m->stream3));
    const uint32_t rng = (uint32_t)(high - 1);
    DevBuf<unsigned long long> dbg;
    if (env_is_set("TFR_RNG_DEBUG") && dbg.reserve(2, m->stream3) != hipSuccess) (void)hipGetLastError();   // diagnostic: in-kernel clock of the generator
    launch_mt_draw(m->d_rng, d, count, rng, mask_for(rng), m->stream3, dbg, &m->rng_ws);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ids_out, d, (size_t)count * 8, hipMemcpyDeviceToHost, m->stream3);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream3);
    if (dbg && e == hipSuccess) {
        unsigned long long h[2] = {0, 0};
        (void)hipMemcpy(h, dbg, 16, hipMemcpyDeviceToHost);
        fprintf(stderr, "k_mt_draw: %lld ids, %llu shader cycles, %.1f us, %.0f MHz, %.1f cycles per 624-word block (mask %u, rng %u)\n",
                (long long)count, h[0], h[1] / 100.0, h[1] ? h[0] * 100.0 / h[1] : 0.0,
                h[0] / ((double)count * ((double)mask_for(rng) + 1.0) / ((double)rng + 1.0) / 624.0), mask_for(rng), rng);
    }
    if (e != hipSuccess) return fail(TFR_ERR_HIP, "draw_ids: %s", hipGetErrorString(e));
    return TFR_OK;
}

int tfr_draw_ids_dev(tfr_model* m, int64_t high, int64_t count, int64_t* d_ids_out) {
    MODEL_ENTER(m);
    int rc;
    if ((rc = check_high(high))) return rc;
    if (count < 0 || (count > 0 && !d_ids_out)) return fail(TFR_ERR_ARG, "draw_ids_dev: bad count / null output");
    if (!m->rng_set) return fail(TFR_ERR_STATE, "no generator state: call tfr_rng_seed / tfr_rng_set_state first");
    if (count == 0) return TFR_OK;
    if ((rc = cancel_run_ahead(m))) return rc;
    hipEvent_t& dev = m->draw_evs[m->draw_count % tfr_model::DRAW_RING];
    if (!dev) HIPCHK(hipEventCreateWithFlags(&dev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(m->ev_ids_free, m->stream));     // the buffer's readers queued so far
    HIPCHK(hipStreamWaitEvent(m->stream3, m->ev_ids_free, 0));
    if (high == 1) {                                       // rng == 0: no draw is consumed
        HIPCHK(hipMemsetAsync(d_ids_out, 0, (size_t)count * 8, m->stream3));
    } else {
        const uint32_t rng = (uint32_t)(high - 1);
        launch_mt_draw(m->d_rng, d_ids_out, count, rng, mask_for(rng), m->stream3, nullptr, &m->rng_ws);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(dev, m->stream3));
    m->draw_count += 1;
    for (IdBuf* b : {&m->ids, &m->ids_alt}) {              // a draw into one of the model's id buffers rewrites it
        if (!ids_overlap(*b, d_ids_out, count)) continue;
        b->n_recs = 0;
        if (m->pf_valid && ids_overlap(*b, m->pf_ids, 1)) m->pf_valid = false;
    }
    return TFR_OK;
}

// the model's stream waits for the first `ordinal` draws issued by tfr_draw_ids_dev (1-based count; draws complete in issue
// order).  A draw whose event slot has been reused by a later draw is covered by waiting for that later one.
static int join_draw_upto(tfr_model* m, int64_t ordinal) {
    if (ordinal > m->draw_count) ordinal = m->draw_count;
    if (ordinal <= m->draw_joined) return TFR_OK;
    int64_t k = ordinal - 1;                                   // index of the draw to wait for
    while (k + tfr_model::DRAW_RING < m->draw_count) k += tfr_model::DRAW_RING;   // its slot now holds a later draw of the same residue
    HIPCHK(hipStreamWaitEvent(m->stream, m->draw_evs[k % tfr_model::DRAW_RING], 0));
    m->draw_joined = k + 1 > ordinal ? ordinal : k + 1;
    if (k + 1 > m->draw_joined) m->draw_joined = k + 1;
    return TFR_OK;
}

int tfr_join_draws(tfr_model* m) {
    MODEL_ENTER(m);
    return join_draw_upto(m, m->draw_count);
}

int tfr_join_draw(tfr_model* m, int64_t ordinal) {
    MODEL_ENTER(m);
    if (ordinal < 1) return fail(TFR_ERR_ARG, "join_draw: ordinal counts issued draws from 1");
    return join_draw_upto(m, ordinal);
}

// run ahead: the next call's first batches, drawn into the other id buffer (last read by the call before the current one)
static int enqueue_run_ahead(tfr_model* m, int64_t B, int64_t nsteps, uint32_t rng) {
    if (rng != 0) {
        int64_t spec = 131072 / B;
        if (spec > 8) spec = 8;
        if (spec > nsteps) spec = nsteps;
        if (spec < 1) spec = 1;
        DevBuf<int64_t>& alt = m->ids_alt.ids;
        const int64_t cap = m->ids.ids.capacity();
        if (spec * B > alt.capacity() || alt.capacity() < cap) {   // keep both buffers the same size: a repeat of this call then fits
            HIPCHK(hipStreamSynchronize(m->stream));       // the old alternate buffer may still be read by queued steps
            m->ids_alt.n_recs = 0;
            int64_t want = spec * B > cap ? spec * B : cap;
            if (want < IDS_MIN_CAP) want = IDS_MIN_CAP;
            HIPCHK(alt.reserve(want, m->stream3));
        }
        HIPCHK(hipStreamWaitEvent(m->stream3, m->ev_ids_free, 0));  // the alternate buffer's last readers (before this call) are done
        HIPCHK(hipMemcpyAsync(m->d_rng_snap, m->d_rng, 625 * 4, hipMemcpyDeviceToDevice, m->stream3));
        launch_mt_draw(m->d_rng, alt, spec * B, rng, mask_for(rng), m->stream3, nullptr, &m->rng_ws);
        recs_follow(m, m->ids_alt, 0, spec * B, m->stream3);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(m->spec_ev, m->stream3));
        m->spec_valid = true; m->spec_B = B; m->spec_N = m->N; m->spec_steps = spec;
    }
    return TFR_OK;
}

int tfr_train_steps_drawn(tfr_model* m, int64_t B, int32_t nsteps, float* loss_out) {
    MODEL_ENTER(m);
    if (!m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples first");
    if (!m->rng_set) return fail(TFR_ERR_STATE, "no generator state: call tfr_rng_seed / tfr_rng_set_state first");
    if (B < 1 || nsteps < 0) return fail(TFR_ERR_ARG, "bad batch/nsteps");
    if (nsteps == 0) return TFR_OK;
    int rc;
    if ((rc = check_high(m->N))) return rc;
    CallTrace tr("steps_drawn");
    const int64_t total = B * (int64_t)nsteps;
    const uint32_t rng = (uint32_t)(m->N - 1);
    int64_t pre = 0;
    if (m->spec_valid && m->spec_B == B && m->spec_N == m->N && nsteps >= m->spec_steps) {
        // the previous call left the first spec_steps batches of this one in the alternate buffer
        pre = m->spec_steps;
        m->spec_valid = false;
        std::swap(m->ids, m->ids_alt);                     // (each id buffer with its records)
        if (total > m->ids.ids.capacity()) {               // grow, keeping the head (rare: a longer call than ever before)
            HIPCHK(hipStreamSynchronize(m->stream3));
            IdBuf bigger;
            HIPCHK(bigger.ids.reserve(total, m->stream3));  // total > capacity >= IDS_MIN_CAP
            HIPCHK(hipMemcpy(bigger.ids, m->ids.ids, (size_t)pre * B * 8, hipMemcpyDeviceToDevice));
            m->ids = std::move(bigger);
            recs_follow(m, m->ids, 0, pre * B, m->stream3);
        }
        HIPCHK(hipEventRecord(m->ev_ids_free, m->stream));          // everything queued so far: the earlier calls' steps
    } else {
        if ((rc = cancel_run_ahead(m))) return rc;
        if (total > m->ids.ids.capacity()) {               // (re)allocation: nothing may still read the old buffer
            HIPCHK(hipStreamSynchronize(m->stream));
            if ((rc = ensure_ids(m, total))) return rc;
        }
        // the draws overwrite the id buffer: they may start once every step already queued has read it
        HIPCHK(hipEventRecord(m->ev_ids_free, m->stream));
        HIPCHK(hipStreamWaitEvent(m->stream3, m->ev_ids_free, 0));
        m->ids.n_recs = 0;
    }
    m->pf_valid = false;                                   // the buffer's contents change: no published look-ahead sort survives
    m->n_ids = total;
    IdsReady ready;
    ready.m = m; ready.B = B; ready.nsteps = nsteps; ready.rng = rng;
    // How large a chunk may grow.  Every chunk costs the small-table step's stream about 4 us (the wait for its event, the five
    // launches of its draw beside the steps): at 6 steps per chunk, 0.6 us of a 16.7-us step.  plan()'s
    // growth rule alone keeps the generator ahead of the steps, so the cap only bounds how many steps wait behind one draw where
    // the generator is the slower of the two: 256 steps (at most 2^22 ids, one pass of the wide draw: a small-table batch is
    // <= 16 tiles) on the small-table path, TFR_CHUNK_STEPS=<n> for A/B (6 = the former cap at the headline batch); the
    // big-table step keeps ~64K ids / 16 steps.
    static const int64_t tile_chunk_steps = [] { const int64_t v = env_int("TFR_CHUNK_STEPS", 256); return v < 1 ? 256 : v; }();
    ready.plan(tiles_eligible(m, B) ? tile_chunk_steps : B >= 65536 ? 1 : (65536 / B < 16 ? 65536 / B : 16), pre);
    if (rng == 0) {                                        // one-rating store: no draw consumed
        HIPCHK(hipMemsetAsync(m->ids.ids, 0, (size_t)total * 8, m->stream3));
        m->ids.n_recs = 0;
    }
    tr.mark(pre ? "ids drawn ahead taken" : "no ids drawn ahead");
    if ((rc = staged_steps(m, 0, B, nsteps, loss_out, &ready))) return rc;
    tr.mark("all steps enqueued");
    if ((rc = ready.enqueue_through(nsteps))) return rc;   // (every chunk is out by now; this is a no-op kept for clarity)
    if (rng != 0 && (rc = ready.run_ahead())) return rc;
    tr.mark("run-ahead draw enqueued");
    return TFR_OK;
}

// which kernels (rocprof's demangled spelling of the template arguments) one training step of this model
// launches at this batch size - so that bench.py can name what it timed and look the same kernels up in
// the committed rocprofv3 summaries
int tfr_kernel_plan(tfr_model* m, int64_t B, char* buf, int64_t buflen) {
    MODEL_ENTER(m);
    if (!buf || buflen < 64 || B < 1) return fail(TFR_ERR_ARG, "kernel_plan: need a buffer of >= 64 bytes and batch >= 1");
    const OptStep k = opt_step(m);
    const int G = m->G, V = m->VEC;
    const int64_t ntiles = (B + CSORT_TILE - 1) / CSORT_TILE;
    char tmp[1024];
    if (tiles_eligible(m, B) && switch_tile_split()) {       // the three launches of run_train_step's !one_launch: k_front sorts tile-locally
        snprintf(tmp, sizeof(tmp), "forward=k_front<%d, %d>;reduce_item=k_seg_reduce<%d, %d, %d, false, true, false>;apply=k_dense_tiles<%d, %d, false, %d>",
                 G, V, G, V, (int)RMODE_SCRATCH, G, V, dense_tiles_nt(ntiles));
    } else if (tiles_eligible(m, B)) {
        snprintf(tmp, sizeof(tmp), "reduce_item=k_tile_step<%d, %d, %d>;apply=k_dense_tiles<%d, %d, false, %d>", G, V,
                 tile_step_epg((int)ntiles, G, V), G, V, dense_tiles_nt(ntiles));
    } else if (fwd_in_reduce(m, B)) {
        const int rm = reduce_mode(k);
        // the sixth argument: the three-round load form (launch_seg_reduce picks it for the two-table step on full-width rows)
        // (a coarser rule than seg_reduce_pick's, kept: bench.py looks kernels up by this string)
        const bool fast = switch_dualq() && switch_fast() && switch_lean() && m->D == G * V;
        // the fifth: LEAN, false on the item side of the Adam step under TFR_LEAN=0 only (seg_reduce_pick)
        const bool lean = fast || !(rm == RMODE_ADAM && !switch_lean());
        snprintf(tmp, sizeof(tmp), "sort=%s x%d passes (the first gathers the batch);reduce_item=k_seg_reduce<%d, %d, %d, true, %s, %s>;"
                 "reduce_user=k_seg_reduce<%d, %d, %d, false, true, %s>;apply=k_apply_rows<%d, %d, %d>",   // K4 rides in the apply launch
                 rsort_wide_taken(B) ? "k_rsortw_hist/k_rsort_scan/k_rsortw_scatter" : "k_rsort_rank/scan/scatter",
                 ((m->bits_u > m->bits_i ? m->bits_u : m->bits_i) + 7) / 8, G, V, rm, lean ? "true" : "false", fast ? "true" : "false", G, V, rm, fast ? "true" : "false", G, V, apply_mode(k));
    } else if (csort_path(m, B)) {
        snprintf(tmp, sizeof(tmp), "forward=k_front<%d, %d>;sort=k_csort_scan/scatter;reduce_item=k_seg_reduce<%d, %d, %d, false, true, false>;apply=%s",
                 G, V, G, V, reduce_mode(k), k.tf1 ? "k_adam_dense" : "k_apply_rows");
    } else {
        snprintf(tmp, sizeof(tmp), "forward=k_forward<%d, %d, 1, 4, false>;sort=k_rsort_rank/scan/scatter;reduce_item=k_seg_reduce<%d, %d, 0, false, true, false>;apply=k_adam_dense<%d, %d>;finalize=k_finalize",
                 G, V, G, V, G, V);
    }
    snprintf(buf, (size_t)buflen, "%s", tmp);
    return TFR_OK;
}

// which forward instantiation a shape launches and on how many blocks, by the functions run_forward launches by.
// Needs no model and no device: tests/test_width_coverage.py and tests/test_forward_paths_host.py read it.
int tfr_forward_plan(int32_t dim, int64_t user_num, int32_t mode, int32_t rows, int64_t batch, char* buf, int64_t buflen) {
    int G, VEC;
    if (!geometry(dim, &G, &VEC)) return fail(TFR_ERR_ARG, "unsupported dim %d", dim);
    if (user_num < 1 || user_num > 0x7fffffffLL || batch < 0) return fail(TFR_ERR_ARG, "forward_plan: need user_num in [1, 2^31) and batch >= 0");
    if (mode != MODE_INFER && mode != MODE_TRAIN && mode != MODE_EVAL) return fail(TFR_ERR_ARG, "forward_plan: mode must be 0 (INFER), 1 (TRAIN) or 2 (EVAL)");
    if (rows != ROWS_F32 && rows != ROWS_BF16) return fail(TFR_ERR_ARG, "forward_plan: rows must be 0 (float32) or 1 (bf16 snapshot)");
    if (rows == ROWS_BF16 && mode == MODE_TRAIN) return fail(TFR_ERR_ARG, "forward_plan: the snapshot has no TRAIN forward");
    const FwdPlan p = forward_plan(dim, G, user_num, mode, (FwdRows)rows, batch);
    char tmp[128];
    int n;
    if (rows == ROWS_F32) n = snprintf(tmp, sizeof(tmp), "k_forward<%d, %d, %d, 4, %s>;grid=%d", p.G, VEC, mode, p.pnt ? "true" : "false", p.grid);
    else n = snprintf(tmp, sizeof(tmp), "k_forward_bf16<%d, %d, %d, %s>;grid=%d", p.G, mode, p.unr, p.pnt ? "true" : "false", p.grid);
    if (!buf || buflen < (int64_t)n + 1) return fail(TFR_ERR_ARG, "forward_plan: need a buffer of >= %d bytes", n + 1);
    memcpy(buf, tmp, (size_t)n + 1);
    return TFR_OK;
}

// static + dynamic LDS bytes per workgroup of the shape-dependent kernels, computed exactly as the launchers do.
// Needs no device (pure host arithmetic): tests/test_lds_budget.py enumerates every selectable combination.
int tfr_lds_bytes(int32_t kernel, int32_t dim, int64_t batch, int64_t user_num, int64_t item_num,
                  int64_t* static_bytes, int64_t* dynamic_bytes) {
    int G, VEC;
    if (!geometry(dim, &G, &VEC)) return fail(TFR_ERR_ARG, "unsupported dim %d", dim);
    if (batch < 1 || user_num < 1 || item_num < 1) return fail(TFR_ERR_ARG, "lds_bytes: batch and row counts must be >= 1");
    const int bu = bits_for(user_num), bi = bits_for(item_num);
    const int nbmax = 1 << (bu > bi ? bu : bi);
    int64_t st = 0, dy = 0;
    if (kernel == 0 || kernel == 2) {                    // k_tile_step / k_front: small tables only
        if (nbmax > CSORT_MAX_BINS || !csort_eligible(batch, bu, bi)) return fail(TFR_ERR_ARG, "shape does not take the counting-sort path");
        const int64_t ntiles = (batch + CSORT_TILE - 1) / CSORT_TILE;
        if (kernel == 0) {
            if (ntiles > 16) return fail(TFR_ERR_ARG, "batch beyond 16 tiles does not take k_tile_step");
            const int epg = tile_step_epg((int)ntiles, G, VEC);
            st = (int64_t)tile_step_static_lds(G, epg);
            dy = (int64_t)tile_step_dyn_lds(G, VEC, epg, nbmax);
        } else {
            st = 256 * 4 + 16 * 64 * 4 + 16 * 3 * 4;     // wtot, the forward's LDS-staged reduce slot, block_sum_store
            dy = (int64_t)nbmax * 4;
        }
    } else if (kernel == 1 || kernel == 4) {             // k_seg_reduce with / without the forward inside
        st = (int64_t)seg_reduce_static_lds(G, VEC, kernel == 1);
    } else if (kernel == 3) {                            // k_mt_draw: two generator blocks + the wave counts
        st = 2 * 624 * 4 + 2 * 10 * 4;
    } else {
        return fail(TFR_ERR_ARG, "lds_bytes: kernel must be 0 (k_tile_step), 1 (k_seg_reduce fwd), 2 (k_front), 3 (k_mt_draw), 4 (k_seg_reduce)");
    }
    if (static_bytes) *static_bytes = st;
    if (dynamic_bytes) *dynamic_bytes = dy;
    return TFR_OK;
}

// what keeps the small-table sweep one shift of workgroups: its step instantiation's resident workgroups per CU and
// scratch bytes per lane as the runtime reports them for the loaded code object, and the grid the shape launches
int tfr_sweep_residency(int32_t dim, int64_t batch, int64_t user_num, int64_t item_num,
                        int32_t* blocks_per_cu, int64_t* scratch_bytes, int64_t* grid_blocks) {
    int G, VEC;
    if (!geometry(dim, &G, &VEC)) return fail(TFR_ERR_ARG, "unsupported dim %d", dim);
    if (batch < 1 || user_num < 1 || item_num < 1) return fail(TFR_ERR_ARG, "sweep_residency: batch and row counts must be >= 1");
    const int bu = bits_for(user_num), bi = bits_for(item_num);
    const int64_t ntiles = (batch + CSORT_TILE - 1) / CSORT_TILE;
    if ((1 << (bu > bi ? bu : bi)) > CSORT_MAX_BINS || !csort_eligible(batch, bu, bi) || ntiles > 16)
        return fail(TFR_ERR_ARG, "shape does not take k_dense_tiles");
    const void* k = dense_tiles_kernel(false, G, VEC, (int)ntiles);
    if (!k) return fail(TFR_ERR_ARG, "no k_dense_tiles instantiation for dim %d", dim);
    int nblk = 0;
    hipFuncAttributes attr;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, k, 256, 0));
    HIPCHK(hipFuncGetAttributes(&attr, k));
    if (blocks_per_cu) *blocks_per_cu = nblk;
    if (scratch_bytes) *scratch_bytes = (int64_t)attr.localSizeBytes;
    if (grid_blocks) *grid_blocks = 2 * ((int64_t)dense_tiles_grid(user_num > item_num ? user_num : item_num, G) + 1);
    return TFR_OK;
}

static int ensure_ring(tfr_model* m, int64_t B) {
    if (B <= m->ring_cap) return TFR_OK;
    const int64_t cap = pow2_cap(B);
    m->ring_cap = 0;
    HIPCHK(m->d_ring.reserve(cap * tfr_model::HRING, m->stream));
    HIPCHK(m->h_ring.reserve(cap * tfr_model::HRING, m->stream));
    for (int z = 0; z < tfr_model::HRING; ++z)
        if (!m->ring_ev[z]) HIPCHK(hipEventCreateWithFlags(&m->ring_ev[z], hipEventDisableTiming));
    m->ring_cap = cap;
    return TFR_OK;
}

int tfr_train_step_ids(tfr_model* m, const int64_t* ids, int64_t B) {
    MODEL_ENTER(m);
    if (!m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples first");
    if (B < 1 || !ids) return fail(TFR_ERR_ARG, "bad batch / null ids");
    int rc;
    if ((rc = ensure_capacity(m, B))) return rc;
    if ((rc = ensure_ring(m, B))) return rc;
    const int z = m->ring_pos;
    m->ring_pos = (z + 1) % tfr_model::HRING;
    HIPCHK(hipEventSynchronize(m->ring_ev[z]));            // the copy that last used this pinned slot has left it
    int64_t* h = m->h_ring + (size_t)z * m->ring_cap;
    int64_t* d = m->d_ring + (size_t)z * m->ring_cap;
    memcpy(h, ids, (size_t)B * 8);
    HIPCHK(hipMemcpyAsync(d, h, (size_t)B * 8, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipEventRecord(m->ring_ev[z], m->stream));
    m->pf_valid = false;
    return run_train_step(m, m->d_u, m->d_i, m->d_r, B, nullptr, nullptr, d, nullptr);
}

int tfr_forward_resident(tfr_model* m, int64_t lo, int64_t hi, float* logits_out) {
    MODEL_ENTER(m);
    if (!m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples first");
    if (lo < 0 || hi < lo || hi > m->N) return fail(TFR_ERR_ARG, "bad store range [%lld,%lld)", (long long)lo, (long long)hi);
    const int64_t B = hi - lo;
    if (B == 0) return TFR_OK;
    int rc;
    if ((rc = ensure_capacity(m, B))) return rc;
    if ((rc = gather_batch(m, nullptr, lo, B))) return rc;      // (forgets the kept batch: d_r and d_logits are rewritten)
    if ((rc = run_forward(m, MODE_INFER, m->d_u, m->d_i, nullptr, B, m->d_logits, nullptr, nullptr))) return rc;
    if (logits_out) {
        HIPCHK(hipMemcpyAsync(logits_out, m->d_logits, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
        return check_device_error(m);
    }
    return TFR_OK;
}

int tfr_sort_segments(tfr_model* m, int32_t side, const int32_t* ids, int64_t B, int32_t* ks_out, int32_t* ps_out) {
    MODEL_ENTER(m);
    if (side != 0 && side != 1) return fail(TFR_ERR_ARG, "side must be 0 (user) or 1 (item)");
    if (B < 0 || (B > 0 && (!ids || !ks_out || !ps_out))) return fail(TFR_ERR_ARG, "bad batch / null pointer");
    if (B == 0) return TFR_OK;
    int rc;
    if ((rc = ensure_capacity(m, B))) return rc;
    HIPCHK(hipMemcpyAsync(m->d_u, ids, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->d_i, ids, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    if ((rc = sort_columns(m, m->d_u, m->d_i, B))) return rc;      // the training step's own sort path
    HIPCHK(hipMemcpyAsync(ks_out, side == 0 ? m->ks_u : m->ks_i, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(ps_out, side == 0 ? m->ps_u : m->ps_i, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

// ---- row-sharded building blocks --------------------------------------------
// The model handle holds this rank's shard: user rows [U_local], item rows [I_local].  User
// rows of a sample are always local (samples are routed to the owner of their user row);
// item rows are fetched from and their gradients returned to their owners through fixed-capacity
// exchange buffers laid out [world][slot_cap] rows of tfr_shard_row_stride() floats: D features, the bias, padding.

// floats per exchanged row: features, bias, the sender's error flag, padding to 16 bytes where rows are read as float4
static int shard_stride(const tfr_model* m) { return m->VEC == 4 ? m->D + 4 : m->D + 2; }

int32_t tfr_shard_row_stride(tfr_model* m) { return m ? shard_stride(m) : 0; }

static int shard_route_core(tfr_model* m, const int32_t* d_user, const int32_t* d_item, const float* d_rate, const int64_t* d_ids,
                            int64_t Bg, int32_t rank, int32_t world, int64_t U_global, int64_t I_global, int32_t sample_cap,
                            int32_t slot_cap, int32_t* d_req, const int4* d_recs = nullptr) {
    if (Bg < 0 || world < 1 || rank < 0 || rank >= world || sample_cap < 1 || slot_cap < 1 || !d_req || U_global < 1 || I_global < 1 ||
        I_global >= 0x7fffffffLL || U_global >= 0x7fffffffLL || (Bg > 0 && !d_ids && !d_recs && (!d_user || !d_item || !d_rate)))
        return fail(TFR_ERR_ARG, "shard_route: bad arguments");
    if ((int64_t)world * slot_cap >= 0x7fffffffLL) return fail(TFR_ERR_ARG, "shard_route: world * slot_cap too large");
    int rc;
    const int64_t need = sample_cap > (int64_t)world * slot_cap ? sample_cap : (int64_t)world * slot_cap;
    if ((rc = ensure_capacity(m, need > Bg ? need : (Bg > 0 ? Bg : 1)))) return rc;
    tfr_model::RouteSet& R = m->rt[m->rt_sel];
    HIPCHK(reserve_each(sample_cap, m->stream, R.mine, R.u, R.it, R.r, R.slot, R.ks_u, R.ps_u, R.ks_i, R.ps_i));
    HIPCHK(R.counts.reserve(world + 4, m->stream));
    R.B = sample_cap; R.slots = world * slot_cap; R.world = world;
    R.sorted_fwd = false; R.sorted_req = nullptr;
    hipStream_t s = m->stream;
    RouteArgs a;
    memset(&a, 0, sizeof(a));
    a.u = d_user; a.it = d_item; a.r = d_rate; a.Bg = Bg; a.U = U_global; a.I = I_global;
    if (d_ids) { a.ids = d_ids; a.store = m->store; a.N = m->N; }
    a.recs = d_recs;
    a.per_u = (U_global + world - 1) / world; a.per_i = (I_global + world - 1) / world; a.u_lo = a.per_u * rank;
    a.rank = rank; a.world = world; a.Bcap = sample_cap; a.cap = slot_cap;
    a.u_pad = (int32_t)m->U; a.i_pad = (int32_t)I_global;
    a.mine = R.mine; a.u_local = R.u; a.it_glob = R.it; a.r_loc = R.r; a.slot = R.slot;
    a.req = d_req; a.counts = R.counts; a.blk = m->lrank_u; a.err = m->d_err;      // lrank_u: [cap] ints of sort scratch
    HIPCHK(hipMemsetAsync(d_req, 0xff, (size_t)world * slot_cap * 4, s));             // every slot unused (-1)
    launch_route_compact(a, s);
    HIPCHK(hipGetLastError());
    {   // the local samples sorted by global item id: distinct ids become adjacent and grouped by owner
        const int32_t* keys[2] = {R.it, nullptr};           // (into the set's own arrays: the step buffers may be in use by a step
        const int bits[2] = {bits_for(I_global + 1), 0};    //  that runs beside this routing)
        int32_t* ks[2] = {R.ks_i, nullptr};
        int32_t* ps[2] = {R.ps_i, nullptr};
        if ((rc = radix_sort_columns(m, 1, keys, bits, ks, ps, sample_cap))) return rc;
    }
    a.ks = R.ks_i; a.ps = R.ps_i;
    launch_route_slots(a, s);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

int tfr_shard_route(tfr_model* m, const int32_t* d_user, const int32_t* d_item, const float* d_rate, int64_t Bg,
                    int32_t rank, int32_t world, int64_t U_global, int64_t I_global, int32_t sample_cap, int32_t slot_cap,
                    int32_t* d_req) {
    MODEL_ENTER(m);
    return shard_route_core(m, d_user, d_item, d_rate, nullptr, Bg, rank, world, U_global, I_global, sample_cap, slot_cap, d_req);
}

int tfr_shard_route_ids(tfr_model* m, const int64_t* d_ids, int64_t Bg, int32_t rank, int32_t world, int64_t U_global,
                        int64_t I_global, int32_t sample_cap, int32_t slot_cap, int32_t* d_req) {
    MODEL_ENTER(m);
    if (!m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples / tfr_set_triples_dev first (global row ids)");
    if (Bg > 0 && !d_ids) return fail(TFR_ERR_ARG, "shard_route_ids: null ids");
    return shard_route_core(m, nullptr, nullptr, nullptr, d_ids, Bg, rank, world, U_global, I_global, sample_cap, slot_cap, d_req);
}

int tfr_shard_bucket_ids(tfr_model* m, const int64_t* d_ids, int64_t B, int32_t world, int64_t U_global, int32_t pair_cap,
                         void* d_send) {
    MODEL_ENTER(m);
    if (!m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples / tfr_set_triples_dev first (global row ids)");
    if (B < 0 || world < 1 || world > 4096 || U_global < 1 || pair_cap < 1 || !d_send || (B > 0 && !d_ids))
        return fail(TFR_ERR_ARG, "shard_bucket_ids: bad arguments");
    int rc;
    const int64_t nblocks = (B + 1023) / 1024 > 0 ? (B + 1023) / 1024 : 1;
    const int64_t need = nblocks * world > B ? nblocks * world : (B > 0 ? B : 1);
    if ((rc = ensure_capacity(m, need))) return rc;
    hipStream_t s = m->stream;
    HIPCHK(hipMemsetAsync(d_send, 0xff, (size_t)world * pair_cap * sizeof(int4), s));      // every slot unused (u = -1)
    BucketArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids; a.store = m->store; a.N = m->N; a.B = B; a.U = U_global; a.per_u = (U_global + world - 1) / world;
    a.world = world; a.cap = pair_cap; a.send = reinterpret_cast<int4*>(d_send); a.blk = m->lrank_u; a.err = m->d_err;
    launch_bucket(a, s);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

int tfr_shard_route_recs(tfr_model* m, const void* d_recs, int64_t n, int32_t rank, int32_t world, int64_t U_global,
                         int64_t I_global, int32_t sample_cap, int32_t slot_cap, int32_t* d_req) {
    MODEL_ENTER(m);
    if (n > 0 && !d_recs) return fail(TFR_ERR_ARG, "shard_route_recs: null records");
    return shard_route_core(m, nullptr, nullptr, nullptr, nullptr, n, rank, world, U_global, I_global, sample_cap, slot_cap, d_req,
                            reinterpret_cast<const int4*>(d_recs));
}

int tfr_shard_routed_devptrs(tfr_model* m, void** mine, void** u_local, void** slot, void** counts) {
    MODEL_ENTER(m);
    const tfr_model::RouteSet& R = m->rt[m->rt_sel];
    if (!R.counts) return fail(TFR_ERR_STATE, "no routed batch: call tfr_shard_route first");
    if (mine) *mine = R.mine;
    if (u_local) *u_local = R.u;
    if (slot) *slot = R.slot;
    if (counts) *counts = R.counts;
    return TFR_OK;
}

int tfr_shard_gather(tfr_model* m, const int32_t* d_req_recv, int64_t n, float* d_rows_out) {
    MODEL_ENTER(m);
    if (n < 0 || (n > 0 && (!d_req_recv || !d_rows_out))) return fail(TFR_ERR_ARG, "shard_gather: bad arguments");
    if (n == 0) return TFR_OK;
    { const int rcq = settle_q(m); if (rcq) return rcq; }
    GatherPackedArgs g;
    g.ids = d_req_recv; g.table = m->w[TFR_Q]; g.bias = m->w[TFR_BI]; g.out = d_rows_out; g.err = m->d_err;
    g.n = n; g.rows = m->I; g.D = m->D; g.stride = shard_stride(m);
    launch_gather_packed(g, m->G, m->VEC, m->stream);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// part: 1 = the item half (sort, forward + item-side reduce into the exchange buffer, local scalars), 2 = the user half (user-side
// reduce + apply; needs nothing the gradient exchange touches, so a caller may run it beside that exchange), 3 = both
static int shard_forward_reduce_part(tfr_model* m, const float* d_item_rows, float* d_logits, float* d_item_grad, float* d_scalars4, int part) {
    tfr_model::RouteSet& R = m->rt[m->rt_sel];
    if (!R.counts) return fail(TFR_ERR_STATE, "no routed batch: call tfr_shard_route first");
    if (!d_item_rows || ((part & 1) && (!d_item_grad || !d_scalars4))) return fail(TFR_ERR_ARG, "shard_forward_reduce: null pointer");
    const int64_t B = R.B, nI = R.slots;
    const int DS = shard_stride(m);
    const int32_t* du = R.u; const int32_t* dslot = R.slot; const float* dr = R.r;
    const int32_t* dB = R.counts;                         // the local batch size, on the device
    int rc;
    forget_kept_batch(m);                                // a training call
    if ((rc = ensure_capacity(m, B > nI ? B : nI))) return rc;
    const OptStep k = opt_step(m);
    hipStream_t s = m->stream;
    int nblk = (int)((B + 1024 / m->G - 1) / (1024 / m->G));
    RedPair pr;
    ApplyPair app;
    if (part & 1) {
        // a peer that had to void this step (capacity overflow, id out of range) said so beside its rows: void it here too, before
        // anything is updated - every rank then skips the same step and reports it at its next sync
        launch_adopt_peer_err(d_item_rows, (int64_t)(nI / R.world) * DS, R.world, m->D, m->d_err, s);
        HIPCHK(hipGetLastError());
        // the reduce writes the features and the bias of the slots in use and nothing else: the rest of the buffer goes to the
        // owners as zeros (they skip slots they were not asked for, but the wire carries no stale or uninitialised rows)
        launch_clear_grad_slots(d_item_grad, R.counts + 2, R.world, (int32_t)(nI / R.world), m->D, DS, s);
        HIPCHK(hipGetLastError());
        // K1 runs inside the item-side reduce, on the rows it has in registers anyway (as in the single-GPU big-table step);
        // a separate k_forward launch cost 68 us of the 464 (world-1 rehearsal)
        if (R.sorted_fwd) {             // tfr_shard_presort made the sorted orders ahead of time
            R.fks_u = R.ks_u; R.fps_u = R.ps_u; R.fks_i = R.ks_i; R.fps_i = R.ps_i;
        } else {
            Prof p(m, TFR_K_SORT);                        // unused sample slots carry keys one past the last row: they sort last
            const int32_t* keys[2] = {du, dslot};
            const int bits[2] = {bits_for(m->U + 1), bits_for(nI + 1)};
            int32_t* ks[2] = {m->ks_u, m->ks_i};
            int32_t* ps[2] = {m->ps_u, m->ps_i};
            if ((rc = radix_sort_columns(m, 2, keys, bits, ks, ps, B))) return rc;
            R.fks_u = m->ks_u; R.fps_u = m->ps_u; R.fks_i = m->ks_i; R.fps_i = m->ps_i;
        }
        RedArgs& ri = pr.a[0];          // item side: own = the fetched rows, indexed by slot
        ri = rating_side(m, TFR_Q, R.fks_i, R.fps_i, du, B);
        ri.dB = dB; set_hyper(ri, k);
        ri.own = d_item_rows; ri.ostride = DS; ri.own_bias = d_item_rows + m->D; ri.obstride = DS;
        // a slot whose samples lie in one block of the sorted order (nearly all) goes straight into the exchange buffer;
        // k_apply_rows then only finishes the slots cut by a block boundary (it emitted every slot before: 102 us)
        ri.dense_rows = d_item_grad; ri.dstride = DS; ri.dense_bias = d_item_grad + m->D; ri.dbstride = DS;
        ri.partner_bias = m->w[TFR_BU]; ri.mu = m->w[TFR_MU]; ri.r = dr; ri.loss = m->o.loss;
        ri.g_out = m->d_g; ri.logits_out = d_logits; ri.partials = m->partials; ri.stage_sum = 1;
        {
            Prof p(m, TFR_K_REDUCE_ITEM);
            launch_seg_reduce(pr, 1, RMODE_SCRATCH, m->G, m->VEC, s, true);
        }
        HIPCHK(hipGetLastError());
        ApplyArgs& ap = app.a[0];       // reduced gradient row (+ bias gradient) of the split slots, in the exchange layout
        ap = apply_split(m, TFR_Q, R.fks_i, B);
        ap.dB = dB; set_hyper(ap, k);
        ap.w = d_item_grad; ap.wstride = DS; ap.bias_w = d_item_grad + m->D; ap.wbstride = DS;
        {
            Prof p(m, TFR_K_APPLY);
            launch_apply_rows(app, 1, APPLY_EMIT_ROWS, m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
        FinArgs f = local_fin(m, d_scalars4);
        f.nblk = nblk;
        {
            Prof p(m, TFR_K_FINALIZE);
            launch_finalize(f, s);
        }
        HIPCHK(hipGetLastError());
    }
    if (part & 2) {
        if (!R.fks_u) return fail(TFR_ERR_STATE, "shard_reduce_users: call tfr_shard_forward_items on this routed batch first");
        RedArgs& ru = pr.a[0];          // user side: rows are local; partner = fetched item rows
        ru = rating_side(m, TFR_P, R.fks_u, R.fps_u, dslot, B);
        ru.dB = dB; set_hyper(ru, k); bind_side(ru, m, TFR_P);
        ru.partner = d_item_rows; ru.pstride = DS;
        ru.map = k.tf1 ? m->map_u : nullptr;
        {
            Prof p(m, TFR_K_REDUCE_USER);
            launch_seg_reduce(pr, 1, reduce_mode(k), m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
        if (!k.tf1) {
            ApplyArgs& ap = app.a[0];
            ap = apply_split(m, TFR_P, R.fks_u, B);
            ap.dB = dB; set_hyper(ap, k); bind_side(ap, m, TFR_P);
            Prof p(m, TFR_K_APPLY);
            launch_apply_rows(app, 1, apply_mode(k), m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
    }
    if (k.tf1 && (part & 2)) {          // dense sweep of the local user rows (every row moves)
        DensePair dp;
        memset(&dp, 0, sizeof(dp));
        dp.a[0] = dense_side(m, k, TFR_P, R.fks_u, B);
        Prof p(m, TFR_K_APPLY);
        launch_adam_dense(dp, 1, m->G, m->VEC, s);
        HIPCHK(hipGetLastError());
    }
    return TFR_OK;
}

int tfr_shard_forward_reduce(tfr_model* m, const float* d_item_rows, float* d_logits, float* d_item_grad, float* d_scalars4) {
    MODEL_ENTER(m);
    return shard_forward_reduce_part(m, d_item_rows, d_logits, d_item_grad, d_scalars4, 3);
}

int tfr_shard_forward_items(tfr_model* m, const float* d_item_rows, float* d_logits, float* d_item_grad, float* d_scalars4) {
    MODEL_ENTER(m);
    return shard_forward_reduce_part(m, d_item_rows, d_logits, d_item_grad, d_scalars4, 1);
}

int tfr_shard_reduce_users(tfr_model* m, const float* d_item_rows) {
    MODEL_ENTER(m);
    return shard_forward_reduce_part(m, d_item_rows, nullptr, nullptr, nullptr, 2);
}

int tfr_shard_apply_items(tfr_model* m, const int32_t* d_req_recv, const float* d_grad_recv, int64_t n) {
    MODEL_ENTER(m);
    if (n < 0 || (n > 0 && (!d_req_recv || !d_grad_recv))) return fail(TFR_ERR_ARG, "shard_apply_items: bad arguments");
    tfr_model::RouteSet& R = m->rt[m->rt_sel];
    if (!R.counts) return fail(TFR_ERR_STATE, "no routed batch: call tfr_shard_route first");
    int rc;
    if ((rc = settle_q(m))) return rc;
    if ((rc = ensure_capacity(m, n > 0 ? n : 1))) return rc;
    const OptStep k = opt_step(m);
    const int DS = shard_stride(m);
    hipStream_t s = m->stream;
    int32_t* d_nvalid = R.counts + R.world + 2;           // requests actually received (unused slots excluded)
    const int32_t* aks = m->ks_i; const int32_t* aps = m->ps_i;
    if (n > 0) {
        if (R.sorted_req == d_req_recv && R.sorted_req_n == n) {       // tfr_shard_presort has sorted these requests already
            aks = R.aks; aps = R.aps;
        } else {
            // unused slots (-1) get the key one past the last row: they sort behind every real request and fall outside the count
            launch_pad_keys(d_req_recv, m->d_i, n, (int32_t)m->I, d_nvalid, s);
            HIPCHK(hipGetLastError());
            Prof p(m, TFR_K_SORT);
            const int32_t* keys[2] = {m->d_i, nullptr};
            const int bits[2] = {bits_for(m->I + 1), 0};
            int32_t* ks[2] = {m->ks_i, nullptr};
            int32_t* ps[2] = {m->ps_i, nullptr};
            if ((rc = radix_sort_columns(m, 1, keys, bits, ks, ps, n))) return rc;
        }
        RedPair pr;
        RedArgs& r = pr.a[0];           // the received gradient rows, reduced by item row
        r = reduce_side(m, TFR_Q, aks, aps, n);
        r.dB = d_nvalid; set_hyper(r, k); bind_side(r, m, TFR_Q);
        r.rows_in = d_grad_recv; r.rstride = DS; r.bias_in = d_grad_recv + m->D; r.rbstride = DS;
        r.map = k.tf1 ? m->map_i : nullptr;
        {
            Prof p(m, TFR_K_REDUCE_ITEM);
            launch_seg_reduce(pr, 1, reduce_mode(k), m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
        if (!k.tf1) {
            ApplyPair app;
            ApplyArgs& ap = app.a[0];
            ap = apply_split(m, TFR_Q, aks, n);
            ap.dB = d_nvalid; set_hyper(ap, k); bind_side(ap, m, TFR_Q);
            Prof p(m, TFR_K_APPLY);
            launch_apply_rows(app, 1, apply_mode(k), m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
    }
    if (k.tf1) {
        DensePair dp;
        memset(&dp, 0, sizeof(dp));
        dp.a[0] = dense_side(m, k, TFR_Q, aks, n);
        Prof p(m, TFR_K_APPLY);
        launch_adam_dense(dp, 1, m->G, m->VEC, s);
        HIPCHK(hipGetLastError());
    }
    return TFR_OK;
}

// which of the two routed-batch sets the shard calls fill (route_*) and consume (forward / reduce / apply): a caller that
// prepares batch s+1 on a side stream while step s runs alternates between them
int tfr_shard_select(tfr_model* m, int32_t which) {
    MODEL_ENTER(m);
    if (which != 0 && which != 1) return fail(TFR_ERR_ARG, "shard_select: 0 or 1");
    m->rt_sel = which;
    return TFR_OK;
}

// the index work of a step, ahead of time (all of it depends on the routed batch and the requests only, not on any table):
// the routed samples sorted by local user row and by request slot, and - with d_req_recv - the requests received as an owner
// padded and sorted by item row.  tfr_shard_forward_items / _reduce_users / _apply_items then skip their own sorts.
int tfr_shard_presort(tfr_model* m, const int32_t* d_req_recv, int64_t n) {
    MODEL_ENTER(m);
    tfr_model::RouteSet& R = m->rt[m->rt_sel];
    if (!R.counts) return fail(TFR_ERR_STATE, "no routed batch: call tfr_shard_route first");
    if (n < 0 || (n > 0 && !d_req_recv)) return fail(TFR_ERR_ARG, "shard_presort: bad arguments");
    int rc;
    const int64_t B = R.B, nI = R.slots;
    if ((rc = ensure_capacity(m, (B > nI ? B : nI) > n ? (B > nI ? B : nI) : n))) return rc;
    {
        const int32_t* keys[2] = {R.u, R.slot};
        const int bits[2] = {bits_for(m->U + 1), bits_for(nI + 1)};
        int32_t* ks[2] = {R.ks_u, R.ks_i};
        int32_t* ps[2] = {R.ps_u, R.ps_i};
        if ((rc = radix_sort_columns(m, 2, keys, bits, ks, ps, B))) return rc;
        R.sorted_fwd = true;
    }
    if (n > 0) {
        HIPCHK(reserve_each(n, m->stream, R.akeys, R.aks, R.aps));
        launch_pad_keys(d_req_recv, R.akeys, n, (int32_t)m->I, R.counts + R.world + 2, m->stream);
        HIPCHK(hipGetLastError());
        const int32_t* keys[2] = {R.akeys, nullptr};
        const int bits[2] = {bits_for(m->I + 1), 0};
        int32_t* ks[2] = {R.aks, nullptr};
        int32_t* ps[2] = {R.aps, nullptr};
        if ((rc = radix_sort_columns(m, 1, keys, bits, ks, ps, n))) return rc;
        R.sorted_req = d_req_recv; R.sorted_req_n = n;
    }
    return TFR_OK;
}

int tfr_shard_finish_step(tfr_model* m, const float* d_scalars4) {
    MODEL_ENTER(m);
    if (!d_scalars4) return fail(TFR_ERR_ARG, "shard_finish_step: null scalars");
    FinArgs f = mu_fin(m, opt_step(m), !((m->frozen >> TFR_MU) & 1), nullptr);
    f.partials = d_scalars4; f.nblk = 1;
    {
        Prof p(m, TFR_K_FINALIZE);
        launch_finalize(f, m->stream);
    }
    HIPCHK(hipGetLastError());
    advance_step(m);
    return TFR_OK;
}

// ---- data-parallel building blocks: replicated tables, one all-reduce per step -----------
// flat gradient buffer layout (floats): [P grads U*D | Q grads I*D | user_bias U | item_bias I |
// loss, reg, sum_g, 0].  It must be all zeros before the first tfr_dp_local_grads (tfr_dp_apply
// leaves it zeroed again, so one cudaMemset at allocation is enough).
int64_t tfr_dp_flat_size(tfr_model* m) {
    if (!m) return 0;
    return m->U * m->D + m->I * m->D + m->U + m->I + 4;
}

int tfr_dp_hint_next(tfr_model* m, const int64_t* d_next_store_ids) {
    MODEL_ENTER(m);
    m->dp_next_ids = d_next_store_ids;
    return TFR_OK;
}

int tfr_dp_local_grads(tfr_model* m, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                       const int64_t* d_store_ids, float* d_flat) {
    MODEL_ENTER(m);
    if (!d_flat || B < 0) return fail(TFR_ERR_ARG, "dp_local_grads: bad arguments");
    if (!d_store_ids && B > 0 && (!du || !di || !dr)) return fail(TFR_ERR_ARG, "dp_local_grads: null batch pointers");
    if (d_store_ids && !m->N) return fail(TFR_ERR_STATE, "no resident triples: call tfr_upload_triples first");
    if (m->o.optimizer == TFR_OPT_ADAM && !tf1_mode(m))
        return fail(TFR_ERR_STATE, "data-parallel steps need dense semantics: Adam tf1 or SGD");
    int rc;
    if ((rc = settle_q(m))) return rc;
    forget_kept_batch(m);
    const int64_t* next_ids = d_store_ids ? m->dp_next_ids : nullptr;     // one-shot hint (tfr_dp_hint_next)
    m->dp_next_ids = nullptr;
    if ((rc = ensure_capacity(m, B > 0 ? B : 1))) return rc;
    float* gP = d_flat;
    float* gQ = gP + m->U * m->D;
    float* gbu = gQ + m->I * m->D;
    float* gbi = gbu + m->U;
    float* tail = gbi + m->I;
    hipStream_t s = m->stream;
    int nblk = 0;
    bool fin_done = false;
    FinArgs f = local_fin(m, tail);    // local {loss, reg, sum g} -> tail of the flat buffer; no mu update yet
    if (B > 0 && tiles_eligible(m, B)) {
        // small tables: k_tile_step (look-ahead sort of the hinted next batch included), then one sweep that
        // writes every touched row's gradient into the flat buffer and reduces the local scalars (K4 without
        // the mu update)
        int par = 0;
        if ((rc = tile_step_launch(m, du, di, dr, B, nullptr, d_store_ids, next_ids, &par, &nblk))) return rc;
        f.nblk = nblk;
        TileDenseLaunch L = tile_dense(m, B, par, f);
        L.a[0].out_rows = gQ; L.a[0].out_bias = gbi;
        L.a[1].out_rows = gP; L.a[1].out_bias = gbu;
        {
            Prof p(m, TFR_K_APPLY);
            launch_dense_tiles(L, true, true, m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
        fin_done = true;
    } else if (B > 0) {
        if ((rc = front_and_sort(m, du, di, dr, B, nullptr, d_store_ids, f, nblk, fin_done))) return rc;
        RedPair pr;                    // whole runs go straight to their row of the flat buffer
        pr.a[0] = rating_side(m, TFR_Q, m->ks_i, m->ps_i, du, B);
        pr.a[0].dense_rows = gQ; pr.a[0].dense_bias = gbi;
        pr.a[1] = rating_side(m, TFR_P, m->ks_u, m->ps_u, di, B);
        pr.a[1].dense_rows = gP; pr.a[1].dense_bias = gbu;
        {
            Prof p(m, TFR_K_REDUCE_ITEM);
            launch_seg_reduce(pr, 2, RMODE_SCRATCH, m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
        ApplyPair app;                 // runs split over several reduce blocks: add their pieces, emit the row
        memset(&app, 0, sizeof(app));
        app.a[0] = apply_split(m, TFR_Q, m->ks_i, B);
        app.a[0].w = gQ; app.a[0].bias_w = gbi;
        app.a[1] = apply_split(m, TFR_P, m->ks_u, B);
        app.a[1].w = gP; app.a[1].bias_w = gbu;
        {
            Prof p(m, TFR_K_APPLY);
            launch_apply_rows(app, 2, APPLY_EMIT_ROWS, m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
    }
    if (!fin_done) {
        f.nblk = nblk;
        Prof p(m, TFR_K_FINALIZE);
        launch_finalize(f, s);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

int tfr_dp_apply(tfr_model* m, float* d_flat) {
    MODEL_ENTER(m);
    if (!d_flat) return fail(TFR_ERR_ARG, "dp_apply: null buffer");
    const OptStep k = opt_step(m);
    if (k.adam && !k.tf1) return fail(TFR_ERR_STATE, "data-parallel steps need dense semantics: Adam tf1 or SGD");
    { const int rcq = settle_q(m); if (rcq) return rcq; }
    float* gP = d_flat;
    float* gQ = gP + m->U * m->D;
    float* gbu = gQ + m->I * m->D;
    float* gbi = gbu + m->U;
    float* tail = gbi + m->I;
    DensePair dp;
    memset(&dp, 0, sizeof(dp));
    dp.a[0] = dense_side(m, k, TFR_P);
    dp.a[0].dense_grad = gP; dp.a[0].dense_gbias = gbu;
    dp.a[1] = dense_side(m, k, TFR_Q);
    dp.a[1].dense_grad = gQ; dp.a[1].dense_gbias = gbi;
    FinArgs f = mu_fin(m, k, !((m->frozen >> TFR_MU) & 1), nullptr);   // bias_global from the all-reduced {loss, reg, sum g}
    f.partials = tail; f.nblk = 1;                                       // rides in the sweep
    f.clear_partials = 1;                                                // scalars consumed: clean for the next step
    {
        Prof p(m, TFR_K_APPLY);
        launch_adam_dense(dp, 2, m->G, m->VEC, m->stream, &f);
    }
    HIPCHK(hipGetLastError());
    advance_step(m);
    return TFR_OK;
}

int tfr_staged_ids_devptr(tfr_model* m, void** ptr, int64_t* n) {
    MODEL_ENTER(m);
    if (ptr) *ptr = m->ids.ids;
    if (n) *n = m->n_ids;
    return TFR_OK;
}

}  // extern "C"

// ---- second-order FM (BASELINE config 5) -------------------------------------
// The handle wraps a regular model: V = its user_features [F,D], W = its user_bias [F],
// mu = its bias_global; so the FM backward reuses the radix sort, the segmented reduce (K3) and
// the fused SGD / lazy-Adam apply unchanged.
struct FmFit;                                           // fm_fit_api.inc.h
struct tfr_fm {
    tfr_model* m = nullptr;
    FmFit* fit = nullptr;                                // the resident row stores and what the steps drawn from them need
    DevBuf<int64_t> d_indptr;
    DevBuf<int32_t> d_indices;
    DevBuf<float> d_data, d_y, d_out, s_rows;
    DevBuf<int4> ent;                                    // per non-zero {row, g x, lam - g x^2, -} of the training step
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

static void fm_fit_release(tfr_fm* f);

static int fm_stage_csr(tfr_fm* f, const int64_t* indptr, const int32_t* indices, const float* data,
                        const float* y, int64_t n_rows, int64_t* nnz_out) {
    tfr_model* m = f->m;
    const int64_t nnz = indptr[n_rows];
    if (nnz < 0 || indptr[0] != 0) return fail(TFR_ERR_ARG, "indptr must start at 0 and be non-decreasing");
    for (int64_t r = 0; r < n_rows; ++r)
        if (indptr[r + 1] < indptr[r]) return fail(TFR_ERR_ARG, "indptr must be non-decreasing");
    if (nnz > 0 && (!indices || !data)) return fail(TFR_ERR_ARG, "null indices/data");
    HIPCHK(f->d_indptr.reserve(n_rows + 1, m->stream));
    HIPCHK(reserve_each(n_rows, m->stream, f->d_out, f->d_y));
    HIPCHK(reserve_each(nnz, m->stream, f->d_indices, f->d_data));
    HIPCHK(hipMemcpyAsync(f->d_indptr, indptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, m->stream));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(f->d_indices, indices, (size_t)nnz * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(f->d_data, data, (size_t)nnz * 4, hipMemcpyHostToDevice, m->stream));
    }
    if (y) HIPCHK(hipMemcpyAsync(f->d_y, y, (size_t)n_rows * 4, hipMemcpyHostToDevice, m->stream));
    *nnz_out = nnz;
    return TFR_OK;
}

// k_fm_forward variant (launch_fm): TFR_FM_VARIANT=<bits> overrides for A/B
static int fm_variant(const tfr_model* m) {
    static const int ov = (int)env_int("TFR_FM_VARIANT", -1);
    if (ov >= 0) return ov;
    return ((size_t)m->U * m->D * 4 >= ((size_t)128 << 20)) ? 2 : 0;      // V beyond half the Infinity Cache: stream it
}

static int fm_bf16_need_snapshot(const tfr_fm* f) { return bf16_need_snapshot(f->m, "tfr_fm_bf16_snapshot"); }

// TFR_FM_BF16_NTV=0|1: A/B override of the non-temporal V rows of k_fm_forward_bf16 (unset: fm_variant's rule on the
// snapshot's bytes).  Read at every launch, so that one process can alternate the two (tools/bench_bf16_fm.py --ntv-ab).
static bool fm_bf16_ntv(const tfr_model* m) {
    if (env_default_off("TFR_FM_BF16_NTV")) return true;
    if (!env_default_on("TFR_FM_BF16_NTV")) return false;
    return (size_t)m->U * bf16_row_stride(m->D) * 2 >= ((size_t)128 << 20);
}

// the same forward on the snapshot's rows (fm_bf16.hip); the caller has tested for the snapshot
static int fm_bf16_forward_core(tfr_fm* f, const int64_t* d_indptr, const int32_t* d_indices, const float* d_data,
                                int64_t n_rows, float* d_out) {
    tfr_model* m = f->m;
    FmBf16Args a;
    memset(&a, 0, sizeof(a));
    a.V = m->bf.p; a.W = m->bf.bu; a.mu = m->bf.mu;
    a.indptr = d_indptr; a.indices = d_indices; a.data = d_data; a.out = d_out; a.err = m->d_err;
    a.n_rows = n_rows; a.F = m->U; a.DP = bf16_row_stride(m->D);
    const int G = bf16_geometry(m->D);
    (void)hipEventRecord(f->ev0, m->stream);
    launch_fm_bf16(a, G, fm_bf16_grid(n_rows, G), fm_bf16_ntv(m), m->stream);
    (void)hipEventRecord(f->ev1, m->stream);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

static int fm_forward_core(tfr_fm* f, const int64_t* d_indptr, const int32_t* d_indices, const float* d_data,
                           int64_t n_rows, float* d_out, FwdRows rows = ROWS_F32) {
    if (rows == ROWS_BF16) return fm_bf16_forward_core(f, d_indptr, d_indices, d_data, n_rows, d_out);
    tfr_model* m = f->m;
    FmArgs a;
    memset(&a, 0, sizeof(a));
    a.V = m->w[TFR_P]; a.W = m->w[TFR_BU]; a.mu = m->w[TFR_MU];
    a.indptr = d_indptr; a.indices = d_indices; a.data = d_data; a.out = d_out; a.err = m->d_err;
    a.n_rows = n_rows; a.F = m->U; a.D = m->D;
    a.variant = fm_variant(m);
    (void)hipEventRecord(f->ev0, m->stream);
    launch_fm(a, false, m->G, m->VEC, fm_grid(n_rows, m->G, false), m->stream);
    (void)hipEventRecord(f->ev1, m->stream);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// one minibatch: forward (+ s, g, per-entry coefficients) -> radix sort of the non-zeros by
// feature id -> segmented reduce with fused SGD / lazy Adam on V and W -> mu
static int fm_train_core(tfr_fm* f, const int64_t* d_indptr, const int32_t* d_indices, const float* d_data,
                         const float* d_y, int64_t n_rows, int64_t nnz, float* d_pred, float* out3) {
    tfr_model* m = f->m;
    const tfr_opts& o = m->o;
    const OptStep k = opt_step(m);
    const bool adam = k.adam;
    if (adam && o.adam_mode != TFR_ADAM_LAZY) return fail(TFR_ERR_STATE, "FM training supports SGD and lazy Adam");
    int rc;
    if ((rc = ensure_capacity(m, nnz > 0 ? nnz : 1))) return rc;
    HIPCHK(f->s_rows.reserve(n_rows * m->D, m->stream));
    HIPCHK(f->ent.reserve(nnz, m->stream));
    hipStream_t s = m->stream;
    FmArgs a;
    memset(&a, 0, sizeof(a));
    a.V = m->w[TFR_P]; a.W = m->w[TFR_BU]; a.mu = m->w[TFR_MU];
    a.indptr = d_indptr; a.indices = d_indices; a.data = d_data; a.out = d_pred; a.err = m->d_err;
    a.y = d_y; a.s_rows = f->s_rows; a.ent = f->ent; a.partials = m->partials;
    a.n_rows = n_rows; a.F = m->U; a.D = m->D; a.loss = o.loss; a.lam = o.reg;
    a.variant = fm_variant(m);
    const int grid = fm_grid(n_rows, m->G, true);
    (void)hipEventRecord(f->ev0, s);
    {
        Prof p(m, TFR_K_FORWARD);
        launch_fm(a, true, m->G, m->VEC, grid, s);
    }
    HIPCHK(hipGetLastError());
    if (nnz > 0) {
        {
            Prof p(m, TFR_K_SORT);
            if ((rc = sort_model_columns(m, d_indices, nullptr, nnz, false))) return rc;
        }
        RedPair pr;
        RedArgs& r = pr.a[0];
        r = reduce_side(m, TFR_P, m->ks_u, m->ps_u, nnz);   // V and W: the wrapped model's user side (its frozen mask stays 0)
        r.reg_bias = 1; r.lam = o.reg;
        set_hyper(r, k); bind_side(r, m, TFR_P);
        r.ent = f->ent; r.partner = f->s_rows;
        {
            Prof p(m, TFR_K_REDUCE_USER);
            launch_seg_reduce(pr, 1, reduce_mode(k), m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
        ApplyPair app;
        ApplyArgs& ap = app.a[0];
        ap = apply_split(m, TFR_P, m->ks_u, nnz);
        set_hyper(ap, k); bind_side(ap, m, TFR_P);
        {
            Prof p(m, TFR_K_APPLY);
            launch_apply_rows(app, 1, apply_mode(k), m->G, m->VEC, s);
        }
        HIPCHK(hipGetLastError());
    }
    FinArgs fin = mu_fin(m, k, true, out3);
    fin.partials = m->partials; fin.nblk = grid;
    {
        Prof p(m, TFR_K_FINALIZE);
        launch_finalize(fin, s);
    }
    (void)hipEventRecord(f->ev1, s);
    HIPCHK(hipGetLastError());
    advance_step(m);
    return TFR_OK;
}

extern "C" {

const char* tfr_fm_last_error(void) { return g_err; }

int tfr_fm_destroy(tfr_fm* f) {
    if (!f) return TFR_OK;
    tfr_model* m = f->m;
    if (m) {
        (void)hipSetDevice(m->device);
        (void)hipStreamSynchronize(m->stream);
    }
    if (f->ev0) (void)hipEventDestroy(f->ev0);
    if (f->ev1) (void)hipEventDestroy(f->ev1);
    fm_fit_release(f);
    delete f;                                            // the FM buffers go first, under the wrapped model's device
    return tfr_destroy(m);
}

int tfr_fm_create(tfr_fm** out, int64_t n_features, int32_t dim, const tfr_opts* opts) {
    if (!out) return fail(TFR_ERR_ARG, "out is null");
    *out = nullptr;
    tfr_opts o;
    if (opts) o = *opts;
    else {
        tfr_default_opts(&o);
        o.loss = TFR_LOSS_NLL;          // fm.py:104 task = 'classification'
        o.optimizer = TFR_OPT_SGD;
        o.lr = 0.01f; o.reg = 0.0f;
    }
    if (o.optimizer == TFR_OPT_ADAM) o.adam_mode = TFR_ADAM_LAZY;
    tfr_fm* f = new (std::nothrow) tfr_fm();
    if (!f) return fail(TFR_ERR_NOMEM, "host allocation failed");
    int rc = tfr_create(&f->m, n_features, 1, dim, &o);
    if (rc == TFR_OK && (hipEventCreate(&f->ev0) != hipSuccess || hipEventCreate(&f->ev1) != hipSuccess))
        rc = fail(TFR_ERR_HIP, "event creation failed");
    if (rc) {
        char keep[512];
        strncpy(keep, g_err, sizeof(keep));
        tfr_fm_destroy(f);
        strncpy(g_err, keep, sizeof(g_err));
        return rc;
    }
    *out = f;
    return TFR_OK;
}

int tfr_fm_set(tfr_fm* f, float mu, const float* W, const float* V) {
    if (!f || !W || !V) return fail(TFR_ERR_ARG, "null argument");
    int rc = tfr_set_table(f->m, TFR_MU, &mu, 1);
    if (!rc) rc = tfr_set_table(f->m, TFR_BU, W, f->m->U);
    if (!rc) rc = tfr_set_table(f->m, TFR_P, V, f->m->U * f->m->D);
    return rc;
}

int tfr_fm_get(tfr_fm* f, float* mu, float* W, float* V) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    int rc = TFR_OK;
    if (mu) rc = tfr_get_table(f->m, TFR_MU, mu, 1);
    if (!rc && W) rc = tfr_get_table(f->m, TFR_BU, W, f->m->U);
    if (!rc && V) rc = tfr_get_table(f->m, TFR_P, V, f->m->U * f->m->D);
    return rc;
}

// V, W, mu and their Adam slots are the wrapped model's user side; its item side is a one-row stub and not part of the FM model
int tfr_fm_get_table(tfr_fm* f, int32_t which, float* host, int64_t n) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    const int t = which & 7;
    if (t != TFR_MU && t != TFR_BU && t != TFR_P) return fail(TFR_ERR_ARG, "bad FM table id %d (TFR_MU, TFR_BU = W, TFR_P = V)", which);
    return tfr_get_table(f->m, which, host, n);
}

int tfr_fm_get_step(tfr_fm* f, int64_t* step, float* b1p, float* b2p) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    return tfr_get_step(f->m, step, b1p, b2p);
}

int tfr_fm_init(tfr_fm* f, uint64_t seed, float stddev) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    m->tab_gen += 1;
    launch_init_trunc_normal(m->w[TFR_P], m->n[TFR_P], stddev, seed * 2 + 0, m->stream);
    launch_init_trunc_normal(m->w[TFR_BU], m->n[TFR_BU], stddev, seed * 2 + 1, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(m->w[TFR_MU], 0, 4, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

}  // extern "C"

// the bodies of tfr_fm_forward_dev / tfr_fm_forward and of their snapshot twins, which differ in `rows` and in the snapshot
// test (which comes before n_rows == 0, as in the tfr_bf16_* entries)
static int fm_forward_dev(tfr_fm* f, FwdRows rows, const int64_t* d_indptr, const int32_t* d_indices, const float* d_data,
                          int64_t n_rows, float* d_out) {
    if (!f || n_rows < 0 || (n_rows > 0 && (!d_indptr || !d_out))) return fail(TFR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(f->m->device));
    int rc;
    if (rows == ROWS_BF16 && (rc = fm_bf16_need_snapshot(f))) return rc;
    if (n_rows == 0) return TFR_OK;
    if ((rc = ensure_capacity(f->m, 1))) return rc;
    return fm_forward_core(f, d_indptr, d_indices, d_data, n_rows, d_out, rows);
}

static int fm_forward_host(tfr_fm* f, FwdRows rows, const int64_t* indptr, const int32_t* indices, const float* data,
                           int64_t n_rows, float* out) {
    if (!f || n_rows < 0 || (n_rows > 0 && (!indptr || !out))) return fail(TFR_ERR_ARG, "bad arguments");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    int rc;
    if (rows == ROWS_BF16 && (rc = fm_bf16_need_snapshot(f))) return rc;
    if (n_rows == 0) return TFR_OK;
    int64_t nnz = 0;
    if ((rc = fm_stage_csr(f, indptr, indices, data, nullptr, n_rows, &nnz))) return rc;
    if ((rc = fm_forward_core(f, f->d_indptr, f->d_indices, f->d_data, n_rows, f->d_out, rows))) return rc;
    HIPCHK(hipMemcpyAsync(out, f->d_out, (size_t)n_rows * 4, hipMemcpyDeviceToHost, m->stream));
    return check_device_error(m);
}

extern "C" {

int tfr_fm_forward_dev(tfr_fm* f, const int64_t* d_indptr, const int32_t* d_indices, const float* d_data,
                       int64_t n_rows, float* d_out) {
    return fm_forward_dev(f, ROWS_F32, d_indptr, d_indices, d_data, n_rows, d_out);
}

int tfr_fm_forward(tfr_fm* f, const int64_t* indptr, const int32_t* indices, const float* data,
                   int64_t n_rows, float* out) {
    return fm_forward_host(f, ROWS_F32, indptr, indices, data, n_rows, out);
}

// ---- the FM on the bf16 snapshot (fm_bf16.h): V = the wrapped model's P, W = its bu, so the snapshot is the wrapped model's
int tfr_fm_bf16_snapshot(tfr_fm* f) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    return tfr_bf16_snapshot(f->m);
}

int tfr_fm_bf16_drop(tfr_fm* f) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    return tfr_bf16_drop(f->m);
}

int tfr_fm_bf16_get_rows(tfr_fm* f, uint16_t* host, int64_t n) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    HIPCHK(hipSetDevice(f->m->device));
    if (int rc = fm_bf16_need_snapshot(f)) return rc;
    return tfr_bf16_get_rows(f->m, TFR_P, host, n);
}

int tfr_fm_bf16_forward_dev(tfr_fm* f, const int64_t* d_indptr, const int32_t* d_indices, const float* d_data,
                            int64_t n_rows, float* d_out) {
    return fm_forward_dev(f, ROWS_BF16, d_indptr, d_indices, d_data, n_rows, d_out);
}

int tfr_fm_bf16_forward(tfr_fm* f, const int64_t* indptr, const int32_t* indices, const float* data,
                        int64_t n_rows, float* out) {
    return fm_forward_host(f, ROWS_BF16, indptr, indices, data, n_rows, out);
}

int tfr_fm_train_step_dev(tfr_fm* f, const int64_t* d_indptr, const int32_t* d_indices, const float* d_data,
                          const float* d_y, int64_t n_rows, int64_t nnz, float* d_pred) {
    if (!f || n_rows < 1 || nnz < 0 || !d_indptr || !d_y) return fail(TFR_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(f->m->device));
    return fm_train_core(f, d_indptr, d_indices, d_data, d_y, n_rows, nnz, d_pred, nullptr);
}

int tfr_fm_train_step(tfr_fm* f, const int64_t* indptr, const int32_t* indices, const float* data, const float* y,
                      int64_t n_rows, float* pred_out, float* loss_out) {
    if (!f || n_rows < 1 || !indptr || !y) return fail(TFR_ERR_ARG, "bad arguments");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    int64_t nnz = 0;
    int rc = fm_stage_csr(f, indptr, indices, data, y, n_rows, &nnz);
    if (rc) return rc;
    const StepMark mark = mark_step(m);
    if ((rc = fm_train_core(f, f->d_indptr, f->d_indices, f->d_data, f->d_y, n_rows, nnz, f->d_out, nullptr))) return rc;
    float sc[4] = {0.f, 0.f, 0.f, 0.f};
    if (pred_out) HIPCHK(hipMemcpyAsync(pred_out, f->d_out, (size_t)n_rows * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(sc, m->scalars, 16, hipMemcpyDeviceToHost, m->stream));
    if ((rc = check_device_error(m))) {
        rollback_step(m, mark);
        return rc;
    }
    if (loss_out) *loss_out = sc[0];
    return TFR_OK;
}

int tfr_fm_sync(tfr_fm* f, float* last_kernel_ms) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    HIPCHK(hipSetDevice(f->m->device));
    int rc = check_device_error(f->m);
    if (rc) return rc;
    if (last_kernel_ms) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, f->ev0, f->ev1) != hipSuccess) {   // no timed launch yet (a snapshot is none)
            ms = 0.f;
            (void)hipGetLastError();                     // or the next launch's check would report this one
        }
        *last_kernel_ms = ms;
    }
    return TFR_OK;
}

}  // extern "C"

// ---- the tables top-K (topk.hip) and held-out ranking (rank.hip) score, and the host checks they share with neighbours ----
struct TopkTables { const float *P, *bu, *Q, *bi, *mu; int64_t U, n_items; int32_t item_abs; };

static TopkTables svd_topk_tables(const tfr_model* m) {
    return {m->w[TFR_P], m->w[TFR_BU], m->w[TFR_Q], m->w[TFR_BI], m->w[TFR_MU], m->U, m->I, m->o.item_abs};
}

// FM: V / W of the wrapped model are the users' and the items' features, mu its bias_global; items are features
// [item_lo, item_hi).  `who` prefixes the error.
static int fm_topk_tables(const tfr_model* m, const char* who, int64_t item_lo, int64_t item_hi, TopkTables* t) {
    if (item_lo < 0 || item_hi <= item_lo || item_hi > m->U)
        return fail(TFR_ERR_ARG, "%s: item feature range [%lld, %lld) not inside [0, %lld)", who, (long long)item_lo,
                    (long long)item_hi, (long long)m->U);
    *t = {m->w[TFR_P], m->w[TFR_BU], m->w[TFR_P] + item_lo * m->D, m->w[TFR_BU] + item_lo, m->w[TFR_MU], m->U, item_hi - item_lo, 0};
    return TFR_OK;
}

// host ids: every ids[0..n) inside [0, rows)
static int check_ids(const char* who, const char* what, const int32_t* ids, int64_t n, int64_t rows) {
    for (int64_t r = 0; r < n; ++r)
        if (ids[r] < 0 || (int64_t)ids[r] >= rows)
            return fail(TFR_ERR_OOB, "%s: %s %d outside [0, %lld)", who, what, ids[r], (long long)rows);
    return TFR_OK;
}

// a host CSR of n item rows, targets (each row strictly increasing) or exclusions (each row sorted): indptr non-decreasing from
// >= 0, checked whole before any item is read, and items inside [0, n_items)
static int check_csr(const char* who, bool targets, const int64_t* ip, const int32_t* it, int64_t n, int64_t n_items) {
    const char* what = targets ? "target" : "exclusion";
    if (ip[0] < 0) return fail(TFR_ERR_ARG, "%s: %s indptr starts below 0", who, what);
    for (int64_t r = 0; r < n; ++r)
        if (ip[r + 1] < ip[r]) return fail(TFR_ERR_ARG, "%s: %s indptr decreases at row %lld", who, what, (long long)r);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t e = ip[r]; e < ip[r + 1]; ++e) {
            if (it[e] < 0 || (int64_t)it[e] >= n_items)
                return fail(TFR_ERR_OOB, "%s: %s item %d outside [0, %lld)", who, targets ? "target" : "excluded", it[e],
                            (long long)n_items);
            if (e > ip[r] && (targets ? it[e - 1] >= it[e] : it[e - 1] > it[e]))
                return fail(TFR_ERR_ARG, "%s: %s row %lld is not %s", who, what, (long long)r,
                            targets ? "strictly increasing" : "sorted");
        }
    return TFR_OK;
}

// ---- the best k rows by a tile score: the driver of top-K (topk.hip) and nearest neighbours (neighbours.hip) ----------------
// What a family tells the driver: its name in errors, the bound of the exclusion ids, the candidate count, whether item rows
// the fused big-table step left in q_alt must come back first.  A query derives from it and adds
// score(common, plan, stream): fill the family's own argument fields and launch its score kernel for one chunk.
struct SlicedQuery { const char* who; int64_t excl_rows, n_cand; int32_t item_abs; bool settle; };

static int check_k(const char* who, int32_t k) {
    return k < 1 || k > TOPK_KMAX ? fail(TFR_ERR_ARG, "%s: k must be in [1, %d] (got %d)", who, TOPK_KMAX, k) : TFR_OK;
}

// the body of tfr_topk_plan and tfr_neighbours_plan; `counts` words the family's range error
static int sliced_plan_entry(const char* who, const char* counts, int32_t dim, int32_t k, int64_t n, int64_t n_cand,
                             int64_t* lds_bytes, int32_t* rows_per_block, int32_t* slices, int64_t* row_chunk) {
    int G, VEC;
    if (!geometry(dim, &G, &VEC)) return fail(TFR_ERR_ARG, "unsupported dim %d", dim);
    if (n < 0 || n_cand < 1) return fail(TFR_ERR_ARG, "%s plan: %s", who, counts);
    if (int rc = check_k(who, k)) return rc;
    TopkPlan p;
    topk_plan(k, n, n_cand, &p);                         // cannot refuse: its conditions are the two above
    if (lds_bytes) *lds_bytes = (int64_t)(p.lds_score > p.lds_merge ? p.lds_score : p.lds_merge);
    if (rows_per_block) *rows_per_block = p.upb;
    if (slices) *slices = p.slices;
    if (row_chunk) *row_chunk = p.chunk;
    return TFR_OK;
}

// what every run starts with, after the family's argument checks: the plan and the reset of the bad-exclusions flag
template <class Query>
static int sliced_begin(tfr_model* m, const Query& q, int32_t k, int64_t n, TopkPlan* p) {
    if (!topk_plan(k, n, q.n_cand, p)) return fail(TFR_ERR_ARG, "%s: no plan for k %d", q.who, k);
    HIPCHK(m->tk_bad.reserve(1, m->stream));
    HIPCHK(hipMemsetAsync(m->tk_bad, 0, sizeof(int32_t), m->stream));
    return q.settle ? settle_q(m) : TFR_OK;
}

// one chunk of rows, all pointers on the device: scoring (candidate slices) -> merge into d_out / d_scores
template <class Query>
static int sliced_chunk(tfr_model* m, const Query& q, const TopkPlan& p, const int32_t* d_ids, int64_t rows, int32_t k,
                        const int64_t* d_indptr, const int32_t* d_excl, int32_t* d_out, float* d_scores) {
    HIPCHK(m->tk_part.reserve(pow2_cap(rows * p.slices * k), m->stream));
    SlicedArgs c = {};
    c.rows = d_ids; c.indptr = d_indptr; c.excl = d_excl; c.excl_bad = m->tk_bad;
    c.part = m->tk_part; c.err = m->d_err;
    c.n_rows = rows; c.D = m->D; c.k = k; c.slices = p.slices; c.item_abs = q.item_abs;
    q.score(c, p, m->stream);
    HIPCHK(hipGetLastError());
    TopkMergeArgs g;
    memset(&g, 0, sizeof(g));
    g.part = m->tk_part; g.items_out = d_out; g.scores_out = d_scores; g.n_rows = rows; g.k = k; g.slices = p.slices;
    launch_topk_merge(g, m->stream);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// the host entries, their ids and exclusion CSR checked by the family before any device work: chunk by chunk staged, scored,
// merged and copied back.  Outputs are written only when every check passed.
template <class Query>
static int sliced_host(tfr_model* m, const Query& q, const int32_t* ids, int64_t n, int32_t k, const int64_t* indptr,
                       const int32_t* excl, int32_t* ids_out, float* scores_out) {
    TopkPlan p;
    int rc = sliced_begin(m, q, k, n, &p);
    if (rc) return rc;
    HIPCHK(m->tk_users.reserve(pow2_cap(p.chunk), m->stream));
    HIPCHK(m->tk_items.reserve(pow2_cap(p.chunk * k), m->stream));
    if (scores_out) HIPCHK(m->tk_scores.reserve(pow2_cap(p.chunk * k), m->stream));
    std::vector<int64_t> rebased;
    for (int64_t c0 = 0; c0 < n; c0 += p.chunk) {
        const int64_t rows = n - c0 < p.chunk ? n - c0 : p.chunk;
        HIPCHK(hipMemcpyAsync(m->tk_users, ids + c0, (size_t)rows * 4, hipMemcpyHostToDevice, m->stream));
        const int64_t* d_ip = nullptr;
        const int32_t* d_ex = nullptr;
        if (indptr) {
            const int64_t e0 = indptr[c0], nnz = indptr[c0 + rows] - e0;
            rebased.resize((size_t)rows + 1);
            for (int64_t r = 0; r <= rows; ++r) rebased[(size_t)r] = indptr[c0 + r] - e0;
            HIPCHK(m->tk_indptr.reserve(pow2_cap(rows + 1), m->stream));
            if (nnz > 0) HIPCHK(m->tk_excl.reserve(pow2_cap(nnz), m->stream));
            HIPCHK(hipMemcpyAsync(m->tk_indptr, rebased.data(), (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, m->stream));
            if (nnz > 0) HIPCHK(hipMemcpyAsync(m->tk_excl, excl + e0, (size_t)nnz * 4, hipMemcpyHostToDevice, m->stream));
            d_ip = m->tk_indptr;
            d_ex = m->tk_excl;
        }
        if ((rc = sliced_chunk(m, q, p, m->tk_users, rows, k, d_ip, d_ex, m->tk_items, scores_out ? m->tk_scores : nullptr)))
            return rc;
        HIPCHK(hipMemcpyAsync(ids_out + c0 * k, m->tk_items, (size_t)rows * k * 4, hipMemcpyDeviceToHost, m->stream));
        if (scores_out)
            HIPCHK(hipMemcpyAsync(scores_out + c0 * k, m->tk_scores, (size_t)rows * k * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));         // the staged inputs are rewritten by the next chunk
    }
    return check_device_error(m);
}

// the device entries: every pointer on the device, the exclusion CSR checked there; no synchronisation
template <class Query>
static int sliced_dev(tfr_model* m, const Query& q, const int32_t* d_ids, int64_t n, int32_t k, const int64_t* d_indptr,
                      const int32_t* d_excl, int32_t* d_ids_out, float* d_scores_out) {
    TopkPlan p;
    int rc = sliced_begin(m, q, k, n, &p);
    if (rc) return rc;
    if (d_indptr) {
        launch_topk_check_excl(d_indptr, d_excl, n, q.excl_rows, m->tk_bad, m->d_err, m->stream);
        HIPCHK(hipGetLastError());
    }
    for (int64_t c0 = 0; c0 < n; c0 += p.chunk) {
        const int64_t rows = n - c0 < p.chunk ? n - c0 : p.chunk;
        if ((rc = sliced_chunk(m, q, p, d_ids + c0, rows, k, d_indptr ? d_indptr + c0 : nullptr, d_excl, d_ids_out + c0 * k,
                               d_scores_out ? d_scores_out + c0 * k : nullptr)))
            return rc;
    }
    return TFR_OK;
}

// ---- top-K recommendation: its queries (float32 tables, bf16 snapshot), their argument checks and the entries --------------
struct TopkQuery : SlicedQuery {
    TopkTables t;
    explicit TopkQuery(const TopkTables& t_) : SlicedQuery{"top-K", t_.n_items, t_.n_items, t_.item_abs, true}, t(t_) {}
    int64_t users() const { return t.U; }
    void score(const SlicedArgs& c, const TopkPlan& p, hipStream_t s) const {
        TopkArgs a = {};
        static_cast<SlicedArgs&>(a) = c;
        a.P = t.P; a.bu = t.bu; a.Q = t.Q; a.bi = t.bi; a.mu = t.mu;
        a.U = t.U; a.n_items = t.n_items;
        launch_topk_score(a, p, s);
    }
};

// the same query on the model's bf16 snapshot, which was settled when it was made and is all the kernel reads
struct Bf16TopkQuery : SlicedQuery {
    tfr_model* m;
    explicit Bf16TopkQuery(tfr_model* m_) : SlicedQuery{"bf16 top-K", m_->I, m_->I, m_->o.item_abs, false}, m(m_) {}
    int64_t users() const { return m->U; }
    void score(const SlicedArgs& c, const TopkPlan& p, hipStream_t s) const {
        Bf16TopkArgs a = {};
        static_cast<SlicedArgs&>(a) = c;
        a.P = m->bf.p; a.bu = m->bf.bu; a.Q = m->bf.q; a.bi = m->bf.bi; a.mu = m->bf.mu;
        a.U = m->U; a.n_items = m->I; a.DP = bf16_row_stride(m->D);
        launch_bf16_topk_score(a, p, s);
    }
};

template <class Query>
static int topk_host(tfr_model* m, const Query& q, const int32_t* users, int64_t n, int32_t k, const int64_t* indptr,
                     const int32_t* excl, int32_t* items_out, float* scores_out) {
    if (n < 0) return fail(TFR_ERR_ARG, "%s: negative n_users", q.who);
    int rc = check_k(q.who, k);
    if (rc || n == 0) return rc;
    if (!users || !items_out) return fail(TFR_ERR_ARG, "%s: null users / items_out", q.who);
    if (indptr && !excl && indptr[n] > indptr[0]) return fail(TFR_ERR_ARG, "%s: exclusion indptr without items", q.who);
    if ((rc = check_ids(q.who, "user id", users, n, q.users()))) return rc;
    if (indptr && (rc = check_csr(q.who, false, indptr, excl, n, q.n_cand))) return rc;
    return sliced_host(m, q, users, n, k, indptr, excl, items_out, scores_out);
}

template <class Query>
static int topk_dev(tfr_model* m, const Query& q, const int32_t* d_users, int64_t n, int32_t k,
                    const int64_t* d_excl_indptr, const int32_t* d_excl_items, int32_t* d_items_out, float* d_scores_out) {
    if (n < 0) return fail(TFR_ERR_ARG, "%s: negative n_users", q.who);
    const int rc = check_k(q.who, k);
    if (rc || n == 0) return rc;
    if (!d_users || !d_items_out) return fail(TFR_ERR_ARG, "%s: null users / items_out", q.who);
    if (d_excl_indptr && !d_excl_items) return fail(TFR_ERR_ARG, "%s: exclusion indptr without items", q.who);
    return sliced_dev(m, q, d_users, n, k, d_excl_indptr, d_excl_items, d_items_out, d_scores_out);
}

// the float32 tables' entries (SVD, FM, SVD++) name their tables
static int topk_host(tfr_model* m, const TopkTables& t, const int32_t* users, int64_t n, int32_t k, const int64_t* indptr,
                     const int32_t* excl, int32_t* items_out, float* scores_out) {
    return topk_host(m, TopkQuery(t), users, n, k, indptr, excl, items_out, scores_out);
}

static int topk_dev(tfr_model* m, const TopkTables& t, const int32_t* d_users, int64_t n, int32_t k,
                    const int64_t* d_excl_indptr, const int32_t* d_excl_items, int32_t* d_items_out, float* d_scores_out) {
    return topk_dev(m, TopkQuery(t), d_users, n, k, d_excl_indptr, d_excl_items, d_items_out, d_scores_out);
}

extern "C" {

int tfr_topk_plan(int32_t dim, int32_t k, int64_t n_users, int64_t item_num, int64_t* lds_bytes, int32_t* users_per_block,
                  int32_t* item_slices, int64_t* user_chunk) {
    return sliced_plan_entry("top-K", "n_users >= 0 and item_num >= 1", dim, k, n_users, item_num, lds_bytes, users_per_block,
                             item_slices, user_chunk);
}

int tfr_topk(tfr_model* m, const int32_t* users, int64_t n_users, int32_t k, const int64_t* excl_indptr,
             const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    MODEL_ENTER(m);
    return topk_host(m, svd_topk_tables(m), users, n_users, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_topk_dev(tfr_model* m, const int32_t* d_users, int64_t n, int32_t k, const int64_t* d_excl_indptr,
                 const int32_t* d_excl_items, int32_t* d_items_out, float* d_scores_out) {
    MODEL_ENTER(m);
    return topk_dev(m, svd_topk_tables(m), d_users, n, k, d_excl_indptr, d_excl_items, d_items_out, d_scores_out);
}

// the snapshot test comes before every other check, n_users == 0 included, as in the other tfr_bf16_* entries
int tfr_bf16_topk(tfr_model* m, const int32_t* users, int64_t n_users, int32_t k, const int64_t* excl_indptr,
                  const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    MODEL_ENTER(m);
    if (int rc = bf16_need_snapshot(m)) return rc;
    return topk_host(m, Bf16TopkQuery(m), users, n_users, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_bf16_topk_dev(tfr_model* m, const int32_t* d_users, int64_t n, int32_t k, const int64_t* d_excl_indptr,
                      const int32_t* d_excl_items, int32_t* d_items_out, float* d_scores_out) {
    MODEL_ENTER(m);
    if (int rc = bf16_need_snapshot(m)) return rc;
    return topk_dev(m, Bf16TopkQuery(m), d_users, n, k, d_excl_indptr, d_excl_items, d_items_out, d_scores_out);
}

int tfr_fm_topk(tfr_fm* f, const int32_t* user_features, int64_t n_users, int64_t item_lo, int64_t item_hi, int32_t k,
                const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    TopkTables t;
    int rc = check_k("top-K", k);
    if (rc || (rc = fm_topk_tables(m, "top-K", item_lo, item_hi, &t))) return rc;
    return topk_host(m, t, user_features, n_users, k, excl_indptr, excl_items, items_out, scores_out);
}

}  // extern "C"

// fm_topk_tables taken from the wrapped model's snapshot: users are all features, items the features [item_lo, item_hi)
struct FmBf16TopkQuery : SlicedQuery {
    tfr_model* m;
    int64_t item_lo;
    FmBf16TopkQuery(tfr_model* m_, int64_t lo, int64_t n_items)
        : SlicedQuery{"bf16 top-K", n_items, n_items, 0, false}, m(m_), item_lo(lo) {}
    int64_t users() const { return m->U; }
    void score(const SlicedArgs& c, const TopkPlan& p, hipStream_t s) const {
        Bf16TopkArgs a = {};
        static_cast<SlicedArgs&>(a) = c;
        const int DP = bf16_row_stride(m->D);
        a.P = m->bf.p; a.bu = m->bf.bu; a.Q = m->bf.p + item_lo * DP; a.bi = m->bf.bu + item_lo; a.mu = m->bf.mu;
        a.U = m->U; a.n_items = n_cand; a.DP = DP;
        launch_bf16_topk_score(a, p, s);
    }
};

extern "C" {

// the snapshot test comes before every other check, n_users == 0 included, as in tfr_bf16_topk
int tfr_fm_bf16_topk(tfr_fm* f, const int32_t* user_features, int64_t n_users, int64_t item_lo, int64_t item_hi, int32_t k,
                     const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    int rc = fm_bf16_need_snapshot(f);
    if (rc) return rc;
    TopkTables t;                                        // for its range check and item count; the float32 pointers are not used
    if ((rc = check_k("bf16 top-K", k)) || (rc = fm_topk_tables(m, "bf16 top-K", item_lo, item_hi, &t))) return rc;
    return topk_host(m, FmBf16TopkQuery(m, item_lo, t.n_items), user_features, n_users, k, excl_indptr, excl_items, items_out,
                     scores_out);
}

}  // extern "C"

// ---- held-out ranking (rank.hip, bf16_rank.hip) -----------------------------------------------------------------------------
// Which tables a ranking reads and which launcher scores them: what rank_host is generic over, as the sliced driver is over
// its queries.  who: the name in errors; U / n_items: the id bounds; settle: item rows the fused big-table step left in q_alt
// must come back first.  A query derives from it and adds launch(common, plan, stream): fill the family's own argument
// fields and launch one chunk's kernels.
struct RankFamily { const char* who; int64_t U, n_items; int32_t item_abs; bool settle; };

struct RankQuery : RankFamily {
    TopkTables t;
    explicit RankQuery(const TopkTables& t_) : RankFamily{"rank", t_.U, t_.n_items, t_.item_abs, true}, t(t_) {}
    void launch(const RankCommon& c, const RankPlan& p, hipStream_t s) const {
        RankArgs a = {};
        static_cast<RankCommon&>(a) = c;
        a.P = t.P; a.bu = t.bu; a.Q = t.Q; a.bi = t.bi; a.mu = t.mu;
        launch_rank(a, p, s);
    }
};

// the same on the model's bf16 snapshot, which was settled when it was made and is all the kernels read
struct Bf16RankQuery : RankFamily {
    tfr_model* m;
    explicit Bf16RankQuery(tfr_model* m_) : RankFamily{"bf16 rank", m_->U, m_->I, m_->o.item_abs, false}, m(m_) {}
    void launch(const RankCommon& c, const RankPlan& p, hipStream_t s) const {
        Bf16RankArgs a = {};
        static_cast<RankCommon&>(a) = c;
        a.P = m->bf.p; a.bu = m->bf.bu; a.Q = m->bf.q; a.bi = m->bf.bi; a.mu = m->bf.mu;
        a.DP = bf16_row_stride(m->D);
        launch_bf16_rank(a, p, s);
    }
};

// the host entries: ids, the target rows and the exclusion CSR are checked here, before any device work; the rows are cut
// into pieces of at most RANK_CAP targets and ranked chunk by chunk of pieces.  ranks_out is written only when every check
// passed.
template <class Query>
static int rank_host(tfr_model* m, const Query& t, const int32_t* users, int64_t n, const int64_t* tip,
                     const int32_t* tit, const int64_t* xip, const int32_t* xit, int32_t* ranks_out) {
    if (n < 0) return fail(TFR_ERR_ARG, "%s: negative n_users", t.who);
    if (n == 0) return TFR_OK;
    if (!users || !tip) return fail(TFR_ERR_ARG, "%s: null users / target indptr", t.who);
    const int64_t n_tgt = tip[n] - tip[0];
    if (n_tgt > 0 && (!tit || !ranks_out)) return fail(TFR_ERR_ARG, "%s: null target items / ranks_out", t.who);
    if (xip && !xit && xip[n] > xip[0]) return fail(TFR_ERR_ARG, "%s: exclusion indptr without items", t.who);
    int rc = check_ids(t.who, "user id", users, n, t.U);
    if (rc || (rc = check_csr(t.who, true, tip, tit, n, t.n_items)) || (xip && (rc = check_csr(t.who, false, xip, xit, n, t.n_items))))
        return rc;
    if (n_tgt == 0) return TFR_OK;
    // pieces in row order: tlo absolute into tit, xlo / xhi absolute into xit (rebased per chunk below); prow = their rows
    std::vector<RankPiece> pieces;
    std::vector<int64_t> prow;
    for (int64_t r = 0; r < n; ++r)
        for (int64_t e = tip[r]; e < tip[r + 1]; e += RANK_CAP) {
            const int64_t nt = tip[r + 1] - e < RANK_CAP ? tip[r + 1] - e : RANK_CAP;
            pieces.push_back({e, xip ? xip[r] : 0, xip ? xip[r + 1] : 0, users[r], (int32_t)nt});
            prow.push_back(r);
        }
    const int64_t np = (int64_t)pieces.size();
    RankPlan p;
    if (!rank_plan(np, t.n_items, &p)) return fail(TFR_ERR_ARG, "%s: no plan for %lld pieces", t.who, (long long)np);
    if (t.settle && (rc = settle_q(m))) return rc;       // item rows the fused big-table step left in q_alt come back first
    hipStream_t s = m->stream;
    HIPCHK(m->rk_pieces.reserve(pow2_cap(p.chunk), s));
    HIPCHK(reserve_each(pow2_cap(p.chunk * RANK_CAP), s, m->rk_tgt, m->rk_ranks, m->rk_order, m->rk_bins));
    HIPCHK(m->rk_keys.reserve(pow2_cap(p.chunk * RANK_CAP), s));
    HIPCHK(m->rk_nr.reserve(pow2_cap(p.chunk), s));
    std::vector<RankPiece> staged;
    for (int64_t c0 = 0; c0 < np; c0 += p.chunk) {
        const int64_t cnt = np - c0 < p.chunk ? np - c0 : p.chunk;
        const int64_t t0 = pieces[(size_t)c0].tlo;
        const int64_t t1 = pieces[(size_t)(c0 + cnt - 1)].tlo + pieces[(size_t)(c0 + cnt - 1)].nt;
        const int64_t x0 = xip ? xip[prow[(size_t)c0]] : 0;
        const int64_t x1 = xip ? xip[prow[(size_t)(c0 + cnt - 1)] + 1] : 0;
        staged.assign(pieces.begin() + c0, pieces.begin() + c0 + cnt);
        for (auto& q : staged) { q.tlo -= t0; q.xlo -= x0; q.xhi -= x0; }
        HIPCHK(hipMemcpyAsync(m->rk_pieces, staged.data(), (size_t)cnt * sizeof(RankPiece), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(m->rk_tgt, tit + t0, (size_t)(t1 - t0) * 4, hipMemcpyHostToDevice, s));
        if (x1 > x0) {
            HIPCHK(m->rk_excl.reserve(pow2_cap(x1 - x0), s));
            HIPCHK(hipMemcpyAsync(m->rk_excl, xit + x0, (size_t)(x1 - x0) * 4, hipMemcpyHostToDevice, s));
        }
        RankCommon a = {};
        a.pieces = m->rk_pieces; a.tgt = m->rk_tgt; a.excl = m->rk_excl;
        a.keys = m->rk_keys; a.order = m->rk_order; a.nr = m->rk_nr; a.bins = m->rk_bins; a.ranks = m->rk_ranks;
        a.n_pieces = cnt; a.n_items = t.n_items;
        a.D = m->D; a.slices = p.slices; a.item_abs = t.item_abs;
        t.launch(a, p, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ranks_out + (t0 - tip[0]), m->rk_ranks, (size_t)(t1 - t0) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                 // the staged inputs are rewritten by the next chunk
    }
    return check_device_error(m);
}

// the float32 tables' entries (SVD, FM, SVD++) name their tables
static int rank_host(tfr_model* m, const TopkTables& t, const int32_t* users, int64_t n, const int64_t* tip,
                     const int32_t* tit, const int64_t* xip, const int32_t* xit, int32_t* ranks_out) {
    return rank_host(m, RankQuery(t), users, n, tip, tit, xip, xit, ranks_out);
}

extern "C" {

int tfr_rank_plan(int32_t dim, int64_t n_users, int64_t n_targets, int64_t item_num, int64_t* lds_bytes,
                  int32_t* pieces_per_block, int32_t* item_slices, int32_t* targets_per_piece, int64_t* piece_chunk) {
    int G, VEC;
    if (!geometry(dim, &G, &VEC)) return fail(TFR_ERR_ARG, "unsupported dim %d", dim);
    if (n_users < 0 || n_targets < 0 || item_num < 1)
        return fail(TFR_ERR_ARG, "rank plan: n_users >= 0, n_targets >= 0 and item_num >= 1");
    RankPlan p;
    if (!rank_plan(rank_pieces_bound(n_users, n_targets), item_num, &p)) return fail(TFR_ERR_ARG, "rank plan: no plan");
    if (lds_bytes) *lds_bytes = (int64_t)(p.lds_count > p.lds_targets ? p.lds_count : p.lds_targets);
    if (pieces_per_block) *pieces_per_block = p.ppb;
    if (item_slices) *item_slices = p.slices;
    if (targets_per_piece) *targets_per_piece = p.cap;
    if (piece_chunk) *piece_chunk = p.chunk;
    return TFR_OK;
}

int tfr_rank_items(tfr_model* m, const int32_t* users, int64_t n_users, const int64_t* tgt_indptr, const int32_t* tgt_items,
                   const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    MODEL_ENTER(m);
    return rank_host(m, svd_topk_tables(m), users, n_users, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

// the snapshot test comes before every other check, n_users == 0 included, as in the other tfr_bf16_* entries
int tfr_bf16_rank_items(tfr_model* m, const int32_t* users, int64_t n_users, const int64_t* tgt_indptr,
                        const int32_t* tgt_items, const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    MODEL_ENTER(m);
    if (int rc = bf16_need_snapshot(m)) return rc;
    return rank_host(m, Bf16RankQuery(m), users, n_users, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

int tfr_fm_rank_items(tfr_fm* f, const int32_t* user_features, int64_t n_users, int64_t item_lo, int64_t item_hi,
                      const int64_t* tgt_indptr, const int32_t* tgt_items, const int64_t* excl_indptr,
                      const int32_t* excl_items, int32_t* ranks_out) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    TopkTables t;
    const int rc = fm_topk_tables(m, "rank", item_lo, item_hi, &t);
    return rc ? rc : rank_host(m, t, user_features, n_users, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

}  // extern "C"

// ---- batched per-user fine-tuning (finetune.hip) ----------------------------------------------------------------------------
// beta powers of the sequential drivers: the model's float32 recurrence (one multiply per step after the applies) replayed from
// its current values.  out[2k], out[2k+1] = the powers at step seq[k] of the call; end = after n_total steps.  The walk stops
// early once both powers reach a fixed point (they underflow to zero after ~10^5 steps with the default betas).
static void ft_replay_powers(float b1p, float b2p, float b1, float b2, const int64_t* seq, int64_t n, int64_t n_total,
                             std::vector<float>& out, float* end1, float* end2) {
    std::vector<int64_t> idx((size_t)n);
    for (int64_t k = 0; k < n; ++k) idx[(size_t)k] = k;
    std::sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return seq[x] < seq[y]; });
    out.resize((size_t)n * 2);
    int64_t t = 0;
    size_t q = 0;
    bool fixed = false;
    while (true) {
        while (q < idx.size() && seq[idx[q]] == t) {
            out[(size_t)idx[q] * 2] = b1p; out[(size_t)idx[q] * 2 + 1] = b2p;
            ++q;
        }
        if (t == n_total || fixed) break;
        const float n1 = b1p * b1, n2 = b2p * b2;
        fixed = n1 == b1p && n2 == b2p;
        b1p = n1; b2p = n2;
        ++t;
    }
    for (; q < idx.size(); ++q) { out[(size_t)idx[q] * 2] = b1p; out[(size_t)idx[q] * 2 + 1] = b2p; }
    *end1 = b1p; *end2 = b2p;
}

static size_t ft_align(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" {

int tfr_finetune_plan(int32_t dim, int64_t max_rows, int64_t* lds_bytes, int32_t* rows_staged, int32_t* waves_per_block) {
    int G, VEC;
    if (!geometry(dim, &G, &VEC)) return fail(TFR_ERR_ARG, "unsupported dim %d", dim);
    if (max_rows < 0) return fail(TFR_ERR_ARG, "fine-tune plan: negative max_rows");
    const FtPlan p = ft_plan(dim, max_rows);
    if (lds_bytes) *lds_bytes = (int64_t)p.lds_bytes;
    if (rows_staged) *rows_staged = p.rows_staged;
    if (waves_per_block) *waves_per_block = FT_WAVES;
    return TFR_OK;
}

int tfr_finetune_users(tfr_model* m, int64_t n_users, const int32_t* users, const int64_t* row_ptr, const int32_t* items,
                       const float* rates, const int64_t* round_ptr, const int32_t* ask_items, const int32_t* prefix_len,
                       const int64_t* round_seq, int32_t nsteps, float* ask_logits_out, float* round_loss_out,
                       float* final_logits_out) {
    MODEL_ENTER(m);
    const tfr_opts& o = m->o;
    const bool adam = o.optimizer == TFR_OPT_ADAM;
    // --- every check before any device work: on an error nothing changes
    if (n_users < 0) return fail(TFR_ERR_ARG, "fine-tune: negative n_users");
    if (nsteps < 1) return fail(TFR_ERR_ARG, "fine-tune: nsteps must be at least 1 (got %d)", nsteps);
    if (adam && o.adam_mode == TFR_ADAM_TF1)
        return fail(TFR_ERR_ARG, "fine-tune: tf1-mode Adam moves every user row at every step, so the users are not independent "
                                 "(use lazy Adam or SGD, or the sequential drivers)");
    const uint32_t need = (1u << TFR_MU) | (1u << TFR_BI) | (1u << TFR_Q);
    if ((m->frozen & need) != need)
        return fail(TFR_ERR_ARG, "fine-tune: bias_global, item_bias and item_features must be frozen (frozen mask 0x%x)", m->frozen);
    if (n_users == 0) return TFR_OK;
    if (!users || !row_ptr || !round_ptr || !ask_logits_out) return fail(TFR_ERR_ARG, "fine-tune: null users / offsets / output");
    if (row_ptr[0] != 0 || round_ptr[0] != 0) return fail(TFR_ERR_ARG, "fine-tune: row_ptr and round_ptr must start at 0");
    for (int64_t u = 0; u < n_users; ++u) {
        if (row_ptr[u + 1] < row_ptr[u]) return fail(TFR_ERR_ARG, "fine-tune: row_ptr decreases at user %lld", (long long)u);
        if (round_ptr[u + 1] < round_ptr[u]) return fail(TFR_ERR_ARG, "fine-tune: round_ptr decreases at user %lld", (long long)u);
    }
    const int64_t n_rows = row_ptr[n_users], n_rounds = round_ptr[n_users];
    if (n_rows > 0 && (!items || !rates)) return fail(TFR_ERR_ARG, "fine-tune: null items / rates");
    if (n_rounds > 0 && (!ask_items || !prefix_len)) return fail(TFR_ERR_ARG, "fine-tune: null ask_items / prefix_len");
    if (n_rounds > INT64_MAX / nsteps) return fail(TFR_ERR_ARG, "fine-tune: n_rounds x nsteps overflows");
    if (n_users > INT32_MAX) return fail(TFR_ERR_ARG, "fine-tune: too many users");
    int rc;
    if ((rc = check_ids("fine-tune", "user id", users, n_users, m->U)) || (rc = check_ids("fine-tune", "item id", items, n_rows, m->I)) ||
        (rc = check_ids("fine-tune", "asked item id", ask_items, n_rounds, m->I)))
        return rc;
    {
        // two waves on one user row would race: every user at most once
        std::vector<int32_t> sorted(users, users + n_users);
        std::sort(sorted.begin(), sorted.end());
        for (int64_t u = 1; u < n_users; ++u)
            if (sorted[(size_t)u] == sorted[(size_t)u - 1])
                return fail(TFR_ERR_ARG, "fine-tune: user %d appears more than once", sorted[(size_t)u]);
    }
    const int64_t n_total = n_rounds * nsteps;
    int64_t max_rows = 0;
    std::vector<int64_t> work((size_t)n_users, 0);
    for (int64_t u = 0; u < n_users; ++u) {
        const int64_t n = row_ptr[u + 1] - row_ptr[u];
        if (n > max_rows && round_ptr[u + 1] > round_ptr[u]) max_rows = n;
        for (int64_t k = round_ptr[u]; k < round_ptr[u + 1]; ++k) {
            if (prefix_len[k] < 1 || prefix_len[k] > n)
                return fail(TFR_ERR_ARG, "fine-tune: round %lld trains on %d rows, its user has %lld", (long long)k, prefix_len[k],
                            (long long)n);
            work[(size_t)u] += prefix_len[k];
        }
    }
    if (round_seq)
        for (int64_t k = 0; k < n_rounds; ++k)
            if (round_seq[k] < 0 || round_seq[k] > n_total - nsteps)
                return fail(TFR_ERR_ARG, "fine-tune: round %lld starts at step %lld, outside [0, %lld]", (long long)k,
                            (long long)round_seq[k], (long long)(n_total - nsteps));
    int G, VEC;
    if (!geometry(m->D, &G, &VEC)) return fail(TFR_ERR_ARG, "fine-tune: unsupported dim %d", m->D);
    // --- host-side schedule: beta powers at each round's first step, users by descending work
    std::vector<float> bpow;
    float end1 = m->b1p, end2 = m->b2p;
    if (adam) {
        std::vector<int64_t> seq;
        if (!round_seq) {
            seq.resize((size_t)n_rounds);
            for (int64_t k = 0; k < n_rounds; ++k) seq[(size_t)k] = k * nsteps;
        }
        ft_replay_powers(m->b1p, m->b2p, o.beta1, o.beta2, round_seq ? round_seq : seq.data(), n_rounds, n_total, bpow, &end1,
                         &end2);
    }
    std::vector<int32_t> order((size_t)n_users);
    for (int64_t u = 0; u < n_users; ++u) order[(size_t)u] = (int32_t)u;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return work[(size_t)x] > work[(size_t)y]; });
    const FtPlan plan = ft_plan(m->D, max_rows);
    // --- one device buffer: inputs, then outputs
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off = ft_align(off + bytes); return at; };
    const size_t o_users = take((size_t)n_users * 4), o_rowp = take((size_t)(n_users + 1) * 8), o_items = take((size_t)n_rows * 4),
                 o_rates = take((size_t)n_rows * 4), o_rndp = take((size_t)(n_users + 1) * 8), o_ask = take((size_t)n_rounds * 4),
                 o_pre = take((size_t)n_rounds * 4), o_bpow = take(bpow.size() * 4), o_order = take((size_t)n_users * 4),
                 o_askout = take((size_t)n_rounds * 4), o_loss = take(round_loss_out ? (size_t)n_rounds * 4 : 0),
                 o_final = take(final_logits_out ? (size_t)n_rows * 4 : 0);
    HIPCHK(m->ft_buf.reserve((int64_t)off, m->stream));
    if ((rc = settle_q(m))) return rc;                   // item rows the fused big-table step left in q_alt come back first
    forget_kept_batch(m);                                // a training call
    char* b = m->ft_buf;
    hipStream_t s = m->stream;
    auto up = [&](size_t at, const void* src, size_t bytes) -> int {
        if (bytes) HIPCHK(hipMemcpyAsync(b + at, src, bytes, hipMemcpyHostToDevice, s));
        return TFR_OK;
    };
    if ((rc = up(o_users, users, (size_t)n_users * 4)) || (rc = up(o_rowp, row_ptr, (size_t)(n_users + 1) * 8)) ||
        (rc = up(o_items, items, (size_t)n_rows * 4)) || (rc = up(o_rates, rates, (size_t)n_rows * 4)) ||
        (rc = up(o_rndp, round_ptr, (size_t)(n_users + 1) * 8)) || (rc = up(o_ask, ask_items, (size_t)n_rounds * 4)) ||
        (rc = up(o_pre, prefix_len, (size_t)n_rounds * 4)) || (rc = up(o_bpow, bpow.data(), bpow.size() * 4)) ||
        (rc = up(o_order, order.data(), (size_t)n_users * 4)) ||
        (final_logits_out && (rc = up(o_final, final_logits_out, (size_t)n_rows * 4))))   // rows the call does not write stay
        return rc;
    FtArgs a;
    memset(&a, 0, sizeof(a));
    a.P = m->w[TFR_P]; a.bu = m->w[TFR_BU];
    a.Pm = m->m[TFR_P]; a.Pv = m->v[TFR_P]; a.bum = m->m[TFR_BU]; a.buv = m->v[TFR_BU];
    a.Q = m->w[TFR_Q]; a.bi = m->w[TFR_BI]; a.mu = m->w[TFR_MU];
    a.users = (const int32_t*)(b + o_users); a.row_ptr = (const int64_t*)(b + o_rowp);
    a.items = (const int32_t*)(b + o_items); a.rates = (const float*)(b + o_rates);
    a.round_ptr = (const int64_t*)(b + o_rndp); a.ask = (const int32_t*)(b + o_ask); a.prefix = (const int32_t*)(b + o_pre);
    a.bpow = adam ? (const float*)(b + o_bpow) : nullptr; a.order = (const int32_t*)(b + o_order);
    a.ask_out = (float*)(b + o_askout);
    a.loss_out = round_loss_out ? (float*)(b + o_loss) : nullptr;
    a.final_out = final_logits_out ? (float*)(b + o_final) : nullptr;
    a.n_users = n_users; a.wave_floats = plan.wave_floats;
    a.D = m->D; a.nsteps = nsteps; a.loss = o.loss; a.item_abs = o.item_abs; a.reg_bias = o.reg_bias; a.adam = adam ? 1 : 0;
    a.frozen_rows = (m->frozen >> TFR_P) & 1; a.frozen_bias = (m->frozen >> TFR_BU) & 1; a.rows_staged = plan.rows_staged;
    a.lam = o.reg; a.lr = o.lr; a.b1 = o.beta1; a.b2 = o.beta2; a.eps = o.eps;
    launch_finetune(a, plan, s);
    HIPCHK(hipGetLastError());
    if (n_rounds) HIPCHK(hipMemcpyAsync(ask_logits_out, a.ask_out, (size_t)n_rounds * 4, hipMemcpyDeviceToHost, s));
    if (round_loss_out && n_rounds) HIPCHK(hipMemcpyAsync(round_loss_out, a.loss_out, (size_t)n_rounds * 4, hipMemcpyDeviceToHost, s));
    if (final_logits_out && n_rows) HIPCHK(hipMemcpyAsync(final_logits_out, a.final_out, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    m->step += n_total;
    if (adam) { m->b1p = end1; m->b2p = end2; }
    return TFR_OK;
}

}  // extern "C"

// ---- SVD++ (tfr_svdpp*, svdpp.hip): the wrapped model's internals are shared, so its entry points live in this unit
#include "svdpp_api.inc.h"
// ---- BPR steps (tfr_bpr_*, bpr.hip) on the model's own tables
#include "bpr_api.inc.h"
// ---- WARP trainer (tfr_warp_*, warp.hip): BPR's step with the violator search and the weighted hinge
#include "warp_api.inc.h"
// ---- FM trainer (tfr_fm_*_resident, fm_fit.hip): resident row stores, gathered minibatches, metrics
#include "fm_fit_api.inc.h"

#include "neighbours_api.inc.h"
