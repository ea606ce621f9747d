// bpr_api.inc.h - the tfr_bpr entry points (include/tfrecomm.h), compiled inside api.hip: a BPR step runs on a
// tfr_model and shares its internals (tables, optimiser, step bookkeeping, radix sort, error flag, k_finalize, generator).
//
// A step on the model's stream:
//   k_bpr_sample   per triple: (u, i) from the columns or the drawn entries, j from the sampler or the caller; the two
//                  2B-key columns (user, item) of the occurrences
//   radix sort     both columns at once (ids checked: a bad id sets the flag and every later kernel returns)
//   k_bpr_users    per user run: scores, g, data and regulariser terms, the pre-step P row to pold, the P update
//   k_bpr_items    per item run: the Q / item_bias gradient from pold and g, and its update
//   k_finalize     {data, reg} over the per-run scalars in position order (bias_global is not touched)
#include "bpr.h"
#include "warp.h"

struct BprState {
    // the positives CSR and the row of each entry
    DevBuf<int64_t> ip;
    DevBuf<int32_t> idx, rowof;
    int64_t nnz = 0;
    bool have_pos = false;
    uint64_t seed = 0;
    int32_t attempts = 16;
    // per triple (cap) and per occurrence (2 cap)
    DevBuf<int32_t> ou, oi, pos, neg, negin, head;
    DevBuf<float> g, pold, scal, out4;
    int64_t cap = 0;
    // the drawn form: its own id buffer, per-step {data, reg, -, flag}, and the events ordering the draw stream with it
    DevBuf<int64_t> ids;
    DevBuf<float> losses;
    hipEvent_t ev_free = nullptr, ev_drawn = nullptr;
};

static void bpr_release(tfr_model* m) {
    BprState* h = m->bpr;
    if (!h) return;
    if (h->ev_free) (void)hipEventDestroy(h->ev_free);
    if (h->ev_drawn) (void)hipEventDestroy(h->ev_drawn);
    delete h;                                            // (the model's device is current: tfr_destroy)
    m->bpr = nullptr;
}

static int bpr_state(tfr_model* m, BprState** out) {
    if (!m->bpr) {
        m->bpr = new (std::nothrow) BprState();
        if (!m->bpr) return fail(TFR_ERR_NOMEM, "host allocation failed");
    }
    *out = m->bpr;
    return TFR_OK;
}

// the search's argument block from the sampler's: the same batch, positives, key and outputs, plus the tables it scores on
static WarpSampleArgs warp_sample_args(const tfr_model* m, const BprSampleArgs& sa, const WarpStep& wp) {
    WarpSampleArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.pos = sa.pos;
    wa.ids = sa.ids; wa.u_in = sa.u_in; wa.i_in = sa.i_in; wa.neg_in = sa.neg_in;
    wa.P = m->w[TFR_P]; wa.Q = m->w[TFR_Q]; wa.bi = m->w[TFR_BI];
    wa.ou = sa.ou; wa.oi = sa.oi; wa.pos_out = sa.pos_out; wa.neg = sa.neg; wa.neg_copy = sa.neg_copy;
    wa.trials = wp.trials; wa.wgt = wp.wgt; wa.trials_copy = wp.trials_copy;
    wa.key = sa.key;
    wa.B = sa.B; wa.U = sa.U; wa.I = sa.I;
    wa.D = m->D; wa.item_abs = m->o.item_abs; wa.attempts = sa.attempts;
    wa.margin = wp.margin;
    return wa;
}

static int bpr_need_pos(const tfr_model* m) {
    return m->bpr && m->bpr->have_pos ? TFR_OK : fail(TFR_ERR_STATE, "BPR: the positives are not set (tfr_bpr_set_positives)");
}

static int bpr_need_opt(const tfr_model* m) {
    if (opt_step(m).tf1) return fail(TFR_ERR_STATE, "BPR training supports SGD and lazy Adam (not tf1 Adam)");
    return TFR_OK;
}

// the per-triple buffers of a B-triple step, and the model's sort workspace for its 2B occurrences
static int bpr_ensure_batch(tfr_model* m, BprState* h, int64_t B) {
    int rc = ensure_capacity(m, B > 0 ? 2 * B : 1);
    if (rc) return rc;
    if (B > h->cap) {
        const int64_t c = pow2_cap(B);
        hipStream_t s = m->stream;
        HIPCHK(reserve_each(2 * c, s, h->ou, h->oi));
        HIPCHK(reserve_each(c, s, h->pos, h->neg, h->negin, h->head));
        HIPCHK(h->g.reserve(c, s));
        HIPCHK(h->pold.reserve(c * m->D, s));
        HIPCHK(h->scal.reserve(c * 4, s));
        h->cap = c;
    }
    HIPCHK(h->out4.reserve(4, m->stream));
    return TFR_OK;
}

// one step: users du + positives dpos, or drawn entries d_ids of the positives; negatives dneg (NULL = sample).
// d_neg_copy (may be NULL) receives the negatives; out4 (device, may be NULL) {data, reg, 0, error flag}.
// wp (warp_api.inc.h) makes it a WARP step: the violator search in place of the sampler, the hinge form of the user runs
static int bpr_step(tfr_model* m, BprState* h, const int32_t* du, const int32_t* dpos, const int32_t* dneg,
                    const int64_t* d_ids, int64_t B, int32_t* d_neg_copy, float* out4, const WarpStep* wp = nullptr) {
    const OptStep k = opt_step(m);
    int rc;
    if ((rc = settle_q(m)) || (rc = bpr_ensure_batch(m, h, B))) return rc;
    forget_kept_batch(m);                                // a training call
    hipStream_t s = m->stream;
    if (B > 0) {
        BprSampleArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.pos = {h->ip, h->idx, h->rowof, h->nnz};
        sa.ids = d_ids; sa.u_in = du; sa.i_in = dpos; sa.neg_in = dneg;
        sa.ou = h->ou; sa.oi = h->oi; sa.pos_out = h->pos; sa.neg = h->neg; sa.neg_copy = d_neg_copy;
        sa.key = bpr_key(h->seed, m->step);
        sa.B = B; sa.U = m->U; sa.I = m->I; sa.attempts = h->attempts;
        {
            Prof p(m, TFR_K_GATHER);
            if (wp) launch_warp_sample(warp_sample_args(m, sa, *wp), s);
            else launch_bpr_sample(sa, s);
        }
        HIPCHK(hipGetLastError());
        {
            Prof p(m, TFR_K_SORT);
            if ((rc = sort_model_columns(m, h->ou, h->oi, 2 * B, true))) return rc;
        }
        BprArgs a;
        memset(&a, 0, sizeof(a));
        a.P = m->w[TFR_P]; a.Q = m->w[TFR_Q]; a.bi = m->w[TFR_BI];
        a.Pm = m->m[TFR_P]; a.Pv = m->v[TFR_P]; a.Qm = m->m[TFR_Q]; a.Qv = m->v[TFR_Q]; a.bim = m->m[TFR_BI]; a.biv = m->v[TFR_BI];
        a.ks_u = m->ks_u; a.ps_u = m->ps_u; a.ks_i = m->ks_i; a.ps_i = m->ps_i;
        a.pos = h->pos; a.neg = h->neg; a.g = h->g; a.head = h->head; a.pold = h->pold; a.scal = h->scal;
        a.err = m->d_err;
        a.B = B; a.D = m->D; a.item_abs = m->o.item_abs; a.reg_bias = m->o.reg_bias; a.opt = k.adam ? 0 : 1;
        a.frozen = m->frozen; a.lam = m->o.reg;
        if (wp) { a.wgt = wp->wgt; a.margin = wp->margin; }
        set_hyper(a, k);
        a.omb1 = 1.f - k.b1; a.omb2 = 1.f - k.b2;
        {
            Prof p(m, TFR_K_REDUCE_USER);
            launch_bpr_users(a, s);
        }
        {
            Prof p(m, TFR_K_REDUCE_ITEM);
            launch_bpr_items(a, s);
        }
        HIPCHK(hipGetLastError());
    }
    FinArgs f = mu_fin(m, k, false, out4);
    f.partials = h->scal; f.nblk = (int32_t)B; f.out_err = out4 ? 1 : 0;
    {
        Prof p(m, TFR_K_FINALIZE);
        launch_finalize(f, s);
    }
    HIPCHK(hipGetLastError());
    advance_step(m);
    return TFR_OK;
}

extern "C" {

int tfr_bpr_set_positives(tfr_model* m, const int64_t* indptr, const int32_t* items) {
    MODEL_ENTER(m);
    const int64_t U = m->U, I = m->I;
    if (!indptr) return fail(TFR_ERR_ARG, "BPR positives: null indptr");
    if (indptr[0] != 0) return fail(TFR_ERR_ARG, "BPR positives: indptr must start at 0");
    if (indptr[U] > 0 && !items) return fail(TFR_ERR_ARG, "BPR positives: null items");
    int rc = check_csr("BPR positives", true, indptr, items, U, I);
    if (rc) return rc;
    const int64_t nnz = indptr[U];
    if (nnz > 0x7fffffffLL) return fail(TFR_ERR_ARG, "BPR positives: more than 2^31 - 1 entries");
    BprState* h;
    if ((rc = bpr_state(m, &h))) return rc;
    std::vector<int32_t> rowof((size_t)(nnz > 0 ? nnz : 1), 0);
    for (int64_t u = 0; u < U; ++u)
        for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) rowof[(size_t)e] = (int32_t)u;
    hipStream_t s = m->stream;
    h->have_pos = false;
    HIPCHK(hipStreamSynchronize(s));                     // nothing in flight still reads the old positives
    HIPCHK(h->ip.reserve(U + 1, s));
    HIPCHK(h->idx.reserve(nnz > 0 ? nnz : 1, s));
    HIPCHK(h->rowof.reserve(nnz > 0 ? nnz : 1, s));
    HIPCHK(hipMemcpyAsync(h->ip, indptr, (size_t)(U + 1) * 8, hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(h->idx, items, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(h->rowof, rowof.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));                     // the host vector goes out of scope
    h->nnz = nnz;
    h->have_pos = true;
    return TFR_OK;
}

int tfr_bpr_set_sampler(tfr_model* m, uint64_t seed, int32_t attempts) {
    MODEL_ENTER(m);
    if (attempts < 1 || attempts > BPR_MAX_ATTEMPTS)
        return fail(TFR_ERR_ARG, "BPR sampler: attempts must be in [1, %d] (got %d)", BPR_MAX_ATTEMPTS, attempts);
    BprState* h;
    int rc = bpr_state(m, &h);
    if (rc) return rc;
    h->seed = seed;
    h->attempts = attempts;
    return TFR_OK;
}

int tfr_bpr_negatives(tfr_model* m, const int32_t* user, int64_t B, int64_t step, int32_t* neg_out) {
    MODEL_ENTER(m);
    if (B < 0) return fail(TFR_ERR_ARG, "negative batch");
    int rc = bpr_need_pos(m);
    if (rc || B == 0) return rc;
    if (!user || !neg_out) return fail(TFR_ERR_ARG, "BPR negatives: null user / neg_out");
    if ((rc = check_ids("BPR negatives", "user id", user, B, m->U))) return rc;
    BprState* h = m->bpr;
    if ((rc = bpr_ensure_batch(m, h, B))) return rc;
    hipStream_t s = m->stream;
    HIPCHK(hipMemcpyAsync(m->d_u, user, (size_t)B * 4, hipMemcpyHostToDevice, s));
    BprSampleArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.pos = {h->ip, h->idx, h->rowof, h->nnz};
    sa.u_in = m->d_u; sa.neg = h->neg;
    sa.key = bpr_key(h->seed, step);
    sa.B = B; sa.U = m->U; sa.I = m->I; sa.attempts = h->attempts;
    launch_bpr_sample(sa, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(neg_out, h->neg, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFR_OK;
}

int tfr_bpr_train_step(tfr_model* m, const int32_t* user, const int32_t* pos, const int32_t* neg, int64_t B,
                       int32_t* neg_out, float* loss_out, float* reg_out, int64_t* n_skipped_out) {
    MODEL_ENTER(m);
    int rc = check_batch(user, pos, B);
    if (rc || (rc = bpr_need_opt(m)) || (rc = bpr_need_pos(m))) return rc;
    BprState* h = m->bpr;
    if ((rc = bpr_ensure_batch(m, h, B))) return rc;
    hipStream_t s = m->stream;
    const StepMark mark = mark_step(m);
    if (B > 0) {
        HIPCHK(hipMemcpyAsync(m->d_u, user, (size_t)B * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(m->d_i, pos, (size_t)B * 4, hipMemcpyHostToDevice, s));
        if (neg) HIPCHK(hipMemcpyAsync(h->negin, neg, (size_t)B * 4, hipMemcpyHostToDevice, s));
    }
    if ((rc = bpr_step(m, h, m->d_u, m->d_i, neg ? h->negin.get() : nullptr, nullptr, B, nullptr, h->out4))) return rc;
    float back4[4];
    std::vector<int32_t> negs;
    const bool want_negs = B > 0 && !neg && (neg_out || n_skipped_out);
    if (want_negs) {
        negs.resize((size_t)B);
        HIPCHK(hipMemcpyAsync(negs.data(), h->neg, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(back4, h->out4, sizeof(back4), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int32_t e = (int32_t)back4[3];
    if (e) {                                             // a bad batch never advances the step
        rollback_step(m, mark);
        return device_error(m, e);
    }
    int64_t skipped = 0;
    if (want_negs)
        for (int64_t b = 0; b < B; ++b) skipped += negs[(size_t)b] < 0;
    if (neg_out && B > 0) memcpy(neg_out, neg ? neg : negs.data(), (size_t)B * 4);
    if (loss_out) *loss_out = back4[0];
    if (reg_out) *reg_out = back4[1];
    if (n_skipped_out) *n_skipped_out = skipped;
    return TFR_OK;
}

int tfr_bpr_train_step_dev(tfr_model* m, const int32_t* d_user, const int32_t* d_pos, const int32_t* d_neg, int64_t B,
                           int32_t* d_neg_out) {
    MODEL_ENTER(m);
    int rc = check_batch(d_user, d_pos, B);
    if (rc || (rc = bpr_need_opt(m)) || (rc = bpr_need_pos(m))) return rc;
    return bpr_step(m, m->bpr, d_user, d_pos, d_neg, nullptr, B, d_neg_out, nullptr);
}

}  // extern "C"

// the drawn form of tfr_bpr_train_steps_drawn and tfr_warp_train_steps_drawn (wp set)
static int bpr_steps_drawn(tfr_model* m, int64_t B, int32_t nsteps, float* loss_out, const WarpStep* wp) {
    int rc;
    if ((rc = bpr_need_opt(m)) || (rc = bpr_need_pos(m))) return rc;
    if (!m->rng_set) return fail(TFR_ERR_STATE, "no generator state: call tfr_rng_seed / tfr_rng_set_state first");
    if (B < 1 || nsteps < 0) return fail(TFR_ERR_ARG, "bad batch/nsteps");
    if (nsteps == 0) return TFR_OK;
    BprState* h = m->bpr;
    if ((rc = check_high(h->nnz))) return rc;
    if ((rc = cancel_run_ahead(m))) return rc;           // the generator goes on from where the consumed ids end
    const int64_t total = B * (int64_t)nsteps;
    hipStream_t s = m->stream;
    if (!h->ev_free) {
        HIPCHK(hipEventCreateWithFlags(&h->ev_free, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_drawn, hipEventDisableTiming));
    }
    HIPCHK(h->ids.reserve(total, s));                    // (a reallocation synchronises the steps that read the old one)
    if (loss_out) HIPCHK(h->losses.reserve(4 * (int64_t)nsteps, s));
    // the draw overwrites the id buffer once every step already queued has read it; the steps wait for the draw
    HIPCHK(hipEventRecord(h->ev_free, s));
    HIPCHK(hipStreamWaitEvent(m->stream3, h->ev_free, 0));
    if (h->nnz == 1) {                                   // rng == 0: no draw is consumed
        HIPCHK(hipMemsetAsync(h->ids, 0, (size_t)total * 8, m->stream3));
    } else {
        const uint32_t rng = (uint32_t)(h->nnz - 1);
        {
            Prof p(m, TFR_K_DRAW);
            launch_mt_draw(m->d_rng, h->ids, total, rng, mask_for(rng), m->stream3, nullptr, &m->rng_ws);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(h->ev_drawn, m->stream3));
    HIPCHK(hipStreamWaitEvent(s, h->ev_drawn, 0));
    const StepMark mark = mark_step(m);
    for (int32_t st = 0; st < nsteps; ++st)
        if ((rc = bpr_step(m, h, nullptr, nullptr, nullptr, h->ids + (int64_t)st * B, B, nullptr,
                           loss_out ? h->losses + 4 * (int64_t)st : nullptr, wp)))
            return rc;
    if (!loss_out) return TFR_OK;
    std::vector<float> back((size_t)nsteps * 4);
    HIPCHK(hipMemcpyAsync(back.data(), h->losses, back.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int32_t st = 0; st < nsteps; ++st) {
        const int32_t e = (int32_t)back[(size_t)st * 4 + 3];
        if (e) {                                         // (drawn ids are in range by construction)
            rollback_step(m, mark);
            return device_error(m, e);
        }
        loss_out[st] = back[(size_t)st * 4];
    }
    return TFR_OK;
}

extern "C" {

int tfr_bpr_train_steps_drawn(tfr_model* m, int64_t B, int32_t nsteps, float* loss_out) {
    MODEL_ENTER(m);
    return bpr_steps_drawn(m, B, nsteps, loss_out, nullptr);
}

}  // extern "C"
