// warp_api.inc.h - the tfr_warp entry points (include/tfrecomm.h), compiled inside api.hip after
// bpr_api.inc.h: a WARP trainer is bound to a tfr_model and steps its tables through bpr_step, with the model's positives,
// sampler settings, per-triple buffers and drawn-id machinery (BprState).  What the trainer owns is the margin and the
// per-triple trial counts and weights.
//
// A step on the model's stream:
//   k_warp_sample  per triple: (u, i) from the columns or the drawn entries; the first margin violator among the
//                  candidates, its trial count and weight (or the caller's negative with N = 1); the two 2B-key columns
//   radix sort, k_bpr_users<NJ, true> (the weighted hinge), k_bpr_items, k_finalize: as a BPR step
#include "warp.h"

struct tfr_warp {
    tfr_model* m = nullptr;
    float margin = 1.f;
    DevBuf<int32_t> trials;                              // [cap] N per triple
    DevBuf<float> wgt;                                   // [cap] w per triple
};

#define WARP_ENTER(w)                                                 \
    if (!(w)) return fail(TFR_ERR_ARG, "null WARP trainer");          \
    tfr_model* m = (w)->m;                                            \
    HIPCHK(hipSetDevice(m->device));

static int warp_check_margin(float margin) {
    return margin != margin ? fail(TFR_ERR_ARG, "WARP: the margin is NaN") : TFR_OK;
}

// what every searching or training call needs: two items at least, the positives, and the buffers of a B-triple batch
static int warp_ready(tfr_warp* w, int64_t B, bool training) {
    tfr_model* m = w->m;
    if (m->I < 2) return fail(TFR_ERR_ARG, "WARP needs item_num >= 2 (the weight is log((item_num - 1) / N))");
    int rc;
    if ((training && (rc = bpr_need_opt(m))) || (rc = bpr_need_pos(m)) || (rc = bpr_ensure_batch(m, m->bpr, B))) return rc;
    const int64_t c = pow2_cap(B > 0 ? B : 1);
    HIPCHK(w->trials.reserve(c, m->stream));
    HIPCHK(w->wgt.reserve(c, m->stream));
    return TFR_OK;
}

extern "C" {

int tfr_warp_create(tfr_warp** out, tfr_model* m, float margin) {
    if (!out) return fail(TFR_ERR_ARG, "null out");
    *out = nullptr;
    MODEL_ENTER(m);
    int rc = warp_check_margin(margin);
    if (rc) return rc;
    BprState* h;
    if ((rc = bpr_state(m, &h))) return rc;
    tfr_warp* w = new (std::nothrow) tfr_warp();
    if (!w) return fail(TFR_ERR_NOMEM, "host allocation failed");
    w->m = m;
    w->margin = margin;
    m->warp_live += 1;
    *out = w;
    return TFR_OK;
}

int tfr_warp_destroy(tfr_warp* w) {
    if (!w) return TFR_OK;
    tfr_model* m = w->m;
    (void)hipSetDevice(m->device);                       // the buffers are freed with the model's device current
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    m->warp_live -= 1;
    delete w;
    return TFR_OK;
}

int tfr_warp_set_margin(tfr_warp* w, float margin) {
    WARP_ENTER(w);
    int rc = warp_check_margin(margin);
    if (rc) return rc;
    w->margin = margin;
    return TFR_OK;
}

int tfr_warp_negatives(tfr_warp* w, const int32_t* user, const int32_t* pos, int64_t B, int64_t step, int32_t* neg_out,
                       int32_t* trials_out) {
    WARP_ENTER(w);
    if (B < 0) return fail(TFR_ERR_ARG, "negative batch");
    int rc = warp_ready(w, B, false);
    if (rc || B == 0) return rc;
    if (!user || !pos || !neg_out) return fail(TFR_ERR_ARG, "WARP negatives: null user / pos / neg_out");
    if ((rc = check_ids("WARP negatives", "user id", user, B, m->U)) || (rc = check_ids("WARP negatives", "item id", pos, B, m->I)))
        return rc;
    if ((rc = settle_q(m))) return rc;
    BprState* h = m->bpr;
    hipStream_t s = m->stream;
    HIPCHK(hipMemcpyAsync(m->d_u, user, (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m->d_i, pos, (size_t)B * 4, hipMemcpyHostToDevice, s));
    BprSampleArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.pos = {h->ip, h->idx, h->rowof, h->nnz};
    sa.u_in = m->d_u; sa.i_in = m->d_i; sa.neg = h->neg;
    sa.key = bpr_key(h->seed, step);
    sa.B = B; sa.U = m->U; sa.I = m->I; sa.attempts = h->attempts;
    const WarpStep wp = {w->margin, w->trials, w->wgt, nullptr};
    launch_warp_sample(warp_sample_args(m, sa, wp), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(neg_out, h->neg, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    if (trials_out) HIPCHK(hipMemcpyAsync(trials_out, w->trials, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFR_OK;
}

int tfr_warp_train_step(tfr_warp* w, const int32_t* user, const int32_t* pos, const int32_t* neg, int64_t B, int32_t* neg_out,
                        int32_t* trials_out, float* loss_out, float* reg_out, int64_t* n_skipped_out) {
    WARP_ENTER(w);
    int rc = check_batch(user, pos, B);
    if (rc || (rc = warp_ready(w, B, true))) return rc;
    BprState* h = m->bpr;
    hipStream_t s = m->stream;
    const StepMark mark = mark_step(m);
    if (B > 0) {
        HIPCHK(hipMemcpyAsync(m->d_u, user, (size_t)B * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(m->d_i, pos, (size_t)B * 4, hipMemcpyHostToDevice, s));
        if (neg) HIPCHK(hipMemcpyAsync(h->negin, neg, (size_t)B * 4, hipMemcpyHostToDevice, s));
    }
    const WarpStep wp = {w->margin, w->trials, w->wgt, nullptr};
    if ((rc = bpr_step(m, h, m->d_u, m->d_i, neg ? h->negin.get() : nullptr, nullptr, B, nullptr, h->out4, &wp))) return rc;
    float back4[4];
    std::vector<int32_t> negs, trials;
    const bool want_negs = B > 0 && !neg && (neg_out || n_skipped_out);
    if (want_negs) {
        negs.resize((size_t)B);
        HIPCHK(hipMemcpyAsync(negs.data(), h->neg, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    }
    if (trials_out && B > 0) {                           // through a vector: a void step leaves the caller's array alone
        trials.resize((size_t)B);
        HIPCHK(hipMemcpyAsync(trials.data(), w->trials, (size_t)B * 4, hipMemcpyDeviceToHost, s));
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
    if (trials_out && B > 0) memcpy(trials_out, trials.data(), (size_t)B * 4);
    if (loss_out) *loss_out = back4[0];
    if (reg_out) *reg_out = back4[1];
    if (n_skipped_out) *n_skipped_out = skipped;
    return TFR_OK;
}

int tfr_warp_train_step_dev(tfr_warp* w, const int32_t* d_user, const int32_t* d_pos, const int32_t* d_neg, int64_t B,
                            int32_t* d_neg_out, int32_t* d_trials_out) {
    WARP_ENTER(w);
    int rc = check_batch(d_user, d_pos, B);
    if (rc || (rc = warp_ready(w, B, true))) return rc;
    const WarpStep wp = {w->margin, w->trials, w->wgt, d_trials_out};
    return bpr_step(m, m->bpr, d_user, d_pos, d_neg, nullptr, B, d_neg_out, nullptr, &wp);
}

int tfr_warp_train_steps_drawn(tfr_warp* w, int64_t B, int32_t nsteps, float* loss_out) {
    WARP_ENTER(w);
    if (B < 1 || nsteps < 0) return fail(TFR_ERR_ARG, "bad batch/nsteps");
    int rc = warp_ready(w, B, true);
    if (rc) return rc;
    const WarpStep wp = {w->margin, w->trials, w->wgt, nullptr};
    return bpr_steps_drawn(m, B, nsteps, loss_out, &wp);
}

}  // extern "C"
