// fm_fit_api.inc.h - the FM trainer's entry points (include/tfrecomm.h), compiled inside api.hip: they run on a
// tfr_fm and share its internals (minibatch buffers, fm_train_core / fm_forward_core, the wrapped model's stream, error flag
// and AUC).
//
// A resident step on the model's stream:
//   launch_fm_gather   rows ids[s * batch ..) of the train store -> the handle's minibatch CSR (fm_fit.hip)
//   fm_train_core      the step tfr_fm_train_step runs on a host-fed minibatch, unchanged
// The radix sort and the segmented reduce are launched with a host-side nnz, so the host keeps the stores' row lengths and
// sums them over each step's ids: no step waits for the device to tell its size.
#include "fm_fit.h"

struct FmStore {
    DevBuf<int64_t> indptr;
    DevBuf<int32_t> indices;
    DevBuf<float> data, y;
    int64_t n = 0, nnz = 0;
    std::vector<int32_t> len;                            // host copy of the row lengths
};

struct FmFit {
    FmStore st[2];                                       // 0 = train, 1 = eval
    DevBuf<int64_t> ids, blk;                            // a call's ids; the length scan's chunk sums
    DevBuf<float> losses, met;                           // per step {data loss, -, sum g, -}; the metrics' per-block {count, nll}
    std::vector<int64_t> step_nnz;
};

static void fm_fit_release(tfr_fm* f) {
    delete f->fit;                                       // (the model's device is current: tfr_fm_destroy)
    f->fit = nullptr;
}

static int fm_fit_store(tfr_fm* f, int32_t which, FmStore** out) {
    if (which != 0 && which != 1) return fail(TFR_ERR_ARG, "which must be 0 (train) or 1 (eval)");
    if (!f->fit || !f->fit->st[which].n)
        return fail(TFR_ERR_STATE, "no resident %s rows: call tfr_fm_upload_rows first", which ? "eval" : "train");
    *out = &f->fit->st[which];
    return TFR_OK;
}

// the host half of a resident call: every id against [0, n), and each step's nnz as the sum of its rows' lengths
static int fm_fit_plan(const FmStore& st, const int64_t* ids, int64_t batch, int32_t nsteps, std::vector<int64_t>& step_nnz,
                       int64_t* max_nnz) {
    step_nnz.assign((size_t)nsteps, 0);
    int64_t mx = 0;
    const int32_t* len = st.len.data();
    for (int32_t s = 0; s < nsteps; ++s) {
        const int64_t* p = ids + (size_t)s * batch;
        int64_t t = 0;
        for (int64_t k = 0; k < batch; ++k) {
            const int64_t id = p[k];
            if ((uint64_t)id >= (uint64_t)st.n)
                return fail(TFR_ERR_OOB, "row id %lld (step %d, position %lld) out of range [0,%lld)", (long long)id, (int)s,
                            (long long)k, (long long)st.n);
            t += len[id];
        }
        step_nnz[(size_t)s] = t;
        if (t > mx) mx = t;
    }
    *max_nnz = mx;
    return TFR_OK;
}

// the minibatch buffers for `batch` rows of up to max_nnz entries, the scan scratch and n_ids ids on the device
static int fm_fit_reserve(tfr_fm* f, int64_t batch, int64_t max_nnz, int64_t n_ids) {
    tfr_model* m = f->m;
    FmFit* h = f->fit;
    hipStream_t s = m->stream;
    HIPCHK(f->d_indptr.reserve(batch + 1, s));
    HIPCHK(reserve_each(batch, s, f->d_out, f->d_y));
    HIPCHK(reserve_each(max_nnz, s, f->d_indices, f->d_data));
    HIPCHK(h->blk.reserve((batch + FM_SCAN_CHUNK - 1) / FM_SCAN_CHUNK, s));
    HIPCHK(h->ids.reserve(n_ids, s));
    return TFR_OK;
}

static int fm_fit_gather(tfr_fm* f, const FmStore& st, const int64_t* d_ids, int64_t batch, int64_t nnz) {
    FmGatherArgs g;
    g.ids = d_ids;
    g.sp = st.indptr; g.si = st.indices; g.sx = st.data; g.sy = st.y;
    g.indptr = f->d_indptr; g.indices = f->d_indices; g.data = f->d_data; g.y = f->d_y;
    g.blk = f->fit->blk;
    g.B = batch; g.nnz = nnz;
    {
        Prof p(f->m, TFR_K_GATHER);
        launch_fm_gather(g, f->m->stream);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// the wrapped model's predictions of a store's rows -> f->d_out, from its float32 tables or from its bf16 snapshot
static int fm_fit_forward(tfr_fm* f, const FmStore& st, FwdRows rows) {
    int rc = ensure_capacity(f->m, 1);
    if (rc) return rc;
    HIPCHK(f->d_out.reserve(st.n, f->m->stream));
    return fm_forward_core(f, st.indptr, st.indices, st.data, st.n, f->d_out, rows);
}

extern "C" {

int tfr_fm_upload_rows(tfr_fm* f, int32_t which, const int64_t* indptr, const int32_t* indices, const float* data,
                       const float* y, int64_t n_rows) {
    if (!f || !indptr || !y || n_rows < 1) return fail(TFR_ERR_ARG, "upload_rows: need n_rows >= 1 and non-null indptr / y");
    if (which != 0 && which != 1) return fail(TFR_ERR_ARG, "which must be 0 (train) or 1 (eval)");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    if (indptr[0] != 0) return fail(TFR_ERR_ARG, "indptr must start at 0 and be non-decreasing");
    std::vector<int32_t> len((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t l = indptr[r + 1] - indptr[r];
        if (l < 0) return fail(TFR_ERR_ARG, "indptr must start at 0 and be non-decreasing");
        if (l > INT32_MAX) return fail(TFR_ERR_ARG, "row %lld holds more than 2^31 - 1 entries", (long long)r);
        len[(size_t)r] = (int32_t)l;
    }
    const int64_t nnz = indptr[n_rows];
    if (nnz > 0 && (!indices || !data)) return fail(TFR_ERR_ARG, "null indices/data");
    for (int64_t k = 0; k < nnz; ++k)
        if ((uint64_t)(int64_t)indices[k] >= (uint64_t)m->U)
            return fail(TFR_ERR_OOB, "feature id %d (entry %lld) out of range [0,%lld)", (int)indices[k], (long long)k, (long long)m->U);
    if (!f->fit) {
        f->fit = new (std::nothrow) FmFit();
        if (!f->fit) return fail(TFR_ERR_NOMEM, "host allocation failed");
    }
    FmStore& st = f->fit->st[which];
    hipStream_t s = m->stream;
    HIPCHK(hipStreamSynchronize(s));                     // queued steps may still read the rows this upload replaces
    st.n = 0; st.nnz = 0;
    HIPCHK(st.indptr.reserve(n_rows + 1, s));
    HIPCHK(st.y.reserve(n_rows, s));
    HIPCHK(reserve_each(nnz, s, st.indices, st.data));
    HIPCHK(hipMemcpyAsync(st.indptr, indptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(st.y, y, (size_t)n_rows * 4, hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(st.indices, indices, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(st.data, data, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    st.len.swap(len);
    st.n = n_rows; st.nnz = nnz;
    return TFR_OK;
}

int tfr_fm_gather_rows(tfr_fm* f, int32_t which, const int64_t* ids, int64_t batch, int64_t* indptr_out, int32_t* indices_out,
                       float* data_out, float* y_out, int64_t nnz_cap) {
    if (!f || !ids || batch < 1 || nnz_cap < 0 || !indptr_out || !y_out) return fail(TFR_ERR_ARG, "gather_rows: bad arguments");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    FmStore* st;
    int rc = fm_fit_store(f, which, &st);
    if (rc) return rc;
    FmFit* h = f->fit;
    int64_t nnz = 0;
    if ((rc = fm_fit_plan(*st, ids, batch, 1, h->step_nnz, &nnz))) return rc;
    if (nnz > nnz_cap) return fail(TFR_ERR_ARG, "gather_rows: the rows hold %lld entries, the outputs %lld", (long long)nnz, (long long)nnz_cap);
    if (nnz > 0 && (!indices_out || !data_out)) return fail(TFR_ERR_ARG, "gather_rows: null indices/data output");
    hipStream_t s = m->stream;
    HIPCHK(hipStreamSynchronize(s));                     // queued steps may still read the ids and the minibatch buffers
    if ((rc = fm_fit_reserve(f, batch, nnz, batch))) return rc;
    HIPCHK(hipMemcpyAsync(h->ids, ids, (size_t)batch * 8, hipMemcpyHostToDevice, s));
    if ((rc = fm_fit_gather(f, *st, h->ids, batch, nnz))) return rc;
    HIPCHK(hipMemcpyAsync(indptr_out, f->d_indptr, (size_t)(batch + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(y_out, f->d_y, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    if (nnz > 0) {
        HIPCHK(hipMemcpyAsync(indices_out, f->d_indices, (size_t)nnz * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(data_out, f->d_data, (size_t)nnz * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return TFR_OK;
}

int tfr_fm_train_steps_resident(tfr_fm* f, const int64_t* ids, int64_t batch, int32_t nsteps, float* loss_out) {
    if (!f || batch < 1 || nsteps < 0 || (nsteps > 0 && !ids)) return fail(TFR_ERR_ARG, "bad batch/nsteps/ids");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    FmStore* st;
    int rc = fm_fit_store(f, 0, &st);
    if (rc) return rc;
    if (nsteps == 0) return TFR_OK;
    FmFit* h = f->fit;
    CallTrace tr("fm_steps_resident");
    int64_t max_nnz = 0;
    if ((rc = fm_fit_plan(*st, ids, batch, nsteps, h->step_nnz, &max_nnz))) return rc;     // a bad id: nothing is queued
    tr.mark("ids checked, steps sized");
    hipStream_t s = m->stream;
    HIPCHK(hipStreamSynchronize(s));                     // an earlier call's steps may still read the id buffer
    // every buffer a step needs, at the call's largest step: no step reallocates (a reserve synchronises)
    if ((rc = ensure_capacity(m, max_nnz > 0 ? max_nnz : 1))) return rc;
    if ((rc = fm_fit_reserve(f, batch, max_nnz, (int64_t)nsteps * batch))) return rc;
    HIPCHK(f->s_rows.reserve(batch * m->D, s));
    HIPCHK(f->ent.reserve(max_nnz, s));
    HIPCHK(h->losses.reserve((int64_t)nsteps * 4, s));
    HIPCHK(hipMemcpyAsync(h->ids, ids, (size_t)nsteps * batch * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                     // the caller's ids are free again
    tr.mark("ids uploaded");
    const StepMark mark = mark_step(m);
    for (int32_t k = 0; k < nsteps; ++k) {
        const int64_t nnz = h->step_nnz[(size_t)k];
        if ((rc = fm_fit_gather(f, *st, h->ids + (size_t)k * batch, batch, nnz)) ||
            (rc = fm_train_core(f, f->d_indptr, f->d_indices, f->d_data, f->d_y, batch, nnz, nullptr, h->losses + (size_t)k * 4))) {
            (void)hipStreamSynchronize(s);               // a launch failed: the call is void (tfr_train_steps_repeat)
            rollback_step(m, mark);
            return rc;
        }
    }
    tr.mark("all steps enqueued");
    if (!loss_out) return TFR_OK;
    std::vector<float> l4((size_t)nsteps * 4);
    HIPCHK(hipMemcpyAsync(l4.data(), h->losses, l4.size() * 4, hipMemcpyDeviceToHost, s));
    if ((rc = check_device_error(m))) {
        rollback_step(m, mark);
        return rc;
    }
    for (int32_t k = 0; k < nsteps; ++k) loss_out[k] = l4[(size_t)k * 4];
    return TFR_OK;
}

}  // extern "C"

// the bodies of tfr_fm_predict_resident / tfr_fm_eval_binary_resident and of their snapshot twins: only the forward differs
static int fm_predict_resident(tfr_fm* f, FwdRows rows, int32_t which, float* out) {
    if (!f || !out) return fail(TFR_ERR_ARG, "predict_resident: null argument");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    int rc;
    if (rows == ROWS_BF16 && (rc = fm_bf16_need_snapshot(f))) return rc;
    FmStore* st;
    if ((rc = fm_fit_store(f, which, &st))) return rc;
    if ((rc = fm_fit_forward(f, *st, rows))) return rc;
    HIPCHK(hipMemcpyAsync(out, f->d_out, (size_t)st->n * 4, hipMemcpyDeviceToHost, m->stream));
    return check_device_error(m);
}

static int fm_eval_binary_resident(tfr_fm* f, FwdRows rows, int64_t* neq_out, double* nll_sum_out, double* auc_out,
                                   int64_t* n_out) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    int rc;
    if (rows == ROWS_BF16 && (rc = fm_bf16_need_snapshot(f))) return rc;
    FmStore* st;
    if ((rc = fm_fit_store(f, 1, &st))) return rc;
    if (m->o.loss != TFR_LOSS_NLL) return fail(TFR_ERR_STATE, "eval_binary needs the binary-outcome model (loss = nll)");
    if (n_out) *n_out = st->n;
    if ((rc = fm_fit_forward(f, *st, rows))) return rc;
    const int nblk = fm_metrics_grid(st->n);
    HIPCHK(f->fit->met.reserve((int64_t)nblk * 2, m->stream));
    launch_fm_binary_metrics(f->d_out, st->y, st->n, f->fit->met, m->stream);
    HIPCHK(hipGetLastError());
    std::vector<float> part((size_t)nblk * 2);
    HIPCHK(hipMemcpyAsync(part.data(), f->fit->met, part.size() * 4, hipMemcpyDeviceToHost, m->stream));
    if ((rc = check_device_error(m))) return rc;
    double nll = 0.0;
    int64_t neq = 0;
    for (int b = 0; b < nblk; ++b) {                     // as eval_device sums the forward's partials
        neq += (int64_t)llround((double)part[(size_t)b * 2]);
        nll += (double)part[(size_t)b * 2 + 1];
    }
    if (neq_out) *neq_out = neq;
    if (nll_sum_out) *nll_sum_out = nll;
    return auc_device(m, f->d_out, st->y, st->n, auc_out);
}

extern "C" {

int tfr_fm_predict_resident(tfr_fm* f, int32_t which, float* out) { return fm_predict_resident(f, ROWS_F32, which, out); }

/* tfr_eval_binary_resident for the FM: accuracy count, summed sigmoid cross-entropy and AUC over the eval store */
int tfr_fm_eval_binary_resident(tfr_fm* f, int64_t* neq_out, double* nll_sum_out, double* auc_out, int64_t* n_out) {
    return fm_eval_binary_resident(f, ROWS_F32, neq_out, nll_sum_out, auc_out, n_out);
}

/* the same two from the bf16 snapshot (fm_bf16.h): TFR_ERR_STATE before tfr_fm_bf16_snapshot, whatever the stores hold */
int tfr_fm_bf16_predict_resident(tfr_fm* f, int32_t which, float* out) { return fm_predict_resident(f, ROWS_BF16, which, out); }

int tfr_fm_bf16_eval_binary_resident(tfr_fm* f, int64_t* neq_out, double* nll_sum_out, double* auc_out, int64_t* n_out) {
    return fm_eval_binary_resident(f, ROWS_BF16, neq_out, nll_sum_out, auc_out, n_out);
}

}  // extern "C"
