// svdpp_api.inc.h - the tfr_svdpp entry points (include/tfrecomm.h), compiled inside api.hip: a tfr_svdpp wraps a
// tfr_model and shares its internals (batch workspace, radix sort, error flag, step bookkeeping, top-K / rank launchers).
//
// A step on the model's stream:
//   radix sort of the batch by user and by item (ids checked: a bad id sets the flag and every later kernel returns)
//   k_pp_mark        stamp the user runs (stamp[u] = this call's number, run_of[u] = the run's head)
//   k_pp_ypart       per piece of N of an active user: sum of Y rows and of their squares
//   k_pp_users       per user run: z_u, peff[u] = P[u] + z_u, logits, g, W_u, c_u, the user side's update, per-run scalars
//   k_pp_items       per item run: the item side's gradient from peff and g, and its update
//   k_pp_ygrad       per piece of NT: the Y gradient of its active users
//   k_pp_yapply      per Y row: the pieces in order, then the update
//   k_finalize       {loss, reg, sum g} over the per-run scalars in position order, the bias_global update
#include "svdpp.h"

struct tfr_svdpp {
    tfr_model* m = nullptr;
    DevBuf<float> Y, Ym, Yv;                             // [I, D] and its Adam slots
    DevBuf<float> peff;                                  // [U, D], rows of the users of the last call
    DevBuf<int32_t> stamp, run_of;                       // [U]
    int32_t cur = 0;                                     // number of the last activation (stamp[] starts at 0)
    // N and its transpose, each with its pieces
    DevBuf<int64_t> n_ip, t_ip;
    DevBuf<int32_t> n_idx, t_idx, n_pbeg, n_prow, t_pbeg, t_prow;
    int64_t nnz = 0, n_pieces = 0, t_pieces = 0;
    bool have_n = false;
    DevBuf<float> part, part_sq, gpart;
    DevBuf<int32_t> gcnt;
    // per batch position: W at run heads, run sizes, per-run scalars
    DevBuf<float> W, scal;
    DevBuf<int32_t> cnt;
    int64_t wcap = 0;
    uint32_t frozen = 0;
};

#define PP_ENTER(h)                                                   \
    if (!(h)) return fail(TFR_ERR_ARG, "null model");                 \
    tfr_model* m = (h)->m;                                            \
    HIPCHK(hipSetDevice(m->device));

static int pp_need_n(const tfr_svdpp* h) {
    return h->have_n ? TFR_OK : fail(TFR_ERR_STATE, "SVD++: the implicit sets are not set (tfr_svdpp_set_implicit)");
}

static int pp_table(tfr_svdpp* h, int32_t which, float** p, int64_t* n) {
    if ((which & 7) != TFR_Y) return table_ptr(h->m, which, p, n);
    if ((which & ~(7 | TFR_SLOT_M | TFR_SLOT_V)) || ((which & TFR_SLOT_M) && (which & TFR_SLOT_V)))
        return fail(TFR_ERR_ARG, "bad table id %d", which);
    float* q = (which & TFR_SLOT_M) ? h->Ym.get() : (which & TFR_SLOT_V) ? h->Yv.get() : h->Y.get();
    if (!q) return fail(TFR_ERR_STATE, "table %d has no such slot (optimizer is not Adam)", which);
    *p = q;
    *n = h->m->I * h->m->D;
    return TFR_OK;
}

// the per-position buffers of a B-entry step
static int pp_ensure_batch(tfr_svdpp* h, int64_t B) {
    tfr_model* m = h->m;
    int rc = ensure_capacity(m, B > 0 ? B : 1);
    if (rc) return rc;
    if (m->cap > h->wcap) {
        HIPCHK(h->W.reserve(m->cap * m->D, m->stream));
        HIPCHK(h->scal.reserve(m->cap * 4, m->stream));
        HIPCHK(h->cnt.reserve(m->cap, m->stream));
        h->wcap = m->cap;
    }
    return TFR_OK;
}

static PpArgs pp_args(tfr_svdpp* h) {
    tfr_model* m = h->m;
    PpArgs a;
    memset(&a, 0, sizeof(a));
    a.P = m->w[TFR_P]; a.bu = m->w[TFR_BU]; a.Q = m->w[TFR_Q]; a.bi = m->w[TFR_BI]; a.mu = m->w[TFR_MU];
    a.Pm = m->m[TFR_P]; a.Pv = m->v[TFR_P]; a.bum = m->m[TFR_BU]; a.buv = m->v[TFR_BU];
    a.Qm = m->m[TFR_Q]; a.Qv = m->v[TFR_Q]; a.bim = m->m[TFR_BI]; a.biv = m->v[TFR_BI];
    a.Y = h->Y; a.Ym = h->Ym; a.Yv = h->Yv;
    a.N = {h->n_ip, h->n_idx, h->n_pbeg, h->n_prow, m->U, h->n_pieces};
    a.NT = {h->t_ip, h->t_idx, h->t_pbeg, h->t_prow, m->I, h->t_pieces};
    a.peff = h->peff; a.part = h->part; a.part_sq = h->part_sq;
    a.W = h->W; a.cnt = h->cnt; a.gpart = h->gpart; a.gcnt = h->gcnt; a.scal = h->scal;
    a.err = m->d_err;
    a.U = m->U; a.I = m->I; a.D = m->D;
    a.loss = m->o.loss; a.item_abs = m->o.item_abs; a.reg_bias = m->o.reg_bias;
    a.frozen = h->frozen; a.lam = m->o.reg;
    return a;
}

// sort n ids by user (and, with di, by item; both columns checked against the tables) and stamp the user runs
static int pp_activate(tfr_svdpp* h, PpArgs& a, const int32_t* du, const int32_t* di, int64_t n) {
    tfr_model* m = h->m;
    int rc;
    {
        Prof p(m, TFR_K_SORT);
        if ((rc = sort_model_columns(m, du, di, n, true))) return rc;
    }
    if (h->cur == 0x7fffffff) {                          // the numbers wrap: start the stamps afresh
        HIPCHK(hipMemsetAsync(h->stamp, 0, (size_t)m->U * 4, m->stream));
        h->cur = 0;
    }
    h->cur += 1;
    a.act = {m->ks_u, m->ps_u, h->stamp, h->run_of, h->cur, n};
    a.ks_i = m->ks_i; a.ps_i = m->ps_i;
    a.B = n;
    launch_pp_mark(a.act, m->d_err, m->stream);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// peff rows (and, for a forward, the logits) of the n users du
static int pp_front(tfr_svdpp* h, PpArgs& a, const int32_t* du, const int32_t* di, int64_t n, int mode) {
    int rc = pp_activate(h, a, du, di, n);
    if (rc) return rc;
    {
        Prof p(h->m, TFR_K_FORWARD);
        launch_pp_ypart(a, h->m->stream);
        launch_pp_users(a, mode, h->m->stream);
    }
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

static int pp_forward(tfr_svdpp* h, const int32_t* du, const int32_t* di, int64_t B, float* d_logits) {
    int rc = pp_need_n(h);
    if (rc || (rc = pp_ensure_batch(h, B))) return rc;
    PpArgs a = pp_args(h);
    a.u = du; a.it = di; a.logits = d_logits;
    return pp_front(h, a, du, di, B, PP_USERS_FORWARD);
}

// one step; out4 (device, may be NULL) receives {loss, reg, sum g, error flag}
static int pp_train(tfr_svdpp* h, const int32_t* du, const int32_t* di, const float* dr, int64_t B, float* d_logits,
                    float* out4) {
    tfr_model* m = h->m;
    const OptStep k = opt_step(m);
    if (k.tf1) return fail(TFR_ERR_STATE, "SVD++ training supports SGD and lazy Adam (not tf1 Adam)");
    int rc = pp_need_n(h);
    if (rc || (rc = pp_ensure_batch(h, B))) return rc;
    hipStream_t s = m->stream;
    PpArgs a = pp_args(h);
    a.u = du; a.it = di; a.r = dr; a.logits = d_logits; a.g = m->d_g;
    a.opt = k.adam ? 0 : 1;
    set_hyper(a, k);
    if (B > 0) {
        if ((rc = pp_activate(h, a, du, di, B))) return rc;
        {
            Prof p(m, TFR_K_FORWARD);
            launch_pp_ypart(a, s);
            launch_pp_users(a, PP_USERS_TRAIN, s);
        }
        {
            Prof p(m, TFR_K_REDUCE_ITEM);
            launch_pp_items(a, s);
        }
        {
            Prof p(m, TFR_K_APPLY);
            launch_pp_y(a, s);
        }
        HIPCHK(hipGetLastError());
    }
    FinArgs f = mu_fin(m, k, !((h->frozen >> TFR_MU) & 1), out4);
    f.partials = h->scal; f.nblk = (int32_t)B; f.out_err = out4 ? 1 : 0;
    {
        Prof p(m, TFR_K_FINALIZE);
        launch_finalize(f, s);
    }
    HIPCHK(hipGetLastError());
    advance_step(m);
    return TFR_OK;
}

// host CSR of N(u) -> pieces of a CSR of `rows` rows: pbeg [rows + 1], prow [pieces]
static int pp_pieces(const std::vector<int64_t>& ip, int64_t rows, std::vector<int32_t>& pbeg, std::vector<int32_t>& prow) {
    pbeg.assign((size_t)rows + 1, 0);
    int64_t np = 0;
    for (int64_t r = 0; r < rows; ++r) {
        pbeg[(size_t)r] = (int32_t)np;
        np += (ip[(size_t)r + 1] - ip[(size_t)r] + PP_PIECE - 1) / PP_PIECE;
        if (np > 0x7fffffffLL) return fail(TFR_ERR_ARG, "SVD++: the implicit sets have too many entries");
    }
    pbeg[(size_t)rows] = (int32_t)np;
    prow.resize((size_t)np);
    for (int64_t r = 0; r < rows; ++r)
        for (int32_t p = pbeg[(size_t)r]; p < pbeg[(size_t)r + 1]; ++p) prow[(size_t)p] = (int32_t)r;
    return TFR_OK;
}

template <typename T>
static int pp_upload(DevBuf<T>& d, const std::vector<T>& v, hipStream_t s) {
    HIPCHK(d.reserve(v.empty() ? 1 : (int64_t)v.size(), s));
    if (!v.empty()) HIPCHK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return TFR_OK;
}

// the entries that check user ids on the host first (top-K, rank): peff for the n users, staged in m->d_u
static int pp_peff_host(tfr_svdpp* h, const char* who, const int32_t* users, int64_t n) {
    int rc = pp_need_n(h);
    if (rc || (rc = check_ids(who, "user id", users, n, h->m->U))) return rc;
    if ((rc = pp_ensure_batch(h, n))) return rc;
    tfr_model* m = h->m;
    HIPCHK(hipMemcpyAsync(m->d_u, users, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    PpArgs a = pp_args(h);
    return pp_front(h, a, m->d_u, nullptr, n, PP_USERS_PEFF);
}

static TopkTables pp_topk_tables(const tfr_svdpp* h) {
    TopkTables t = svd_topk_tables(h->m);
    t.P = h->peff;
    return t;
}

extern "C" {

const char* tfr_svdpp_last_error(void) { return g_err; }

int tfr_svdpp_destroy(tfr_svdpp* h) {
    if (!h) return TFR_OK;
    tfr_model* m = h->m;
    if (m) {
        (void)hipSetDevice(m->device);
        (void)hipStreamSynchronize(m->stream);
    }
    delete h;                                            // the SVD++ buffers go first, under the wrapped model's device
    return tfr_destroy(m);
}

int tfr_svdpp_create(tfr_svdpp** out, int64_t U, int64_t I, int32_t D, const tfr_opts* opts) {
    if (!out) return fail(TFR_ERR_ARG, "out is null");
    *out = nullptr;
    tfr_model* m = nullptr;
    int rc = tfr_create(&m, U, I, D, opts);
    if (rc) return rc;
    tfr_svdpp* h = new (std::nothrow) tfr_svdpp();
    if (!h) {
        tfr_destroy(m);
        return fail(TFR_ERR_NOMEM, "host allocation failed");
    }
    h->m = m;
    hipStream_t s = m->stream;
    hipError_t e = h->Y.reserve(I * D, s);
    if (e == hipSuccess) e = h->peff.reserve(U * D, s);
    if (e == hipSuccess) e = h->stamp.reserve(U, s);
    if (e == hipSuccess) e = h->run_of.reserve(U, s);
    if (e == hipSuccess && opts->optimizer == TFR_OPT_ADAM) {
        e = h->Ym.reserve(I * D, s);
        if (e == hipSuccess) e = h->Yv.reserve(I * D, s);
        if (e == hipSuccess) e = hipMemsetAsync(h->Ym, 0, (size_t)I * D * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(h->Yv, 0, (size_t)I * D * 4, s);
    }
    if (e == hipSuccess) e = hipMemsetAsync(h->Y, 0, (size_t)I * D * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->peff, 0, (size_t)U * D * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->stamp, 0, (size_t)U * 4, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        rc = fail(e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP, "SVD++ tables: %s", hipGetErrorString(e));
        char keep[512];
        strncpy(keep, g_err, sizeof(keep));
        tfr_svdpp_destroy(h);
        strncpy(g_err, keep, sizeof(g_err));
        return rc;
    }
    *out = h;
    return TFR_OK;
}

int tfr_svdpp_set_table(tfr_svdpp* h, int32_t which, const float* host, int64_t n) {
    PP_ENTER(h);
    float* p; int64_t cnt;
    int rc = pp_table(h, which, &p, &cnt);
    if (rc) return rc;
    if (!host || n != cnt) return fail(TFR_ERR_ARG, "table %d expects %lld floats, got %lld", which, (long long)cnt, (long long)n);
    m->tab_gen += 1;
    HIPCHK(hipMemcpyAsync(p, host, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_svdpp_get_table(tfr_svdpp* h, int32_t which, float* host, int64_t n) {
    PP_ENTER(h);
    float* p; int64_t cnt;
    int rc = pp_table(h, which, &p, &cnt);
    if (rc) return rc;
    if (!host || n != cnt) return fail(TFR_ERR_ARG, "table %d holds %lld floats, asked %lld", which, (long long)cnt, (long long)n);
    HIPCHK(hipMemcpyAsync(host, p, (size_t)n * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_svdpp_init(tfr_svdpp* h, uint64_t seed, float fstd, float bstd) {
    PP_ENTER(h);
    int rc = tfr_init_tables(m, seed, fstd, bstd);
    if (rc) return rc;
    const int64_t n = m->I * m->D;
    launch_init_trunc_normal(h->Y, n, fstd, seed * 4 + 0x9e3779b97f4a7c15ull, m->stream);   // apart from the four SVD streams
    HIPCHK(hipGetLastError());
    if (h->Ym) HIPCHK(hipMemsetAsync(h->Ym, 0, (size_t)n * 4, m->stream));
    if (h->Yv) HIPCHK(hipMemsetAsync(h->Yv, 0, (size_t)n * 4, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_svdpp_set_implicit(tfr_svdpp* h, const int64_t* indptr, const int32_t* items) {
    PP_ENTER(h);
    const int64_t U = m->U, I = m->I;
    if (!indptr) return fail(TFR_ERR_ARG, "SVD++ implicit sets: null indptr");
    if (indptr[0] != 0) return fail(TFR_ERR_ARG, "SVD++ implicit sets: indptr must start at 0");
    if (indptr[U] > 0 && !items) return fail(TFR_ERR_ARG, "SVD++ implicit sets: null items");
    int rc = check_csr("SVD++ implicit sets", true, indptr, items, U, I);
    if (rc) return rc;
    const int64_t nnz = indptr[U];
    std::vector<int64_t> nip(indptr, indptr + U + 1), tip((size_t)I + 1, 0);
    std::vector<int32_t> nidx(items, items + nnz), tidx((size_t)nnz);
    for (int64_t e = 0; e < nnz; ++e) tip[(size_t)items[e] + 1] += 1;
    for (int64_t j = 0; j < I; ++j) tip[(size_t)j + 1] += tip[(size_t)j];
    {
        std::vector<int64_t> fill(tip.begin(), tip.end() - 1);
        for (int64_t u = 0; u < U; ++u)                  // users ascending: every column of the transpose is ascending
            for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) tidx[(size_t)fill[(size_t)items[e]]++] = (int32_t)u;
    }
    std::vector<int32_t> npb, npr, tpb, tpr;
    if ((rc = pp_pieces(nip, U, npb, npr)) || (rc = pp_pieces(tip, I, tpb, tpr))) return rc;
    hipStream_t s = m->stream;
    h->have_n = false;
    HIPCHK(hipStreamSynchronize(s));                     // nothing in flight still reads the old sets
    if ((rc = pp_upload(h->n_ip, nip, s)) || (rc = pp_upload(h->n_idx, nidx, s)) || (rc = pp_upload(h->n_pbeg, npb, s)) ||
        (rc = pp_upload(h->n_prow, npr, s)) || (rc = pp_upload(h->t_ip, tip, s)) || (rc = pp_upload(h->t_idx, tidx, s)) ||
        (rc = pp_upload(h->t_pbeg, tpb, s)) || (rc = pp_upload(h->t_prow, tpr, s)))
        return rc;
    h->nnz = nnz;
    h->n_pieces = (int64_t)npr.size();
    h->t_pieces = (int64_t)tpr.size();
    const int64_t pn = h->n_pieces > 0 ? h->n_pieces : 1, pt = h->t_pieces > 0 ? h->t_pieces : 1;
    HIPCHK(h->part.reserve(pn * m->D, s));
    HIPCHK(h->part_sq.reserve(pn, s));
    HIPCHK(h->gpart.reserve(pt * m->D, s));
    HIPCHK(h->gcnt.reserve(pt, s));
    HIPCHK(hipStreamSynchronize(s));                     // the host vectors go out of scope
    h->have_n = true;
    return TFR_OK;
}

int tfr_svdpp_set_frozen(tfr_svdpp* h, uint32_t mask) {
    PP_ENTER(h);
    if (mask & ~0x3fu) return fail(TFR_ERR_ARG, "SVD++ frozen mask: bits 0..5 only");
    h->frozen = mask;
    return tfr_set_frozen(m, mask & 0x1fu);
}

int tfr_svdpp_set_hyper(tfr_svdpp* h, float lr, float reg) {
    if (!h) return fail(TFR_ERR_ARG, "null model");
    return tfr_set_hyper(h->m, lr, reg);
}

int tfr_svdpp_get_step(tfr_svdpp* h, int64_t* step, float* b1p, float* b2p) {
    if (!h) return fail(TFR_ERR_ARG, "null model");
    return tfr_get_step(h->m, step, b1p, b2p);
}

int tfr_svdpp_set_step(tfr_svdpp* h, int64_t step, float b1p, float b2p) {
    if (!h) return fail(TFR_ERR_ARG, "null model");
    return tfr_set_step(h->m, step, b1p, b2p);
}

int tfr_svdpp_get_stream(tfr_svdpp* h, void** s) {
    if (!h) return fail(TFR_ERR_ARG, "null model");
    return tfr_get_stream(h->m, s);
}

int tfr_svdpp_sync(tfr_svdpp* h) {
    PP_ENTER(h);
    return check_device_error(m);
}

int tfr_svdpp_forward_dev(tfr_svdpp* h, const int32_t* du, const int32_t* di, int64_t B, float* d_logits) {
    PP_ENTER(h);
    int rc = check_batch(du, di, B);
    if (rc) return rc;
    if (B == 0) return pp_need_n(h);
    if (!d_logits) return fail(TFR_ERR_ARG, "null logits pointer");
    return pp_forward(h, du, di, B, d_logits);
}

int tfr_svdpp_forward(tfr_svdpp* h, const int32_t* u, const int32_t* i, int64_t B, float* logits_out) {
    PP_ENTER(h);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (B == 0) return pp_need_n(h);
    if (!logits_out) return fail(TFR_ERR_ARG, "null logits pointer");
    if ((rc = pp_need_n(h)) || (rc = pp_ensure_batch(h, B))) return rc;
    HIPCHK(hipMemcpyAsync(m->d_u, u, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->d_i, i, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    if ((rc = pp_forward(h, m->d_u, m->d_i, B, m->d_logits))) return rc;
    HIPCHK(hipMemcpyAsync(logits_out, m->d_logits, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    return check_device_error(m);
}

int tfr_svdpp_eval(tfr_svdpp* h, const int32_t* u, const int32_t* i, const float* r, int64_t B, double* sse_out,
                   int64_t* neq_out) {
    PP_ENTER(h);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (sse_out) *sse_out = 0.0;
    if (neq_out) *neq_out = 0;
    if (B == 0) return pp_need_n(h);
    if (!r) return fail(TFR_ERR_ARG, "null rate pointer");
    std::vector<float> x((size_t)B);
    if ((rc = tfr_svdpp_forward(h, u, i, B, x.data()))) return rc;
    double sse = 0.0;
    int64_t neq = 0;
    for (int64_t k = 0; k < B; ++k) {                    // infer = the head: the logit (mse) or round(sigmoid) (nll)
        const double y = m->o.loss == TFR_LOSS_MSE ? (double)x[(size_t)k] : nearbyint(1.0 / (1.0 + exp(-(double)x[(size_t)k])));
        const double d = y - (double)r[k];
        sse += d * d;
        neq += y == (double)r[k];
    }
    if (sse_out) *sse_out = sse;
    if (neq_out) *neq_out = neq;
    return TFR_OK;
}

int tfr_svdpp_train_step_dev(tfr_svdpp* h, const int32_t* du, const int32_t* di, const float* dr, int64_t B,
                             float* d_logits) {
    PP_ENTER(h);
    int rc = check_batch(du, di, B);
    if (rc) return rc;
    if (B > 0 && !dr) return fail(TFR_ERR_ARG, "null rate pointer");
    return pp_train(h, du, di, dr, B, d_logits, nullptr);
}

int tfr_svdpp_train_step(tfr_svdpp* h, const int32_t* u, const int32_t* i, const float* r, int64_t B, float* logits_out,
                         float* loss_out, float* reg_out) {
    PP_ENTER(h);
    int rc = check_batch(u, i, B);
    if (rc) return rc;
    if (B > 0 && !r) return fail(TFR_ERR_ARG, "null rate pointer");
    if ((rc = pp_ensure_batch(h, B))) return rc;
    const StepMark mark = mark_step(m);
    if (B > 0) {
        HIPCHK(hipMemcpyAsync(m->d_u, u, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->d_i, i, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->d_r, r, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    }
    float* out4 = m->d_logits + B;                       // [logits | loss, reg, sum g, error flag]: cap + 4 floats
    if ((rc = pp_train(h, m->d_u, m->d_i, m->d_r, B, m->d_logits, out4))) return rc;
    std::vector<float> back((size_t)B + 4);
    HIPCHK(hipMemcpyAsync(back.data(), m->d_logits, back.size() * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    const int32_t e = (int32_t)back[(size_t)B + 3];
    if (e) {                                             // a bad batch never advances the step
        rollback_step(m, mark);
        return device_error(m, e);
    }
    if (logits_out && B > 0) memcpy(logits_out, back.data(), (size_t)B * 4);
    if (loss_out) *loss_out = back[(size_t)B];
    if (reg_out) *reg_out = back[(size_t)B + 1];
    return TFR_OK;
}

int tfr_svdpp_topk(tfr_svdpp* h, const int32_t* users, int64_t n, int32_t k, const int64_t* excl_indptr,
                   const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    PP_ENTER(h);
    if (n < 0) return fail(TFR_ERR_ARG, "top-K: negative n_users");
    if (int rc = check_k("top-K", k)) return rc;
    if (n == 0) return pp_need_n(h);
    if (!users || !items_out) return fail(TFR_ERR_ARG, "top-K: null users / items_out");
    if (excl_indptr && !excl_items && excl_indptr[n] > excl_indptr[0]) return fail(TFR_ERR_ARG, "top-K: exclusion indptr without items");
    int rc;
    if (excl_indptr && (rc = check_csr("top-K", false, excl_indptr, excl_items, n, m->I))) return rc;
    if ((rc = pp_peff_host(h, "top-K", users, n))) return rc;
    return topk_host(m, pp_topk_tables(h), users, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_svdpp_topk_dev(tfr_svdpp* h, const int32_t* d_users, int64_t n, int32_t k, const int64_t* d_excl_indptr,
                       const int32_t* d_excl_items, int32_t* d_items_out, float* d_scores_out) {
    PP_ENTER(h);
    if (n < 0) return fail(TFR_ERR_ARG, "top-K: negative n_users");
    int rc = check_k("top-K", k);
    if (rc) return rc;
    rc = pp_need_n(h);
    if (rc || n == 0) return rc;
    if (!d_users || !d_items_out) return fail(TFR_ERR_ARG, "top-K: null users / items_out");
    if ((rc = pp_ensure_batch(h, n))) return rc;
    PpArgs a = pp_args(h);
    if ((rc = pp_front(h, a, d_users, nullptr, n, PP_USERS_PEFF))) return rc;
    return topk_dev(m, pp_topk_tables(h), d_users, n, k, d_excl_indptr, d_excl_items, d_items_out, d_scores_out);
}

int tfr_svdpp_rank_items(tfr_svdpp* h, const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
                         const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    PP_ENTER(h);
    if (n < 0) return fail(TFR_ERR_ARG, "rank: negative n_users");
    if (n == 0) return pp_need_n(h);
    if (!users || !tgt_indptr) return fail(TFR_ERR_ARG, "rank: null users / target indptr");
    if (tgt_indptr[n] > tgt_indptr[0] && (!tgt_items || !ranks_out)) return fail(TFR_ERR_ARG, "rank: null target items / ranks_out");
    if (excl_indptr && !excl_items && excl_indptr[n] > excl_indptr[0]) return fail(TFR_ERR_ARG, "rank: exclusion indptr without items");
    int rc = check_csr("rank", true, tgt_indptr, tgt_items, n, m->I);
    if (rc || (excl_indptr && (rc = check_csr("rank", false, excl_indptr, excl_items, n, m->I)))) return rc;
    if ((rc = pp_peff_host(h, "rank", users, n))) return rc;
    return rank_host(m, pp_topk_tables(h), users, n, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

}  // extern "C"
