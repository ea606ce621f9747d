// neighbours_api.inc.h - the tfr_*neighbours* entry points (include/tfrecomm.h), compiled inside api.hip beside
// the top-K entries whose driver (sliced_host / sliced_dev: plan, staging buffers, exclusion check, error flag, merge) they run.
//
// A query on the model's stream:
//   k_row_rnorm        cosine only, and only when the table's cached rn is stale (nb_rnorm) or its rows are rebuilt per call
//                      (k_row_rnorm_bf16 for a table of the bf16 snapshot, whose rn lives and dies with the snapshot)
//   k_topk_check_excl  the device entry's exclusion check (launch_topk_check_excl, row ids against R)
//   per chunk of query rows: k_nb_score (k_nb_score_bf16) over the candidate slices -> k_topk_merge (launch_topk_merge)

struct NbTable {
    const float* T; int64_t R; int32_t item_abs;
    int cache;                                           // slot of m->nb_rn that holds this table's rn
    bool fleeting;                                       // the rows are rebuilt per call (SVD++ peff): so is rn, every query
    const uint16_t* B = nullptr;                         // set: the table is this one of the bf16 snapshot (stride DP), T is not read
};

static const char* const NB_WHO = "neighbours";

static int nb_svd_table(tfr_model* m, int32_t which, NbTable* t) {
    if (which == TFR_NB_ITEMS) *t = {m->w[TFR_Q], m->I, m->o.item_abs, 0, false};
    else if (which == TFR_NB_USERS) *t = {m->w[TFR_P], m->U, 0, 1, false};
    else return fail(TFR_ERR_ARG, "%s: table must be TFR_NB_ITEMS or TFR_NB_USERS (got %d)", NB_WHO, which);
    return TFR_OK;
}

// the snapshot's tables (tfr_bf16_neighbours*): the same rows, counts and item_abs, read from the bf16 copy alone
static int nb_bf16_table(tfr_model* m, int32_t which, NbTable* t) {
    const int rc = nb_svd_table(m, which, t);
    if (rc) return rc;
    t->T = nullptr;
    t->B = which == TFR_NB_ITEMS ? m->bf.q : m->bf.p;
    return TFR_OK;
}

static int nb_check_args(const NbTable& t, int32_t metric, int64_t n, int32_t k, int64_t lo, int64_t hi) {
    if (n < 0) return fail(TFR_ERR_ARG, "%s: negative n", NB_WHO);
    if (int rc = check_k(NB_WHO, k)) return rc;
    if (metric != TFR_NB_DOT && metric != TFR_NB_COSINE)
        return fail(TFR_ERR_ARG, "%s: metric must be TFR_NB_DOT or TFR_NB_COSINE (got %d)", NB_WHO, metric);
    if (lo < 0 || hi <= lo || hi > t.R)
        return fail(TFR_ERR_ARG, "%s: candidate range [%lld, %lld) not inside [0, %lld)", NB_WHO, (long long)lo, (long long)hi,
                    (long long)t.R);
    return TFR_OK;
}

// The inverse norms of table t, for the cosine form (NULL for dot).  A cached slot is valid while the step counter and the
// table generation it was built at still hold and no table pointer has left the library; anything else rebuilds it - one
// read of the table, in stream order before the scoring that uses it.
static int nb_rnorm(tfr_model* m, const NbTable& t, int32_t metric, const float** rn) {
    *rn = nullptr;
    if (metric != TFR_NB_COSINE) return TFR_OK;
    if (t.B) {                                           // the snapshot changes only by tfr_bf16_snapshot / tfr_bf16_drop
        tfr_model::Bf16Snap::Rn& c = m->bf.rn[t.cache];
        if (!c.valid || c.gen != m->bf.gen) {
            c.valid = false;
            HIPCHK(c.rn.reserve(t.R, m->stream));
            launch_row_rnorm_bf16(t.B, t.R, bf16_row_stride(m->D), c.rn, m->stream);
            HIPCHK(hipGetLastError());
            c.gen = m->bf.gen; c.valid = true;
        }
        *rn = c.rn;
        return TFR_OK;
    }
    tfr_model::RnCache& c = m->nb_rn[t.cache];
    if (!c.valid || c.step != m->step || c.gen != m->tab_gen || m->tab_exposed || t.fleeting) {
        c.valid = false;
        HIPCHK(c.rn.reserve(t.R, m->stream));
        launch_row_rnorm(t.T, t.R, m->D, c.rn, m->stream);
        HIPCHK(hipGetLastError());
        c.step = m->step; c.gen = m->tab_gen; c.valid = !t.fleeting;
    }
    *rn = c.rn;
    return TFR_OK;
}

// a query for the driver: table t, rn of nb_rnorm, candidates [lo, hi).  The callers settle the item rows, before rn is built.
struct NbQuery : SlicedQuery {
    NbTable t; const float* rn; int64_t lo, hi;
    NbQuery(const NbTable& t_, const float* rn_, int64_t lo_, int64_t hi_)
        : SlicedQuery{NB_WHO, t_.R, hi_ - lo_, t_.item_abs, false}, t(t_), rn(rn_), lo(lo_), hi(hi_) {}
    void score(const SlicedArgs& c, const TopkPlan& p, hipStream_t s) const {
        NbArgs a = {};
        static_cast<SlicedArgs&>(a) = c;
        a.T = t.T; a.rn = rn; a.R = t.R; a.lo = lo; a.hi = hi;
        launch_nb_score(a, p, s);
    }
};

// the same query on a table of the bf16 snapshot, which was settled when it was made
struct Bf16NbQuery : SlicedQuery {
    NbTable t; const float* rn; int64_t lo, hi; int32_t DP;
    Bf16NbQuery(const NbTable& t_, const float* rn_, int64_t lo_, int64_t hi_, int32_t DP_)
        : SlicedQuery{NB_WHO, t_.R, hi_ - lo_, t_.item_abs, false}, t(t_), rn(rn_), lo(lo_), hi(hi_), DP(DP_) {}
    void score(const SlicedArgs& c, const TopkPlan& p, hipStream_t s) const {
        Bf16NbArgs a = {};
        static_cast<SlicedArgs&>(a) = c;
        a.T = t.B; a.rn = rn; a.R = t.R; a.lo = lo; a.hi = hi; a.DP = DP;
        launch_bf16_nb_score(a, p, s);
    }
};

// what the host entries check before any device work
static int nb_host_checks(const NbTable& t, int32_t metric, const int32_t* rows, int64_t n, int32_t k, const int64_t* indptr,
                          const int32_t* excl, int64_t lo, int64_t hi, const int32_t* ids_out) {
    int rc = nb_check_args(t, metric, n, k, lo, hi);
    if (rc || n == 0) return rc;
    if (!rows || !ids_out) return fail(TFR_ERR_ARG, "%s: null rows / ids_out", NB_WHO);
    if (indptr && !excl && indptr[n] > indptr[0]) return fail(TFR_ERR_ARG, "%s: exclusion indptr without rows", NB_WHO);
    if ((rc = check_ids(NB_WHO, "row id", rows, n, t.R))) return rc;
    return indptr ? check_csr(NB_WHO, false, indptr, excl, n, t.R) : TFR_OK;
}

static int nb_dev_checks(const NbTable& t, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k, const int64_t* d_indptr,
                         const int32_t* d_excl, int64_t lo, int64_t hi, const int32_t* d_ids_out) {
    int rc = nb_check_args(t, metric, n, k, lo, hi);
    if (rc || n == 0) return rc;
    if (!d_rows || !d_ids_out) return fail(TFR_ERR_ARG, "%s: null rows / ids_out", NB_WHO);
    if (d_indptr && !d_excl) return fail(TFR_ERR_ARG, "%s: exclusion indptr without rows", NB_WHO);
    return TFR_OK;
}

// SVD++ users: e_u = P[u] + z_u for every user (peff holds the rows of the users of the last call only), staged through m->d_u
static int pp_peff_all(tfr_svdpp* h) {
    tfr_model* m = h->m;
    int rc = pp_need_n(h);
    if (rc || (rc = pp_ensure_batch(h, m->U))) return rc;
    std::vector<int32_t> all((size_t)m->U);
    for (int64_t u = 0; u < m->U; ++u) all[(size_t)u] = (int32_t)u;
    HIPCHK(hipMemcpyAsync(m->d_u, all.data(), (size_t)m->U * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));             // `all` leaves scope
    PpArgs a = pp_args(h);
    return pp_front(h, a, m->d_u, nullptr, m->U, PP_USERS_PEFF);
}

// the SVD++ table of a query: items as the SVD model, users the effective rows
static int nb_pp_table(tfr_svdpp* h, int32_t which, NbTable* t) {
    int rc = nb_svd_table(h->m, which, t);
    if (rc || which != TFR_NB_USERS) return rc;
    t->T = h->peff;
    t->fleeting = true;
    return TFR_OK;
}

template <class Query>
static int nb_drive(tfr_model* m, const Query& q, bool dev, const int32_t* rows, int64_t n, int32_t k, const int64_t* indptr,
                    const int32_t* excl, int32_t* ids_out, float* scores_out) {
    return dev ? sliced_dev(m, q, rows, n, k, indptr, excl, ids_out, scores_out)
               : sliced_host(m, q, rows, n, k, indptr, excl, ids_out, scores_out);
}

// an SVD / SVD++ entry once its table is named: checks -> (SVD++ users: e_u of every user) -> settle -> rn -> the driver.
// dev: every pointer is on the device.  h is NULL for the SVD model.  A snapshot table is not settled: nothing of the
// float32 tables is read.
static int nb_run(tfr_model* m, tfr_svdpp* h, const NbTable& t, bool dev, int32_t metric, const int32_t* rows, int64_t n,
                  int32_t k, const int64_t* indptr, const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out,
                  float* scores_out) {
    int rc = dev ? nb_dev_checks(t, metric, rows, n, k, indptr, excl, lo, hi, ids_out)
                 : nb_host_checks(t, metric, rows, n, k, indptr, excl, lo, hi, ids_out);
    if (rc || n == 0) return rc;
    if (h && t.fleeting && (rc = pp_peff_all(h))) return rc;
    const float* rn;
    if ((!t.B && (rc = settle_q(m))) || (rc = nb_rnorm(m, t, metric, &rn))) return rc;
    if (t.B) return nb_drive(m, Bf16NbQuery(t, rn, lo, hi, bf16_row_stride(m->D)), dev, rows, n, k, indptr, excl, ids_out, scores_out);
    return nb_drive(m, NbQuery(t, rn, lo, hi), dev, rows, n, k, indptr, excl, ids_out, scores_out);
}

extern "C" {

int tfr_neighbours_plan(int32_t dim, int32_t k, int64_t n, int64_t n_candidates, int64_t* lds_bytes, int32_t* rows_per_block,
                        int32_t* slices, int64_t* row_chunk) {
    return sliced_plan_entry(NB_WHO, "n >= 0 and n_candidates >= 1", dim, k, n, n_candidates, lds_bytes, rows_per_block, slices,
                             row_chunk);
}

int tfr_neighbours(tfr_model* m, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                   const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out, float* scores_out) {
    MODEL_ENTER(m);
    NbTable t;
    const int rc = nb_svd_table(m, which, &t);
    return rc ? rc : nb_run(m, nullptr, t, false, metric, rows, n, k, excl_indptr, excl, lo, hi, ids_out, scores_out);
}

int tfr_neighbours_dev(tfr_model* m, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                       const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi, int32_t* d_ids_out,
                       float* d_scores_out) {
    MODEL_ENTER(m);
    NbTable t;
    const int rc = nb_svd_table(m, which, &t);
    return rc ? rc : nb_run(m, nullptr, t, true, metric, d_rows, n, k, d_excl_indptr, d_excl, lo, hi, d_ids_out, d_scores_out);
}

// the snapshot test comes before every other check, n == 0 included, as in the other tfr_bf16_* entries
int tfr_bf16_neighbours(tfr_model* m, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                        const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out,
                        float* scores_out) {
    MODEL_ENTER(m);
    int rc = bf16_need_snapshot(m);
    if (rc) return rc;
    NbTable t;
    rc = nb_bf16_table(m, which, &t);
    return rc ? rc : nb_run(m, nullptr, t, false, metric, rows, n, k, excl_indptr, excl, lo, hi, ids_out, scores_out);
}

int tfr_bf16_neighbours_dev(tfr_model* m, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                            const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi, int32_t* d_ids_out,
                            float* d_scores_out) {
    MODEL_ENTER(m);
    int rc = bf16_need_snapshot(m);
    if (rc) return rc;
    NbTable t;
    rc = nb_bf16_table(m, which, &t);
    return rc ? rc : nb_run(m, nullptr, t, true, metric, d_rows, n, k, d_excl_indptr, d_excl, lo, hi, d_ids_out, d_scores_out);
}

int tfr_svdpp_neighbours(tfr_svdpp* h, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                         const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out,
                         float* scores_out) {
    PP_ENTER(h);
    NbTable t;
    const int rc = nb_pp_table(h, which, &t);
    return rc ? rc : nb_run(m, h, t, false, metric, rows, n, k, excl_indptr, excl, lo, hi, ids_out, scores_out);
}

int tfr_svdpp_neighbours_dev(tfr_svdpp* h, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                             const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi, int32_t* d_ids_out,
                             float* d_scores_out) {
    PP_ENTER(h);
    NbTable t;
    const int rc = nb_pp_table(h, which, &t);
    return rc ? rc : nb_run(m, h, t, true, metric, d_rows, n, k, d_excl_indptr, d_excl, lo, hi, d_ids_out, d_scores_out);
}

int tfr_fm_neighbours(tfr_fm* f, int32_t metric, const int32_t* features, int64_t n, int32_t k, const int64_t* excl_indptr,
                      const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out, float* scores_out) {
    if (!f) return fail(TFR_ERR_ARG, "null model");
    tfr_model* m = f->m;
    HIPCHK(hipSetDevice(m->device));
    const NbTable t = {m->w[TFR_P], m->U, 0, 1, false};  // V is the wrapped model's user side
    int rc = nb_host_checks(t, metric, features, n, k, excl_indptr, excl, lo, hi, ids_out);
    if (rc || n == 0) return rc;
    const float* rn;
    if ((rc = nb_rnorm(m, t, metric, &rn))) return rc;
    return sliced_host(m, NbQuery(t, rn, lo, hi), features, n, k, excl_indptr, excl, ids_out, scores_out);
}

}  // extern "C"
