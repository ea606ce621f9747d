// neighbours_api.inc.h - the tfr_*neighbours* entry points (include/tfrecomm.h), compiled inside api.hip beside
// the top-K entries whose staging buffers, exclusion check, error flag and merge they share.
//
// A query on the model's stream:
//   k_row_rnorm        cosine only, and only when the table's cached rn is stale (nb_rnorm) or its rows are rebuilt per call
//   k_topk_check_excl  the device entry's exclusion check (launch_topk_check_excl, row ids against R)
//   per chunk of query rows: k_nb_score over the candidate slices -> k_topk_merge (launch_topk_merge)

struct NbTable {
    const float* T; int64_t R; int32_t item_abs;
    int cache;                                           // slot of m->nb_rn that holds this table's rn
    bool fleeting;                                       // the rows are rebuilt per call (SVD++ peff): so is rn, every query
};

static const char* const NB_WHO = "neighbours";

static int nb_svd_table(tfr_model* m, int32_t which, NbTable* t) {
    if (which == TFR_NB_ITEMS) *t = {m->w[TFR_Q], m->I, m->o.item_abs, 0, false};
    else if (which == TFR_NB_USERS) *t = {m->w[TFR_P], m->U, 0, 1, false};
    else return fail(TFR_ERR_ARG, "%s: table must be TFR_NB_ITEMS or TFR_NB_USERS (got %d)", NB_WHO, which);
    return TFR_OK;
}

static int nb_check_args(const NbTable& t, int32_t metric, int64_t n, int32_t k, int64_t lo, int64_t hi) {
    if (n < 0) return fail(TFR_ERR_ARG, "%s: negative n", NB_WHO);
    if (k < 1 || k > TOPK_KMAX) return fail(TFR_ERR_ARG, "%s: k must be in [1, %d] (got %d)", NB_WHO, TOPK_KMAX, k);
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

// one chunk of query rows, all pointers on the device: scoring (candidate slices) -> merge into ids / scores
static int nb_chunk(tfr_model* m, const NbTable& t, const float* rn, const NbPlan& p, const int32_t* d_rows, int64_t rows,
                    int32_t k, const int64_t* d_indptr, const int32_t* d_excl, int64_t lo, int64_t hi, int32_t* d_ids,
                    float* d_scores) {
    HIPCHK(m->tk_part.reserve(pow2_cap(rows * p.slices * k), m->stream));
    NbArgs a;
    memset(&a, 0, sizeof(a));
    a.T = t.T; a.rn = rn; a.rows = d_rows; a.indptr = d_indptr; a.excl = d_excl; a.excl_bad = m->tk_bad;
    a.part = m->tk_part; a.err = m->d_err;
    a.n_rows = rows; a.R = t.R; a.lo = lo; a.hi = hi;
    a.D = m->D; a.k = k; a.slices = p.slices; a.item_abs = t.item_abs;
    launch_nb_score(a, p, m->stream);
    HIPCHK(hipGetLastError());
    TopkMergeArgs g;
    memset(&g, 0, sizeof(g));
    g.part = m->tk_part; g.items_out = d_ids; g.scores_out = d_scores; g.n_rows = rows; g.k = k; g.slices = p.slices;
    launch_topk_merge(g, m->stream);
    HIPCHK(hipGetLastError());
    return TFR_OK;
}

// the host entries: ids and the exclusion CSR are checked here, before any device work; then chunk by chunk staged, scored,
// merged and copied back (the staging buffers of topk_host).  Outputs are written only when every check passed.
static int nb_host(tfr_model* m, const NbTable& t, const float* rn, const int32_t* rows, int64_t n, int32_t k,
                   const int64_t* indptr, const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out, float* scores_out) {
    int rc;
    NbPlan p;
    if (!nb_plan(k, n, hi - lo, &p)) return fail(TFR_ERR_ARG, "%s: no plan for k %d", NB_WHO, k);
    HIPCHK(m->tk_bad.reserve(1, m->stream));
    HIPCHK(hipMemsetAsync(m->tk_bad, 0, sizeof(int32_t), m->stream));
    HIPCHK(m->tk_users.reserve(pow2_cap(p.chunk), m->stream));
    HIPCHK(m->tk_items.reserve(pow2_cap(p.chunk * k), m->stream));
    if (scores_out) HIPCHK(m->tk_scores.reserve(pow2_cap(p.chunk * k), m->stream));
    std::vector<int64_t> rebased;
    for (int64_t c0 = 0; c0 < n; c0 += p.chunk) {
        const int64_t nr = n - c0 < p.chunk ? n - c0 : p.chunk;
        HIPCHK(hipMemcpyAsync(m->tk_users, rows + c0, (size_t)nr * 4, hipMemcpyHostToDevice, m->stream));
        const int64_t* d_ip = nullptr;
        const int32_t* d_ex = nullptr;
        if (indptr) {
            const int64_t e0 = indptr[c0], nnz = indptr[c0 + nr] - e0;
            rebased.resize((size_t)nr + 1);
            for (int64_t r = 0; r <= nr; ++r) rebased[(size_t)r] = indptr[c0 + r] - e0;
            HIPCHK(m->tk_indptr.reserve(pow2_cap(nr + 1), m->stream));
            if (nnz > 0) HIPCHK(m->tk_excl.reserve(pow2_cap(nnz), m->stream));
            HIPCHK(hipMemcpyAsync(m->tk_indptr, rebased.data(), (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, m->stream));
            if (nnz > 0) HIPCHK(hipMemcpyAsync(m->tk_excl, excl + e0, (size_t)nnz * 4, hipMemcpyHostToDevice, m->stream));
            d_ip = m->tk_indptr;
            d_ex = m->tk_excl;
        }
        if ((rc = nb_chunk(m, t, rn, p, m->tk_users, nr, k, d_ip, d_ex, lo, hi, m->tk_items, scores_out ? m->tk_scores : nullptr)))
            return rc;
        HIPCHK(hipMemcpyAsync(ids_out + c0 * k, m->tk_items, (size_t)nr * k * 4, hipMemcpyDeviceToHost, m->stream));
        if (scores_out)
            HIPCHK(hipMemcpyAsync(scores_out + c0 * k, m->tk_scores, (size_t)nr * k * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));         // the staged inputs are rewritten by the next chunk
    }
    return check_device_error(m);
}

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

// the device entry: every pointer on the device, the exclusion CSR checked there; no synchronisation
static int nb_dev(tfr_model* m, const NbTable& t, const float* rn, const int32_t* d_rows, int64_t n, int32_t k,
                  const int64_t* d_indptr, const int32_t* d_excl, int64_t lo, int64_t hi, int32_t* d_ids_out, float* d_scores_out) {
    int rc;
    NbPlan p;
    if (!nb_plan(k, n, hi - lo, &p)) return fail(TFR_ERR_ARG, "%s: no plan for k %d", NB_WHO, k);
    HIPCHK(m->tk_bad.reserve(1, m->stream));
    HIPCHK(hipMemsetAsync(m->tk_bad, 0, sizeof(int32_t), m->stream));
    if (d_indptr) {
        launch_topk_check_excl(d_indptr, d_excl, n, t.R, m->tk_bad, m->d_err, m->stream);
        HIPCHK(hipGetLastError());
    }
    for (int64_t c0 = 0; c0 < n; c0 += p.chunk) {
        const int64_t nr = n - c0 < p.chunk ? n - c0 : p.chunk;
        if ((rc = nb_chunk(m, t, rn, p, d_rows + c0, nr, k, d_indptr ? d_indptr + c0 : nullptr, d_excl, lo, hi,
                           d_ids_out + c0 * k, d_scores_out ? d_scores_out + c0 * k : nullptr)))
            return rc;
    }
    return TFR_OK;
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

extern "C" {

int tfr_neighbours_plan(int32_t dim, int32_t k, int64_t n, int64_t n_candidates, int64_t* lds_bytes, int32_t* rows_per_block,
                        int32_t* slices, int64_t* row_chunk) {
    int G, VEC;
    if (!geometry(dim, &G, &VEC)) return fail(TFR_ERR_ARG, "unsupported dim %d", dim);
    if (n < 0 || n_candidates < 1) return fail(TFR_ERR_ARG, "%s plan: n >= 0 and n_candidates >= 1", NB_WHO);
    NbPlan p;
    if (!nb_plan(k, n, n_candidates, &p)) return fail(TFR_ERR_ARG, "%s: k must be in [1, %d] (got %d)", NB_WHO, TOPK_KMAX, k);
    if (lds_bytes) *lds_bytes = (int64_t)(p.lds_score > p.lds_merge ? p.lds_score : p.lds_merge);
    if (rows_per_block) *rows_per_block = p.upb;
    if (slices) *slices = p.slices;
    if (row_chunk) *row_chunk = p.chunk;
    return TFR_OK;
}

int tfr_neighbours(tfr_model* m, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                   const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out, float* scores_out) {
    MODEL_ENTER(m);
    NbTable t;
    int rc = nb_svd_table(m, which, &t);
    if (rc || (rc = nb_host_checks(t, metric, rows, n, k, excl_indptr, excl, lo, hi, ids_out)) || n == 0) return rc;
    const float* rn;
    if ((rc = settle_q(m)) || (rc = nb_rnorm(m, t, metric, &rn))) return rc;
    return nb_host(m, t, rn, rows, n, k, excl_indptr, excl, lo, hi, ids_out, scores_out);
}

int tfr_neighbours_dev(tfr_model* m, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                       const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi, int32_t* d_ids_out,
                       float* d_scores_out) {
    MODEL_ENTER(m);
    NbTable t;
    int rc = nb_svd_table(m, which, &t);
    if (rc || (rc = nb_dev_checks(t, metric, d_rows, n, k, d_excl_indptr, d_excl, lo, hi, d_ids_out)) || n == 0) return rc;
    const float* rn;
    if ((rc = settle_q(m)) || (rc = nb_rnorm(m, t, metric, &rn))) return rc;
    return nb_dev(m, t, rn, d_rows, n, k, d_excl_indptr, d_excl, lo, hi, d_ids_out, d_scores_out);
}

int tfr_svdpp_neighbours(tfr_svdpp* h, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                         const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi, int32_t* ids_out,
                         float* scores_out) {
    PP_ENTER(h);
    NbTable t;
    int rc = nb_pp_table(h, which, &t);
    if (rc || (rc = nb_host_checks(t, metric, rows, n, k, excl_indptr, excl, lo, hi, ids_out)) || n == 0) return rc;
    if (which == TFR_NB_USERS && (rc = pp_peff_all(h))) return rc;
    const float* rn;
    if ((rc = settle_q(m)) || (rc = nb_rnorm(m, t, metric, &rn))) return rc;
    return nb_host(m, t, rn, rows, n, k, excl_indptr, excl, lo, hi, ids_out, scores_out);
}

int tfr_svdpp_neighbours_dev(tfr_svdpp* h, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                             const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi, int32_t* d_ids_out,
                             float* d_scores_out) {
    PP_ENTER(h);
    NbTable t;
    int rc = nb_pp_table(h, which, &t);
    if (rc || (rc = nb_dev_checks(t, metric, d_rows, n, k, d_excl_indptr, d_excl, lo, hi, d_ids_out)) || n == 0) return rc;
    if (which == TFR_NB_USERS && (rc = pp_peff_all(h))) return rc;
    const float* rn;
    if ((rc = settle_q(m)) || (rc = nb_rnorm(m, t, metric, &rn))) return rc;
    return nb_dev(m, t, rn, d_rows, n, k, d_excl_indptr, d_excl, lo, hi, d_ids_out, d_scores_out);
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
    return nb_host(m, t, rn, features, n, k, excl_indptr, excl, lo, hi, ids_out, scores_out);
}

}  // extern "C"
