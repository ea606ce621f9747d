// puresvd.h - PureSVD (tfr_psvd_*): the constants, the launch plan, the argument blocks of the kernels and the
// handle.  puresvd.hip owns the kernels and the C-ABI entries; the CSR, its transpose, the checks and the handle's base are
// item_lists.h's; the Gram S = Z^T Z is ials.hip's (ials_model.h ials_launch_gram), every dense product ease.hip's
// k_ease_gemm (ease.h ease_launch_gemm); long lists are cut by als_common.h plan_chunks and carried by tfr::ChunkArgs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "tfrecomm.h"
#include "devbuf.h"
#include "als_common.h"
#include "ials_model.h"
#include "item_lists.h"

constexpr int PSVD_MAX_R = 128;                          // widest block: factors + oversample
// A wave's adds are one chain, so its time is its list's length times the latency of a group of loads: the longest list
// ends the launch.  Measured at the ML-1M shape, r = 80: chunk 2048 / ahead 8 left X^T W at 0.349 ms beside
// 0.044 ms for X V, whose longest row is a few hundred entries.
constexpr int PSVD_CHUNK = 256;                          // list entries one wave adds; longer lists are cut (a multiple of 64)
constexpr int PSVD_AHEAD = 16;                           // list entries whose rows a wave has in flight before the first add
constexpr int PSVD_WAVES = 4;                            // waves per block of k_psvd_spmm
constexpr int PSVD_SWEEP_CAP = 30;                       // Jacobi sweeps; the last allowed one must not rotate
constexpr int PSVD_DENSE_THREADS = 512;                  // the one workgroup of k_psvd_chol and k_psvd_jacobi
constexpr int64_t PSVD_LDS_MAX = 160 * 1024;             // LDS of a gfx950 workgroup
// a pivot must exceed this times its column's own diagonal entry of S: below it the column is a combination of the earlier
// ones to within the rounding of r <= 128 products (r eps = 2.8e-14), which is what r > rank X looks like in float64
constexpr double PSVD_PIVOT_REL = 0x1p-44;
// a Jacobi rotation is made where |t_pq| exceeds this times the largest |entry| of T as given
constexpr double PSVD_ROT_REL = 0x1p-52;
static_assert(PSVD_CHUNK % 64 == 0 && 64 % PSVD_AHEAD == 0, "a chunk is whole loads of 64 ids, a load whole groups of PSVD_AHEAD");

constexpr int psvd_ld(int r) { return r + 1; }           // LDS row stride of an r x r matrix: odd, so a column walk spreads the banks
constexpr int64_t psvd_mat_lds(int r) { return (int64_t)r * psvd_ld(r) * 8; }
// the rotations sit in LDS beside T where both fit
constexpr bool psvd_rot_in_lds(int r) { return 2 * psvd_mat_lds(r) + 4096 <= PSVD_LDS_MAX; }
constexpr int64_t psvd_jacobi_lds(int r) { return (psvd_rot_in_lds(r) ? 2 : 1) * psvd_mat_lds(r) + 4096; }
constexpr int64_t psvd_jacobi_lds_max() {
    int64_t most = 0;
    for (int r = 1; r <= PSVD_MAX_R; ++r) most = psvd_jacobi_lds(r) > most ? psvd_jacobi_lds(r) : most;
    return most;
}
static_assert(psvd_jacobi_lds_max() <= PSVD_LDS_MAX, "T must fit in LDS at every width");

struct PsvdPlan {
    int32_t r, lanes, chunk, ahead, sweep_cap, rot_in_lds;  // lanes: 64, a whole wave per row at every width (two columns per lane)
    int64_t gram_slices;                                 // slices of the Gram partial buffer a fit reserves, r * r doubles each
    int64_t lds;                                         // largest LDS of the fit's launches
    int64_t device_bytes;                                // float64 buffers of a fit, the lists and chunk sums aside
};

// Slices the ALS Gram launches write for n rows.  Not monotonic in n: gram_slice_rows stays at 128 up to 131072 rows (1024
// slices) and grows in steps of 32 past it (131073 rows: 820 slices), so a buffer for two sides takes the larger count.
inline int64_t psvd_gram_slices(int64_t n) { return (n + gram_slice_rows(n) - 1) / gram_slice_rows(n); }
inline int64_t psvd_gram_slices(int64_t n_users, int64_t n_items) { return std::max(psvd_gram_slices(n_users), psvd_gram_slices(n_items)); }

inline bool psvd_plan(int64_t n_users, int64_t n_items, int factors, int oversample, PsvdPlan* p) {
    if (n_users < 1 || n_items < 1 || factors < 1 || oversample < 0) return false;
    const int64_t r = (int64_t)factors + oversample;
    if (r > PSVD_MAX_R) return false;
    p->r = (int32_t)r;
    p->lanes = 64;
    p->chunk = PSVD_CHUNK;
    p->ahead = PSVD_AHEAD;
    p->sweep_cap = PSVD_SWEEP_CAP;
    p->rot_in_lds = psvd_rot_in_lds((int)r) ? 1 : 0;
    p->lds = psvd_jacobi_lds((int)r);
    const int64_t slices = p->gram_slices = psvd_gram_slices(n_users, n_items);
    // V and Z [I, r], W [U, r], Q [I, f], P [U, f], the Gram slices' partials, six r x r matrices
    p->device_bytes = (2 * n_items * r + n_users * r + (n_items + n_users) * factors + slices * r * r + 6 * r * r) * 8;
    return true;
}

// out[e, :] = the sum, in list order, of in[ids[t], :] over t in [ptr[e], ptr[e + 1]); r columns, row stride r on both sides
struct PsvdSpmmArgs {
    const int64_t* ptr; const int32_t* ids;
    const double* in; double* out;
    int64_t n;                                           // rows of out
    int32_t r;
};

struct PsvdCholArgs {
    const double* S;                                     // [r, r] symmetric
    double* R; double* Rinv;                             // out [r, r] upper triangular, zeros below
    int32_t* err;                                        // 0, or 1 + the first refused column; a word that is set ends the kernel
    int32_t r;
};

struct PsvdJacobiArgs {
    const double* T;                                     // [r, r] symmetric
    double* rot;                                         // [r, r] scratch: the rotations where they do not fit in LDS
    double* lambda; double* Q;                           // out [r] descending, [r, r] eigenvectors in columns
    int32_t* sweeps;                                     // out: sweeps run, the clean last one included; cap + 1: not converged
    int32_t r, rot_in_lds;
};

struct tfr_psvd : tfr::ItemListModel {
    int32_t factors = 0, r = 0;
    bool has_ritz = false;
    int32_t n_sweeps = 0;
    int64_t fold_n = -1;                                 // rows of the last fold-in; -1 before any
    std::vector<double> sigma, ritz;                     // [factors], [r] on the host
    hipEvent_t ev[2] = {nullptr, nullptr};             // bracket one stage of a fit at a time
    tfr::DevChunks chunks[2];                            // the long lists of the users' rows and of the items' lists
    tfr::DevBuf<double> partial[2];                      // their chunk sums [chunks, width]
    tfr::DevBuf<double> bi[2], bu;                       // [I, r] x 2 (V and Z, by turns), [U, r]
    tfr::DevBuf<double> Q, P;                            // [I, factors], [U, factors]
    tfr::DevBuf<double> gram_partial, small;             // the Gram slices; S, R, Rinv, T, Qe, rot [6][r, r], lambda [r], norms [r]
    tfr::DevBuf<double> blk_in, blk_out;                 // multiply / orthonormalise / residuals: a call's own blocks
    tfr::DevBuf<int32_t> err;                            // [2]: the pivot word, the sweep count
    // fold-in: the last call's chunk plan and rows (its lists are staged in q_ptr / q_ids)
    tfr::DevChunks fold_chunks;
    tfr::DevBuf<double> fold_partial, fold;
};
