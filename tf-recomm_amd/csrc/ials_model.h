// ials_model.h - the implicit-ALS handle and the one argument block of its kernels, shared by the Cholesky path (ials.hip)
// and the conjugate-gradient path (ials_cg.hip).  ials.hip owns the C-ABI entries, the Gram and the loss's last kernel; a
// handle with cg_steps > 0 was made by tfr_ials_create_cg and its half-sweeps and per-user loss go through the two queue_*
// functions below.  Fold-in (tfr_ials_fold_in, ials.hip) gives the same kernels an argument block built from a call's own
// lists: its buffers and its chunk plan are the handle's fold_* members, apart from everything a sweep reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tfrecomm.h"
#include "devbuf.h"
#include "als_common.h"

constexpr int IALS_TILE = 32;                // partner rows staged per LDS tile
constexpr int IALS_CG_MAXD = 256;            // widest table of the conjugate-gradient path
constexpr int64_t IALS_GRAM_ROWS = 128;      // smallest Gram slice
constexpr int64_t IALS_GRAM_SLICES = 1024;   // most Gram slices: bounds the partial buffer at 1024 d^2 doubles

// rows per Gram slice: a function of n alone, a multiple of the tile
__host__ __device__ inline int64_t gram_slice_rows(int64_t n) {
    const int64_t per = (n + IALS_GRAM_SLICES - 1) / IALS_GRAM_SLICES;
    const int64_t rows = (per + IALS_TILE - 1) / IALS_TILE * IALS_TILE;
    return rows < IALS_GRAM_ROWS ? IALS_GRAM_ROWS : rows;
}

struct tfr_ials {
    int64_t n[2] = {0, 0};                               // users, items
    int32_t d = 0;
    int32_t cg_steps = 0;                                // 0: the Cholesky path; > 0: that many CG steps per row
    double lambda = 0.0, alpha = 0.0;
    int device = 0;
    bool loaded = false;
    hipStream_t stream = nullptr;
    tfr::DevBuf<double> tab[2];                          // X [n_users, d], Y [n_items, d]
    // side z: the lists of its entities (side 0: the CSR as given; side 1: its transpose, each list by ascending user)
    tfr::DevBuf<int64_t> ptr[2];
    tfr::DevBuf<int32_t> ids[2];
    tfr::DevBuf<double> vals[2];
    tfr::DevChunks chunks[2];
    tfr::DevBuf<double> partial, G, gram_partial, per_user, loss;
    // Which side's table the Gram in G belongs to, or -1.  Every Gram sets it; whatever may change that side's table
    // (tfr_ials_set, a half-sweep of the side, a fold-in that writes rows of it) clears it.  Only fold-in reads it.
    int gram_of = -1;
    // fold-in: the last call's lists, its chunk plan with the chunks' partial sums, its rows [fold_n, d] and where they went
    tfr::DevBuf<int64_t> fold_ptr;
    tfr::DevBuf<int32_t> fold_ids, fold_rows;
    tfr::DevBuf<double> fold_vals, fold_partial, fold;
    tfr::DevChunks fold_chunks;
    int64_t fold_n = -1;                                 // rows of the last fold-in; -1 before any
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// what every kernel of both paths sees of one side
struct IalsArgs {
    int64_t n;                                                     // entities of this side, empty ones included
    const int64_t* ptr; const int32_t* ids; const double* vals;    // their lists: partner ids, values
    double* own; const double* other; const double* G;             // G = other^T other
    double lambda, alpha;
    int32_t d, cg_steps;
};

namespace tfr {
inline IalsArgs ials_side_args(const tfr_ials* m, int side) {
    return IalsArgs{m->n[side], m->ptr[side].get(), m->ids[side].get(), m->vals[side].get(), m->tab[side].get(),
                    m->tab[1 - side].get(), m->G.get(), m->lambda, m->alpha, m->d, m->cg_steps};
}
// queued on the model's stream; each returns hipGetLastError() after its launches
hipError_t ials_cg_queue_fit(const IalsArgs& a, hipStream_t s); // a.cg_steps steps for every entity of the block, from a.G
hipError_t ials_cg_queue_loss_users(tfr_ials* m);              // m->per_user, from m->G = Y^T Y
// The Gram launches of ials.hip for another family (PureSVD: puresvd.hip): G [d, d] = T^T T of T [n, d], d <= 256,
// in the slice order of gram_slice_rows(n); partial holds ceil(n / gram_slice_rows(n)) * d * d doubles.
void ials_launch_gram(const double* T, int64_t n, int d, double* partial, double* G, hipStream_t s);
}  // namespace tfr
