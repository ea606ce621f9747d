// svdpp.h - SVD++ (Koren's implicit-feedback factor model) on gfx950: argument blocks and launchers shared by svdpp.hip and
// the tfr_svdpp entry points (svdpp_api.inc.h).  DESIGN §14.
//
// The implicit set N(u) is a CSR [U, I] with strictly increasing rows, resident on the device twice: user-major (N) and
// item-major (NT, the transpose).  Both are cut into pieces of at most PP_PIECE entries, a row's pieces consecutive, so a
// long row or a hot column is summed by several waves and the owning wave adds the piece partials in piece order.
// Pieces depend on N only, never on the batch or the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

constexpr int PP_PIECE = 128;                          // entries of N (or NT) per piece
constexpr int PP_WAVES = 4;                            // independent waves per block (no block barrier in any kernel)

// a CSR cut into pieces: piece p covers entries [ip[row[p]] + (p - pbeg[row[p]]) * PP_PIECE, ...) of its row
struct PpCsr {
    const int64_t* ip; const int32_t* idx;             // [rows + 1], [nnz]
    const int32_t* pbeg; const int32_t* prow;          // [rows + 1] first piece of each row, [n_pieces] row of each piece
    int64_t rows, n_pieces;
};

// the active set of a call: the runs of a sorted user column (a run = one user, its head = its first sorted position).
// stamp[u] == cur marks u active in this call and run_of[u] is its head; nothing is cleared between calls.
struct PpActive {
    const int32_t* ks; const int32_t* ps;              // sorted user ids, their batch positions
    int32_t* stamp; int32_t* run_of;
    int32_t cur;
    int64_t n;                                         // sorted entries
};

struct PpArgs {
    // tables (the wrapped model's) and Y with its slots
    float* P; float* bu; float* Q; float* bi; const float* mu;
    float *Pm, *Pv, *bum, *buv, *Qm, *Qv, *bim, *biv;
    float* Y; float* Ym; float* Yv;
    PpCsr N, NT;
    PpActive act;
    const int32_t* ks_i; const int32_t* ps_i;          // the batch sorted by item
    const int32_t* u; const int32_t* it; const float* r;
    float* peff;                                       // [U, D] P[u] + z_u, rows of the active users
    float* part; float* part_sq;                       // [N pieces, D], [N pieces]: sum of Y rows / of their squares
    float* W; int32_t* cnt;                            // [B, D], [B] at run heads: s_u sum_k g_k Q'[i_k], entries of the run
    float* gpart; int32_t* gcnt;                       // [NT pieces, D], [NT pieces]: Y gradient / occurrences per piece
    float* logits; float* g;                           // [B]
    float* scal;                                       // [2B, 4] {loss, reg, sum g, -}: user heads then item heads
    int32_t* err;
    int64_t B, U, I;
    int32_t D, loss, item_abs, reg_bias, opt;          // opt: 0 lazy Adam, 1 SGD
    uint32_t frozen;                                   // bits TFR_MU..TFR_Q, bit 5 = Y
    float lam, alpha, b1, b2, eps, lr;
};

enum { PP_USERS_PEFF = 0, PP_USERS_FORWARD = 1, PP_USERS_TRAIN = 2 };

// stamp the runs of act (heads only); entries past a failed id check do nothing
void launch_pp_mark(const PpActive& a, const int32_t* err, hipStream_t s);
// per piece of an active user: sum of Y rows (ascending j) and of their squared norms
void launch_pp_ypart(const PpArgs& a, hipStream_t s);
// per run: z_u from the piece partials in piece order, peff = P + z; then the forward or the user side of a step
void launch_pp_users(const PpArgs& a, int mode, hipStream_t s);
// per item run of the batch: Q / item_bias gradient from peff and g, in run order, and their update
void launch_pp_items(const PpArgs& a, hipStream_t s);
// per NT piece: sum over its active users (ascending) of W_u + lam c_u Y[j]; then per item the pieces in order and the update
void launch_pp_y(const PpArgs& a, hipStream_t s);

}  // namespace tfr
