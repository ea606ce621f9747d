// ease.h - EASE (tfr_ease_*): the launch plan, the argument blocks of the kernels and the handle.  ease.hip owns
// the kernels and the C-ABI entries; the CSR, the serving drivers, the count loop, the per-wave key queue and the scoring tail
// are item_lists.h's; the per-slice key lists are merged by topk.hip's launch_topk_merge (topk.h).
//
// Fit: G = X^T X + lambda I in float64 (k_ease_gram, on item_lists.h count_row), P = G^-1 by a blocked Cholesky in
// place on the lower triangle (k_ease_diag factors and inverts one EASE_NB block in LDS, k_ease_gemm is every O(n^3)
// stage), B = -P / diag(P) in float32 (k_ease_weights).  Scoring: one wave per (query, slice of EASE_W columns) adds the
// query's rows of B in registers, four waves per block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tfrecomm.h"
#include "devbuf.h"
#include "topk.h"
#include "item_lists.h"

constexpr int64_t EASE_MAX_ITEMS = 32768;                // the dense cap: 8 + 4 bytes per entry = 12 GiB there
constexpr int EASE_KMAX = tfr::TOPK_KMAX;
constexpr int EASE_NB = 64;                              // factorisation block: the diagonal block one workgroup holds in LDS
constexpr int EASE_TILE = 64;                            // C tile of one k_ease_gemm workgroup (4 waves x 16 rows x 64 columns)
constexpr int EASE_KC = 16;                              // k extent of one staged chunk: four v_mfma_f64_16x16x4_f64 steps
constexpr int EASE_LDT = EASE_TILE + 16;                 // LDS row stride (doubles): rows k and k + 1 fall on the two bank halves
constexpr int EASE_LDD = EASE_NB + 1;                    // LDS row stride of the diagonal block's two copies
constexpr int EASE_W_GRAM = 16384;                       // counters per Gram block: 64 KiB
constexpr int EASE_WAVES = 4;                            // waves per block of the Gram and scoring kernels
constexpr int EASE_W = 1024;                             // columns per scoring wave: 16 accumulators per lane
constexpr int EASE_COLS = EASE_W / 64;
constexpr int EASE_AHEAD = 4;                            // list items whose rows of B a scoring wave loads ahead
constexpr int EASE_SCORE_CAP = 512;                      // keys per scoring wave's queue
constexpr int64_t EASE_CHUNK_MAX = 65536;                // queries per chunk
constexpr int EASE_GRID_ROWS = 8192;                     // Gram grid: rows past this are taken in strides
static_assert(EASE_NB == EASE_TILE, "the triangular stages skip whole tiles: blocks and tiles share their edges");
static_assert(EASE_MAX_ITEMS / EASE_W * EASE_KMAX <= tfr::TOPK_MERGE_KEYS, "the cap must be servable at every k");

constexpr size_t ease_gemm_lds() { return (size_t)2 * EASE_KC * EASE_LDT * 8; }
constexpr size_t ease_diag_lds() { return (size_t)2 * EASE_NB * EASE_LDD * 8; }
constexpr size_t ease_gram_lds() { return (size_t)EASE_W_GRAM * 4; }
constexpr size_t ease_score_lds() { return (size_t)EASE_WAVES * EASE_W * 4 + (size_t)EASE_WAVES * EASE_SCORE_CAP * 8; }

struct EasePlan {
    int32_t nb, tile, blocks;                            // fit: block size, update tile, diagonal blocks
    int32_t width, slices, ahead;                        // scoring (which = 1) or Gram (which = 0) slicing
    int64_t chunk;                                       // queries per chunk
    size_t lds;                                          // largest static LDS of the launches of `which`
    int64_t f64_bytes, f32_bytes;                        // device bytes of a fit: G / P, work panel and inverted blocks; B
};

// false: what a launch would refuse.  which 0: the fit (k and n_rows are not used); which 1: scoring n_rows queries for k.
inline bool ease_plan(int which, int64_t n_items, int k, int64_t n_rows, EasePlan* p) {
    if (which < 0 || which > 1 || n_items < 1 || n_items > EASE_MAX_ITEMS || n_rows < 0) return false;
    if (which == 1 && (k < 1 || k > EASE_KMAX)) return false;
    p->nb = EASE_NB;
    p->tile = EASE_TILE;
    p->blocks = (int32_t)((n_items + EASE_NB - 1) / EASE_NB);
    p->f64_bytes = (n_items * n_items + (int64_t)EASE_NB * n_items + (int64_t)p->blocks * EASE_NB * EASE_NB) * 8;
    p->f32_bytes = n_items * n_items * 4;
    p->width = which ? EASE_W : EASE_W_GRAM;
    const int64_t s = (n_items + p->width - 1) / p->width;
    p->slices = (int32_t)s;
    p->ahead = which ? EASE_AHEAD : 64;
    p->chunk = 1;
    if (which == 0) {
        p->lds = ease_gram_lds() > ease_diag_lds() ? ease_gram_lds() : ease_diag_lds();
        return true;
    }
    if (s > tfr::TOPK_MAX_SLICES || s * k > tfr::TOPK_MERGE_KEYS) return false;
    p->lds = ease_score_lds();
    int64_t chunk = n_rows < 1 ? 1 : n_rows > EASE_CHUNK_MAX ? EASE_CHUNK_MAX : n_rows;
    const int64_t by_part = tfr::TOPK_PART_BYTES / (s * k * 8);
    if (chunk > by_part) chunk = by_part;
    p->chunk = chunk < 1 ? 1 : chunk;
    return true;
}

struct EaseGramArgs {
    const int64_t* pu; const int32_t* items;             // the user rows, each strictly increasing
    const int64_t* pi; const int32_t* iu;                // the item lists (users ascending)
    double* G;                                           // out [n_items, n_items]
    int64_t n_items;
    double lambda;
};

// C (M x N) = beta * C + sign * op(A) (M x K) * op(B) (K x N), row-major with the given row strides.
struct EaseGemmArgs {
    const double* A; const double* B; double* C;
    int64_t lda, ldb, ldc;
    int32_t M, N, K;
    int32_t ta, tb;                                      // op(A)[m][k] = ta ? A[k * lda + m] : A[m * lda + k]; op(B) alike
    int32_t sign, beta;                                  // sign +1 / -1; beta 0 (C is not read) / 1
    int32_t lower;                                       // 1: tiles right of the diagonal are skipped (M = N, C symmetric)
    int32_t kskip;                                       // 1: op(B) is lower triangular by whole tiles: k starts at the tile's column
};

struct EaseDiagArgs {
    double* G; int64_t ld;                               // the matrix; block [j, j + b) of its diagonal
    double* W;                                           // out [EASE_NB, EASE_NB]: the inverse of the block's factor, zero elsewhere
    int32_t* err;                                        // 0, or 1 + the first column whose pivot was not positive and finite
    int32_t j, b;
};

struct EaseScoreArgs {
    const int32_t* users;                                // NULL: query q is row q of (ptr, ids); else row users[q]
    const int64_t* ptr; const int32_t* ids;              // the query lists, each strictly increasing
    const float* B;                                      // [n_items, n_items]
    const int64_t* xptr; const int32_t* xids;            // exclusion rows aligned with the queries; xptr may be NULL
    const int64_t* tptr; const int32_t* tids;            // target rows aligned with the queries (ranking)
    uint64_t* part;                                      // top-K: out [n, slices, k] keys of queries q_lo .. q_lo + n
    uint64_t* tkeys; int32_t* ranks;                     // ranking: per target its key (0 = unranked) and its rank
    int64_t q_lo, n, n_items;
    int32_t k, slices;
};

// The launches another dense item x item family shares with EASE (SLIM: slim.hip); the kernels stay ease.hip's.
// k_ease_gram over `slices` column slices of EASE_W_GRAM (ease_plan(0).slices); k_ease_score<mode> for a.n * a.slices waves.
void ease_launch_gram(const EaseGramArgs& a, int32_t slices, hipStream_t s);
// k_ease_gemm over the tiles of C, for a dense float64 product of another family (PureSVD: puresvd.hip)
void ease_launch_gemm(const EaseGemmArgs& g, hipStream_t s);
void ease_launch_score(int mode, const EaseScoreArgs& a, hipStream_t s);

struct tfr_ease : tfr::ItemListModel {
    double lambda = 0.0;
    int f64_is = 0;                                      // what the f64 buffer holds: 0 nothing, 1 G, 2 P
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    float gram_ms = 0.f;                                 // device time of the tfr_ease_gram that built the matrix in G (0: a caller's)
    tfr::DevBuf<double> G;                               // [n_items, n_items]: G, then P in place
    tfr::DevBuf<double> work, dinv;                      // [EASE_NB, n_items] row panel; [blocks, EASE_NB, EASE_NB] inverted blocks
    tfr::DevBuf<float> B;                                // [n_items, n_items]
    tfr::DevBuf<int32_t> err;
};
