// ease.hip - EASE on gfx950 (tfr_ease_*): a dense symmetric positive-definite inverse in float64.
//   X: the binary user x item matrix (a CSR pattern, rows strictly increasing).  G = X^T X + lambda I, P = G^-1,
//   B[i, j] = (float)(-P[i, j] / P[j, j]) with a zero diagonal, score(u, j) = the float32 add chain from +0 over
//   i in N(u) ascending of B[i, j].
//
// k_ease_gram: one block per item and slice of EASE_W_GRAM columns counts the item's co-occurrences in uint32 LDS counters
//   (item_lists.h count_row), then the counters go out as float64 into row i of G, n_i + lambda on the diagonal.
// The inverse works in place on the lower triangle, EASE_NB columns at a time, in three sweeps over the diagonal blocks:
//   1. Cholesky G = L L^T: k_ease_diag factors the block in LDS and leaves its inverse W in `dinv`; the panel below is
//      multiplied by W^T; the trailing lower triangle loses panel * panel^T.
//   2. M = L^-1, block rows ascending: T = L[i, 0:i] * M[0:i, 0:i] (into the work panel), M[i, 0:i] = -W_i * T, M[i, i] = W_i.
//   3. P = M^T M, block rows ascending: P[i, 0:i+1] = M[i:, i]^T * M[i:, 0:i+1] (into the work panel, then copied).
//   Then k_ease_mirror writes the upper triangle from the lower.  Diagonal blocks carry zeros above their diagonal, blocks
//   and tiles share their edges, and the products start at the first block that is not zero (`kskip`) - so nothing ever
//   reads the stale upper triangle.  Every product is k_ease_gemm: one 64 x 64 tile per workgroup, operands staged
//   through LDS in chunks of 16 along k, each wave 16 rows x 64 columns = four v_mfma_f64_16x16x4_f64 accumulators.  One
//   f64 per lane and operand: A[lane & 15][k = lane >> 4], B[k = lane >> 4][lane & 15]; result register r of a lane is
//   C[(lane >> 4) + 4 r][lane & 15].  k ascends, so a fit is the same bits every time.
// k_ease_weights: one pass over P and its diagonal.
// k_ease_score<MODE>: one wave per (query, slice of EASE_W columns); the lanes hold EASE_COLS accumulators each, load the
//   rows of EASE_AHEAD list items at once (coalesced, the addresses depend on the list alone) and add them in list order.
//   The sums then go to the wave's LDS row and everything after is item_lists.h score_tail: exclusions as NaN, keys and
//   queue, part[query, slice, k] for launch_topk_merge, the two ranking modes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include "tfrecomm.h"
#include "svd_kernels.h"
#include "ease.h"

namespace {

using tfr::wave_lds_sync;
using tfr::fail;
using tfr::check_k;
using tfr::window;

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_ease_gram(EaseGramArgs a) {
    __shared__ uint32_t counts[EASE_W_GRAM];
    static_assert(sizeof(counts) == ease_gram_lds(), "ease_plan reports another LDS size");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lo = (int64_t)blockIdx.y * EASE_W_GRAM;
    const int width = (int)(a.n_items - lo < EASE_W_GRAM ? a.n_items - lo : EASE_W_GRAM);

    for (int64_t i = blockIdx.x; i < a.n_items; i += gridDim.x) {
        const int64_t p0 = a.pi[i], p1 = a.pi[i + 1];
        for (int t = tid; t < width; t += 256) counts[t] = 0;
        __syncthreads();

        tfr::count_row<EASE_WAVES>(a, counts, p0, p1, lo, width, lane, wave);
        __syncthreads();

        double* row = a.G + i * a.n_items + lo;
        for (int t = tid; t < width; t += 256) row[t] = lo + t == i ? (double)(p1 - p0) + a.lambda : (double)counts[t];
        __syncthreads();                                 // the next row's zeroing comes after every store has read its counter
    }
}

// Cholesky factor and its inverse of one diagonal block, in LDS.  S holds the lower triangle (zeros above), W the inverse.
__global__ __launch_bounds__(256) void k_ease_diag(EaseDiagArgs a) {
    __shared__ double S[EASE_NB][EASE_LDD];
    __shared__ double W[EASE_NB][EASE_LDD];
    static_assert(sizeof(S) + sizeof(W) == ease_diag_lds(), "ease_plan reports another LDS size");
    const int tid = threadIdx.x, b = a.b;
    if (*a.err != 0) return;                             // an earlier block was refused: its column stays in the word
    for (int e = tid; e < EASE_NB * EASE_NB; e += 256) {
        const int r = e / EASE_NB, c = e % EASE_NB;
        S[r][c] = r < b && c <= r ? a.G[(int64_t)(a.j + r) * a.ld + a.j + c] : 0.0;
        W[r][c] = 0.0;
    }
    __syncthreads();
    for (int c = 0; c < b; ++c) {
        const double p = S[c][c];
        if (!(p > 0.0) || !isfinite(p)) {                // the same value in every thread: the block leaves together
            if (tid == 0) *a.err = a.j + c + 1;
            return;
        }
        const double d = sqrt(p);
        __syncthreads();
        for (int r = c + 1 + tid; r < b; r += 256) S[r][c] = S[r][c] / d;
        if (tid == 0) S[c][c] = d;
        __syncthreads();
        const int m = b - c - 1;
        for (int e = tid; e < m * m; e += 256) {
            const int r = c + 1 + e / m, cc = c + 1 + e % m;
            if (cc <= r) S[r][cc] -= S[r][c] * S[cc][c];
        }
        __syncthreads();
    }
    // W = S^-1 by columns: W[c][c] = 1 / S[c][c], W[r][c] = -(sum over l in [c, r) of S[r][l] W[l][c]) / S[r][r].  The sum
    // runs from l = 0: W is still zero above the diagonal, S[r][l] is one address for the wave and W[l][c] one row.
    if (tid < b) {
        const int c = tid;
        W[c][c] = 1.0 / S[c][c];
        for (int r = c + 1; r < b; ++r) {
            double s = 0.0;
            for (int l = 0; l < r; ++l) s += S[r][l] * W[l][c];
            W[r][c] = -s / S[r][r];
        }
    }
    __syncthreads();
    for (int e = tid; e < EASE_NB * EASE_NB; e += 256) {
        const int r = e / EASE_NB, c = e % EASE_NB;
        if (r < b && c < b) a.G[(int64_t)(a.j + r) * a.ld + a.j + c] = S[r][c];
        a.W[e] = W[r][c];
    }
}

// C = beta C + sign op(A) op(B): the one tile body of the factorisation (ease.h EaseGemmArgs)
__global__ __launch_bounds__(256) void k_ease_gemm(EaseGemmArgs a) {
    __shared__ double As[EASE_KC][EASE_LDT];             // As[k][m] = sign * op(A)[m0 + m][k0 + k]
    __shared__ double Bs[EASE_KC][EASE_LDT];             // Bs[k][n] = op(B)[k0 + k][n0 + n]
    static_assert(sizeof(As) + sizeof(Bs) == ease_gemm_lds(), "ease_plan reports another LDS size");
    const int tn = blockIdx.x, tm = blockIdx.y;
    if (a.lower && tn > tm) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = tm * EASE_TILE, n0 = tn * EASE_TILE;
    const int lc = lane & 15, lk = lane >> 4;

    // the four elements of each operand's chunk this thread stages: the fast index follows the operand's unit stride
    int am[4], ak[4], bk[4], bn[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (a.ta) { am[r] = tid & 63; ak[r] = (tid >> 6) + 4 * r; } else { ak[r] = tid & 15; am[r] = (tid >> 4) + 16 * r; }
        if (a.tb) { bk[r] = tid & 15; bn[r] = (tid >> 4) + 16 * r; } else { bn[r] = tid & 63; bk[r] = (tid >> 6) + 4 * r; }
    }
    const int64_t sam = a.ta ? 1 : a.lda, sak = a.ta ? a.lda : 1;
    const int64_t sbk = a.tb ? 1 : a.ldb, sbn = a.tb ? a.ldb : 1;
    const double sign = a.sign < 0 ? -1.0 : 1.0;

    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + 16 * wave + lk + 4 * r, col = n0 + 16 * t + lc;
            acc[t][r] = a.beta && row < a.M && col < a.N ? a.C[(int64_t)row * a.ldc + col] : 0.0;
        }
    }

    const int k_begin = a.kskip ? n0 : 0;
    double ra[4], rb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + am[r], ka = k_begin + ak[r], n = n0 + bn[r], kb = k_begin + bk[r];
        ra[r] = m < a.M && ka < a.K ? a.A[m * sam + ka * sak] : 0.0;
        rb[r] = n < a.N && kb < a.K ? a.B[kb * sbk + n * sbn] : 0.0;
    }
    for (int k0 = k_begin; k0 < a.K; k0 += EASE_KC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            As[ak[r]][am[r]] = sign * ra[r];
            Bs[bk[r]][bn[r]] = rb[r];
        }
        __syncthreads();
        if (k0 + EASE_KC < a.K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + am[r], ka = k0 + EASE_KC + ak[r], n = n0 + bn[r], kb = k0 + EASE_KC + bk[r];
                ra[r] = m < a.M && ka < a.K ? a.A[m * sam + ka * sak] : 0.0;
                rb[r] = n < a.N && kb < a.K ? a.B[kb * sbk + n * sbn] : 0.0;
            }
        }
#pragma unroll
        for (int kk = 0; kk < EASE_KC; kk += 4) {
            const double av = As[kk + lk][16 * wave + lc];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[kk + lk][16 * t + lc], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + 16 * wave + lk + 4 * r, col = n0 + 16 * t + lc;
            if (row < a.M && col < a.N) a.C[(int64_t)row * a.ldc + col] = acc[t][r];
        }
    }
}

// dst[r, c] = src[r, c] over rows x cols
__global__ __launch_bounds__(256) void k_ease_copy(double* dst, int64_t ldd, const double* src, int64_t lds, int rows, int cols) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / cols, c = e % cols;
        dst[r * ldd + c] = src[r * lds + c];
    }
}

// P[c, r] = P[r, c] for r > c: 32 x 32 tiles of the lower triangle through LDS, both sides coalesced
__global__ __launch_bounds__(256) void k_ease_mirror(double* P, int64_t n) {
    __shared__ double t[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;          // tile (by, bx) of the lower triangle: by >= bx
    if (bx > by) return;
    const int x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
    for (int y = y0; y < 32; y += 8) {
        const int64_t r = (int64_t)by * 32 + y, c = (int64_t)bx * 32 + x;
        if (r < n && c < n) t[y][x] = P[r * n + c];
    }
    __syncthreads();
    for (int y = y0; y < 32; y += 8) {
        const int64_t r = (int64_t)bx * 32 + y, c = (int64_t)by * 32 + x;    // the element above the diagonal
        if (r < n && c < n && c > r) P[r * n + c] = t[x][y];
    }
}

__global__ __launch_bounds__(256) void k_ease_weights(const double* P, float* B, int64_t n) {
    const int64_t total = n * n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / n, j = e % n;
        B[e] = i == j ? 0.f : __double2float_rn(-P[e] / P[j * n + j]);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_ease_score(EaseScoreArgs a) {
    __shared__ float acc[EASE_WAVES][EASE_W];
    __shared__ uint64_t queue[EASE_WAVES][EASE_SCORE_CAP];
    static_assert(sizeof(acc) + sizeof(queue) == ease_score_lds(), "ease_plan reports another LDS size");
    static_assert(EASE_SCORE_CAP >= EASE_KMAX + 64, "a queue must hold k plus one append");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * EASE_WAVES + wave;
    if (w >= a.n * a.slices) return;                     // waves never meet at a block barrier
    const int64_t qi = a.q_lo + w / a.slices;
    const int slice = (int)(w % a.slices);
    const int64_t row = a.users ? (int64_t)a.users[qi] : qi;
    const int64_t l0 = a.ptr[row], l1 = a.ptr[row + 1];
    const int64_t lo = (int64_t)slice * EASE_W;
    const int width = (int)(a.n_items - lo < EASE_W ? a.n_items - lo : EASE_W);
    float* A = acc[wave];

    float s[EASE_COLS];
#pragma unroll
    for (int c = 0; c < EASE_COLS; ++c) s[c] = 0.f;
    for (int64_t g = l0; g < l1; g += EASE_AHEAD) {
        float v[EASE_AHEAD][EASE_COLS];
#pragma unroll
        for (int d = 0; d < EASE_AHEAD; ++d) {
            const bool has = g + d < l1;
            const float* src = a.B + (has ? (int64_t)a.ids[g + d] : 0) * a.n_items + lo;
#pragma unroll
            for (int c = 0; c < EASE_COLS; ++c) {
                const int col = lane + 64 * c;
                v[d][c] = has && col < width ? src[col] : 0.f;
            }
        }
#pragma unroll
        for (int d = 0; d < EASE_AHEAD; ++d) {
            if (g + d < l1) {                            // wave-uniform
#pragma unroll
                for (int c = 0; c < EASE_COLS; ++c) s[c] += v[d][c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < EASE_COLS; ++c)
        if (lane + 64 * c < width) A[lane + 64 * c] = s[c];
    wave_lds_sync();
    tfr::score_tail<MODE, EASE_SCORE_CAP>(a, A, queue[wave], qi, w, lo, width, lane);
}

thread_local tfr::ErrText g_ease_err;

void launch_gemm(hipStream_t s, const double* A, int64_t lda, int ta, const double* B, int64_t ldb, int tb, double* C, int64_t ldc,
                 int M, int N, int K, int sign, int beta, int lower, int kskip) {
    EaseGemmArgs g;
    g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.ta = ta; g.tb = tb; g.sign = sign; g.beta = beta; g.lower = lower; g.kskip = kskip;
    ease_launch_gemm(g, s);
}

void launch_copy(hipStream_t s, double* dst, int64_t ldd, const double* src, int64_t lds, int rows, int cols) {
    const int64_t blocks = ((int64_t)rows * cols + 255) / 256;
    hipLaunchKernelGGL(k_ease_copy, dim3((unsigned)std::min<int64_t>(blocks, 4096)), dim3(256), 0, s, dst, ldd, src, lds, rows, cols);
}

// G = L L^T in place on the lower triangle; the inverted diagonal blocks go to dinv
void ease_factor(tfr_ease* m) {
    const int n = (int)m->n_items;
    const int64_t ld = n;
    double* G = m->G;
    hipStream_t s = m->stream;
    for (int j = 0, kb = 0; j < n; j += EASE_NB, ++kb) {
        const int b = std::min(EASE_NB, n - j), below = n - j - b;
        double* W = m->dinv.get() + (size_t)kb * EASE_NB * EASE_NB;
        EaseDiagArgs d;
        d.G = G; d.ld = ld; d.W = W; d.err = m->err; d.j = j; d.b = b;
        hipLaunchKernelGGL(k_ease_diag, dim3(1), dim3(256), 0, s, d);
        if (below == 0) break;
        double* panel = G + (int64_t)(j + b) * ld + j;
        launch_gemm(s, panel, ld, 0, W, EASE_NB, 1, panel, ld, below, b, b, 1, 0, 0, 0);          // panel * W^T, in place by rows
        launch_gemm(s, panel, ld, 0, panel, ld, 1, G + (int64_t)(j + b) * ld + j + b, ld, below, below, b, -1, 1, 1, 0);
    }
}

// M = L^-1, then P = M^T M, then the upper triangle
void ease_invert_factor(tfr_ease* m) {
    const int n = (int)m->n_items;
    const int64_t ld = n;
    double* G = m->G;
    double* T = m->work;
    hipStream_t s = m->stream;
    for (int j = 0, kb = 0; j < n; j += EASE_NB, ++kb) {
        const int b = std::min(EASE_NB, n - j);
        const double* W = m->dinv.get() + (size_t)kb * EASE_NB * EASE_NB;
        if (j > 0) {
            launch_gemm(s, G + (int64_t)j * ld, ld, 0, G, ld, 0, T, ld, b, j, j, 1, 0, 0, 1);     // T = L[j, 0:j] M[0:j, 0:j]
            launch_gemm(s, W, EASE_NB, 0, T, ld, 0, G + (int64_t)j * ld, ld, b, j, b, -1, 0, 0, 0);
        }
        launch_copy(s, G + (int64_t)j * ld + j, ld, W, EASE_NB, b, b);
    }
    for (int j = 0; j < n; j += EASE_NB) {
        const int b = std::min(EASE_NB, n - j);
        launch_gemm(s, G + (int64_t)j * ld + j, ld, 1, G + (int64_t)j * ld, ld, 0, T, ld, b, j + b, n - j, 1, 0, 0, 0);
        launch_copy(s, G + (int64_t)j * ld, ld, T, ld, b, j + b);
    }
    const unsigned t = (unsigned)((n + 31) / 32);
    hipLaunchKernelGGL(k_ease_mirror, dim3(t, t), dim3(256), 0, s, G, (int64_t)n);
}

// what the serving drivers of item_lists.h ask of a family
struct EaseServe {
    using Model = tfr_ease;
    using Args = EaseScoreArgs;
    using Plan = EasePlan;
    static constexpr auto plan = ease_plan;
    static constexpr const char* load_fn = "tfr_ease_load";
    static constexpr const char* not_fitted = "no weights: call tfr_ease_solve or tfr_ease_set_weights first";

    static Args args(const Model* m) {
        Args a = {};
        a.B = m->B;
        return a;
    }

    template <int MODE>
    static void launch(const Args& a, hipStream_t s) { ease_launch_score(MODE, a, s); }
};

// the f64 buffer and what the factorisation needs beside it
int ease_reserve_f64(tfr_ease* m) {
    EasePlan p;
    if (!ease_plan(0, m->n_items, 1, 0, &p)) return fail(g_ease_err, TFR_ERR_ARG, "no plan for %lld items", (long long)m->n_items);
    LISTCHK(g_ease_err, m->G.reserve(m->n_items * m->n_items, m->stream));
    LISTCHK(g_ease_err, m->work.reserve((int64_t)EASE_NB * m->n_items, m->stream));
    LISTCHK(g_ease_err, m->dinv.reserve((int64_t)p.blocks * EASE_NB * EASE_NB, m->stream));
    return TFR_OK;
}

}  // namespace

void ease_launch_gram(const EaseGramArgs& a, int32_t slices, hipStream_t s) {
    const dim3 g((unsigned)std::min<int64_t>(a.n_items, EASE_GRID_ROWS), (unsigned)slices);
    hipLaunchKernelGGL(k_ease_gram, g, dim3(256), 0, s, a);
}

void ease_launch_gemm(const EaseGemmArgs& g, hipStream_t s) {
    const dim3 grid((unsigned)((g.N + EASE_TILE - 1) / EASE_TILE), (unsigned)((g.M + EASE_TILE - 1) / EASE_TILE));
    hipLaunchKernelGGL(k_ease_gemm, grid, dim3(256), 0, s, g);
}

void ease_launch_score(int mode, const EaseScoreArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.n * a.slices + EASE_WAVES - 1) / EASE_WAVES));
    if (mode == 0) hipLaunchKernelGGL(k_ease_score<0>, g, dim3(256), 0, s, a);
    else if (mode == 1) hipLaunchKernelGGL(k_ease_score<1>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_ease_score<2>, g, dim3(256), 0, s, a);
}

extern "C" {

const char* tfr_ease_last_error(void) { return g_ease_err.text; }

int tfr_ease_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t which, int32_t* block, int32_t* tile, int64_t* lds_bytes,
                  int64_t* f64_bytes, int64_t* f32_bytes, int32_t* slice_width, int32_t* slices, int64_t* row_chunk,
                  int32_t* look_ahead) {
    if (which < 0 || which > 1) return fail(g_ease_err, TFR_ERR_ARG, "ease plan: which must be 0 (fit) or 1 (scoring)");
    if (n_items < 1 || n_items > EASE_MAX_ITEMS || n_rows < 0)
        return fail(g_ease_err, TFR_ERR_ARG, "ease plan: n_rows >= 0 and 1 <= n_items <= %lld", (long long)EASE_MAX_ITEMS);
    if (int rc = check_k(g_ease_err, "ease plan", k)) return rc;
    EasePlan p;
    if (!ease_plan(which, n_items, k, n_rows, &p)) return fail(g_ease_err, TFR_ERR_ARG, "ease plan: no plan for k %d over %lld items", k, (long long)n_items);
    if (block) *block = p.nb;
    if (tile) *tile = p.tile;
    if (lds_bytes) *lds_bytes = (int64_t)(which ? std::max(p.lds, tfr::topk_merge_lds(p.slices, k)) : std::max(p.lds, ease_gemm_lds()));
    if (f64_bytes) *f64_bytes = p.f64_bytes;
    if (f32_bytes) *f32_bytes = p.f32_bytes;
    if (slice_width) *slice_width = p.width;
    if (slices) *slices = p.slices;
    if (row_chunk) *row_chunk = p.chunk;
    if (look_ahead) *look_ahead = p.ahead;
    return TFR_OK;
}

int tfr_ease_destroy(tfr_ease* m) { return m ? tfr::destroy_handle(m, {m->ev0, m->ev1, m->ev2}) : TFR_OK; }

int tfr_ease_create(tfr_ease** out, int64_t n_users, int64_t n_items, double lambda, int32_t device) {
    if (!out) return fail(g_ease_err, TFR_ERR_ARG, "out is null");
    *out = nullptr;
    // an item count past the dense cap is refused with the cap's own message
    if (int rc = tfr::check_counts(g_ease_err, n_users, std::min(n_items, EASE_MAX_ITEMS))) return rc;
    if (n_items > EASE_MAX_ITEMS)
        return fail(g_ease_err, TFR_ERR_ARG, "%lld items are past the dense cap of %lld (12 bytes per entry of the item x item matrices)",
                    (long long)n_items, (long long)EASE_MAX_ITEMS);
    if (!(lambda > 0.0) || !std::isfinite(lambda)) return fail(g_ease_err, TFR_ERR_ARG, "lambda must be positive and finite");
    tfr_ease* m = nullptr;
    if (int rc = tfr::create_handle(g_ease_err, "ease_create", &m, n_users, n_items, device)) return rc;
    m->lambda = lambda;
    hipError_t e = m->err.reserve(1, m->stream);
    if (e == hipSuccess) e = hipEventCreate(&m->ev0);
    if (e == hipSuccess) e = hipEventCreate(&m->ev1);
    if (e == hipSuccess) e = hipEventCreate(&m->ev2);
    if (e != hipSuccess) {
        const int code = e == hipErrorOutOfMemory ? TFR_ERR_NOMEM : TFR_ERR_HIP;
        tfr_ease_destroy(m);
        return fail(g_ease_err, code, "ease_create: %s", hipGetErrorString(e));
    }
    *out = m;
    return TFR_OK;
}

// A load forgets the Gram matrix and the weights (item_lists.h load_lists: `fitted`, and what the f64 buffer holds).
int tfr_ease_load(tfr_ease* m, const int64_t* indptr, const int32_t* items) {
    return tfr::load_lists(g_ease_err, m, indptr, items, [m] { m->f64_is = 0; m->gram_ms = 0.f; });
}

int tfr_ease_gram(tfr_ease* m) {
    if (!m) return fail(g_ease_err, TFR_ERR_ARG, "null model");
    if (!m->loaded) return fail(g_ease_err, TFR_ERR_STATE, "no data: call tfr_ease_load first");
    EasePlan p;
    if (!ease_plan(0, m->n_items, 1, 0, &p)) return fail(g_ease_err, TFR_ERR_ARG, "gram: no plan");
    LISTCHK(g_ease_err, hipSetDevice(m->device));
    m->f64_is = 0;
    if (int rc = ease_reserve_f64(m)) return rc;
    hipStream_t s = m->stream;
    (void)hipEventRecord(m->ev0, s);
    EaseGramArgs a = {};
    a.pu = m->pu; a.items = m->items; a.pi = m->pi; a.iu = m->iu; a.G = m->G; a.n_items = m->n_items; a.lambda = m->lambda;
    ease_launch_gram(a, p.slices, s);
    LISTCHK(g_ease_err, hipGetLastError());
    (void)hipEventRecord(m->ev1, s);
    LISTCHK(g_ease_err, hipStreamSynchronize(s));
    if (hipEventElapsedTime(&m->gram_ms, m->ev0, m->ev1) != hipSuccess) m->gram_ms = 0.f;
    m->f64_is = 1;
    return TFR_OK;
}

int tfr_ease_set_gram(tfr_ease* m, const double* G) {
    if (!m) return fail(g_ease_err, TFR_ERR_ARG, "null model");
    if (!G) return fail(g_ease_err, TFR_ERR_ARG, "set_gram: null matrix");
    const int64_t n = m->n_items;
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(G[i * n + j])) return fail(g_ease_err, TFR_ERR_ARG, "set_gram: entry (%lld, %lld) is not finite", (long long)i, (long long)j);
        if (!(G[i * n + i] > 0.0)) return fail(g_ease_err, TFR_ERR_ARG, "set_gram: diagonal entry %lld is not positive", (long long)i);
        for (int64_t j = 0; j < i; ++j)
            if (memcmp(&G[i * n + j], &G[j * n + i], 8) != 0)
                return fail(g_ease_err, TFR_ERR_ARG, "set_gram: entries (%lld, %lld) and (%lld, %lld) differ", (long long)i, (long long)j,
                                 (long long)j, (long long)i);
    }
    LISTCHK(g_ease_err, hipSetDevice(m->device));
    m->f64_is = 0;
    if (int rc = ease_reserve_f64(m)) return rc;
    LISTCHK(g_ease_err, hipMemcpyAsync(m->G, G, (size_t)n * n * 8, hipMemcpyHostToDevice, m->stream));
    LISTCHK(g_ease_err, hipStreamSynchronize(m->stream));
    m->gram_ms = 0.f;
    m->f64_is = 1;
    return TFR_OK;
}

int tfr_ease_solve(tfr_ease* m, int32_t keep_inverse, float* elapsed_ms) {
    if (!m) return fail(g_ease_err, TFR_ERR_ARG, "null model");
    if (m->f64_is != 1) return fail(g_ease_err, TFR_ERR_STATE, "no Gram matrix: call tfr_ease_gram or tfr_ease_set_gram first");
    const int64_t n = m->n_items;
    LISTCHK(g_ease_err, hipSetDevice(m->device));
    hipStream_t s = m->stream;
    m->fitted = false;
    m->f64_is = 0;                                       // the factorisation overwrites G
    LISTCHK(g_ease_err, m->B.reserve(n * n, s));
    LISTCHK(g_ease_err, hipMemsetAsync(m->err, 0, 4, s));
    (void)hipEventRecord(m->ev0, s);
    ease_factor(m);
    LISTCHK(g_ease_err, hipGetLastError());
    int32_t bad = 0;
    LISTCHK(g_ease_err, hipMemcpyAsync(&bad, m->err, 4, hipMemcpyDeviceToHost, s));
    LISTCHK(g_ease_err, hipStreamSynchronize(s));
    if (bad != 0)
        return fail(g_ease_err, TFR_ERR_ARG, "solve: the matrix is not positive definite: the pivot of column %d is not positive and finite", bad - 1);
    ease_invert_factor(m);
    LISTCHK(g_ease_err, hipGetLastError());
    (void)hipEventRecord(m->ev1, s);
    const int64_t blocks = (n * n + 255) / 256;
    hipLaunchKernelGGL(k_ease_weights, dim3((unsigned)std::min<int64_t>(blocks, 16384)), dim3(256), 0, s, m->G.get(), m->B.get(), n);
    LISTCHK(g_ease_err, hipGetLastError());
    (void)hipEventRecord(m->ev2, s);
    LISTCHK(g_ease_err, hipStreamSynchronize(s));
    if (elapsed_ms) {
        elapsed_ms[0] = m->gram_ms;
        if (hipEventElapsedTime(&elapsed_ms[1], m->ev0, m->ev1) != hipSuccess) elapsed_ms[1] = 0.f;
        if (hipEventElapsedTime(&elapsed_ms[2], m->ev1, m->ev2) != hipSuccess) elapsed_ms[2] = 0.f;
    }
    if (keep_inverse) {
        m->f64_is = 2;
    } else {
        m->G.reset();
        m->work.reset();
        m->dinv.reset();
    }
    m->fitted = true;
    return TFR_OK;
}

int tfr_ease_get_f64(tfr_ease* m, int64_t row_lo, int64_t n_rows, double* out) {
    if (!m) return fail(g_ease_err, TFR_ERR_ARG, "null model");
    if (m->f64_is == 0) return fail(g_ease_err, TFR_ERR_STATE, "no float64 matrix: it holds G after gram / set_gram and P after a solve that kept it");
    if (int rc = window(g_ease_err, m, "get_f64", row_lo, n_rows)) return rc;
    if (n_rows == 0) return TFR_OK;
    if (!out) return fail(g_ease_err, TFR_ERR_ARG, "get_f64: null out");
    LISTCHK(g_ease_err, hipSetDevice(m->device));
    LISTCHK(g_ease_err, hipMemcpyAsync(out, m->G.get() + row_lo * m->n_items, (size_t)n_rows * m->n_items * 8, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_ease_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

int tfr_ease_get_weights(tfr_ease* m, int64_t row_lo, int64_t n_rows, float* out) {
    if (!m) return fail(g_ease_err, TFR_ERR_ARG, "null model");
    if (!m->fitted) return fail(g_ease_err, TFR_ERR_STATE, "no weights: call tfr_ease_solve or tfr_ease_set_weights first");
    if (int rc = window(g_ease_err, m, "get_weights", row_lo, n_rows)) return rc;
    if (n_rows == 0) return TFR_OK;
    if (!out) return fail(g_ease_err, TFR_ERR_ARG, "get_weights: null out");
    LISTCHK(g_ease_err, hipSetDevice(m->device));
    LISTCHK(g_ease_err, hipMemcpyAsync(out, m->B.get() + row_lo * m->n_items, (size_t)n_rows * m->n_items * 4, hipMemcpyDeviceToHost, m->stream));
    LISTCHK(g_ease_err, hipStreamSynchronize(m->stream));
    return TFR_OK;
}

// Rows [row_lo, row_lo + n_rows) of B from a host array.  Checked before any device work.  A handle without weights takes
// all rows at once, which makes it fitted; a fitted one takes any window.
int tfr_ease_set_weights(tfr_ease* m, int64_t row_lo, int64_t n_rows, const float* in) {
    if (!m) return fail(g_ease_err, TFR_ERR_ARG, "null model");
    if (int rc = window(g_ease_err, m, "set_weights", row_lo, n_rows)) return rc;
    if (n_rows > 0 && !in) return fail(g_ease_err, TFR_ERR_ARG, "set_weights: null weights");
    const int64_t n = m->n_items;
    for (int64_t e = 0; e < n_rows * n; ++e)
        if (!std::isfinite(in[e]))
            return fail(g_ease_err, TFR_ERR_ARG, "set_weights: the weight (%lld, %lld) is not finite", (long long)(row_lo + e / n), (long long)(e % n));
    if (!m->fitted && n_rows != n) return fail(g_ease_err, TFR_ERR_STATE, "set_weights: a model without weights takes all %lld rows at once", (long long)n);
    if (n_rows == 0) return TFR_OK;
    LISTCHK(g_ease_err, hipSetDevice(m->device));
    LISTCHK(g_ease_err, m->B.reserve(n * n, m->stream));
    LISTCHK(g_ease_err, hipMemcpyAsync(m->B.get() + row_lo * n, in, (size_t)n_rows * n * 4, hipMemcpyHostToDevice, m->stream));
    LISTCHK(g_ease_err, hipStreamSynchronize(m->stream));
    m->fitted = true;
    return TFR_OK;
}

int tfr_ease_topk(tfr_ease* m, const int32_t* users, int64_t n, int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                  int32_t* items_out, float* scores_out) {
    return tfr::topk_users<EaseServe>(g_ease_err, m, users, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_ease_topk_lists(tfr_ease* m, const int64_t* list_indptr, const int32_t* list_items, int64_t n, int32_t k,
                        const int64_t* excl_indptr, const int32_t* excl_items, int32_t* items_out, float* scores_out) {
    return tfr::topk_lists<EaseServe>(g_ease_err, m, list_indptr, list_items, n, k, excl_indptr, excl_items, items_out, scores_out);
}

int tfr_ease_rank_items(tfr_ease* m, const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
                        const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out) {
    return tfr::rank_users<EaseServe>(g_ease_err, m, users, n, tgt_indptr, tgt_items, excl_indptr, excl_items, ranks_out);
}

}  // extern "C"
