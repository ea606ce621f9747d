// bpr.h - BPR (Rendle et al., UAI 2009) steps on the SVD model's tables on gfx950: argument blocks and launchers shared
// by bpr.hip and the tfr_bpr entry points (bpr_api.inc.h).  DESIGN §15.
//
// A step works on triples (u, i, j): i a positive of u, j a negative drawn by the counter-based sampler (or given by the
// caller).  Triple b has two item occurrences, 2b = (i_b, +g_b) and 2b+1 = (j_b, -g_b), and its user appears at the same two
// positions of the user column, so one radix sort of two 2B-key columns orders both sides.  A skipped triple (every draw
// landed on a positive) has j_b = -1 and both its item keys i_b: it sorts like any other and every kernel passes over it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

constexpr int BPR_WAVES = 4;                           // independent waves per block (no block barrier in any kernel)
constexpr int BPR_MAX_ATTEMPTS = 64;                   // draws per triple: the attempt number fills the low 6 bits of the counter

// the positives CSR [U, I] (rows strictly increasing) and the row of each entry (the drawn form's e -> u)
struct BprPos {
    const int64_t* ip; const int32_t* idx; const int32_t* rowof;
    int64_t nnz;
};

struct BprSampleArgs {
    BprPos pos;
    // the batch: drawn entries of the positives (ids, [B]) or user / positive columns; neg_in = the caller's negatives
    const int64_t* ids;
    const int32_t* u_in; const int32_t* i_in; const int32_t* neg_in;
    // outputs: the two 2B-key columns (NULL: sampling alone), the positive and negative columns, an optional copy of neg
    int32_t* ou; int32_t* oi;
    int32_t* pos_out; int32_t* neg; int32_t* neg_copy;
    uint64_t key;                                      // mix(mix(seed ^ golden) ^ step)
    int64_t B, U, I;
    int32_t attempts;
};

struct BprArgs {
    float* P; float* Q; float* bi;
    float *Pm, *Pv, *Qm, *Qv, *bim, *biv;
    const int32_t* ks_u; const int32_t* ps_u;          // the 2B user keys sorted, their positions
    const int32_t* ks_i; const int32_t* ps_i;          // the 2B item keys sorted, their positions
    const int32_t* pos; const int32_t* neg;            // [B]
    float* g;                                          // [B] g_b = -sigmoid(-x_b); the hinge form: -w_b where x_b < margin, else 0
    int32_t* head;                                     // [B] the pold row of triple b's user
    float* pold;                                       // [B, D] pre-step P rows of the user runs (row = run head / 2)
    float* scal;                                       // [B, 4] {data, reg, -, -} per user run (zero elsewhere)
    const int32_t* err;
    int64_t B;
    int32_t D, item_abs, reg_bias, opt;                // opt: 0 lazy Adam, 1 SGD
    uint32_t frozen;                                   // bits TFR_MU..TFR_Q
    float lam, alpha, b1, b2, eps, omb1, omb2, lr;
    // the hinge form (WARP, warp.h): the per-triple weights and the margin; wgt NULL = the logistic form
    const float* wgt; float margin;
};

// the sampler's counter key of a step: the restatement in include/tfrecomm.h
__host__ __device__ inline uint64_t bpr_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
inline uint64_t bpr_key(uint64_t seed, int64_t step) { return bpr_mix(bpr_mix(seed ^ 0x9E3779B97F4A7C15ull) ^ (uint64_t)step); }

// x of a triple from its two dots and its two biases: the one place it is formed, so that the WARP search (warp.hip) and
// the user runs compare and use the same bits
__device__ __forceinline__ float bpr_x(float di, float bii, float dj, float bij) { return (di + bii) - (dj + bij); }

// one thread per triple: (u, i) from the columns or the drawn entries, j from the sampler or the caller
void launch_bpr_sample(const BprSampleArgs& a, hipStream_t s);
// one wave per user run (B waves, wave w at sorted position 2w): scores, g, the run's scalars, pold, the P update;
// a.wgt set = the hinge form: g = x < margin ? -w : 0 and the data term w max(0, margin - x)
void launch_bpr_users(const BprArgs& a, hipStream_t s);
// one wave per item run (2B waves): the Q / item_bias gradient over the run's occurrences from pold and g, and the update
void launch_bpr_items(const BprArgs& a, hipStream_t s);

}  // namespace tfr
