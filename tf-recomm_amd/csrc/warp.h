// warp.h - WARP (Weston, Bengio, Usunier, "WSABIE", IJCAI 2011) steps on the SVD model's tables on gfx950: the violator
// search's argument block and launcher, shared by warp.hip and the tfr_warp entry points (warp_api.inc.h).  DESIGN §30.
//
// A WARP step is a BPR step (bpr.h) with two things changed.  The negative of a triple (u, i) is not the first candidate
// outside row u of the positives but the first such candidate c that violates the margin, x = s(u, i) - s(u, c) < margin,
// scored on the pre-step tables; N, the number of non-positive candidates examined up to and including it, estimates the
// positive's rank, and the triple's weight is w = log(max(1, (I - 1) / N)).  The user runs then take the weighted hinge
// (k_bpr_users<NJ, true>: g = x < margin ? -w : 0) in place of the logistic g.  The sort, the item runs, the updates and
// k_finalize are BPR's.  A triple none of whose candidates violates is skipped exactly as a BPR triple whose every draw
// landed on a positive: neg = -1, both item keys i.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bpr.h"

namespace tfr {

constexpr int WARP_GROUP = 4;                          // candidate rows in flight per round of the search (independent loads)

struct WarpSampleArgs {
    BprPos pos;
    // the batch: drawn entries of the positives (ids, [B]) or user / positive columns; neg_in = the caller's negatives
    const int64_t* ids;
    const int32_t* u_in; const int32_t* i_in; const int32_t* neg_in;
    const float* P; const float* Q; const float* bi;   // the pre-step tables
    // outputs: the two 2B-key columns (NULL: the search alone), the positive and negative columns, the trial counts and
    // weights, optional copies of neg and trials
    int32_t* ou; int32_t* oi;
    int32_t* pos_out; int32_t* neg; int32_t* trials; float* wgt;
    int32_t* neg_copy; int32_t* trials_copy;
    uint64_t key;                                      // bpr_key(seed, step)
    int64_t B, U, I;
    int32_t D, item_abs, attempts;
    float margin;
};

// what makes a BPR step of the host side (bpr_api.inc.h bpr_step) a WARP step: the margin, the per-triple trial counts
// and weights (device, [B]) and an optional copy of the trial counts for the caller
struct WarpStep {
    float margin;
    int32_t* trials; float* wgt;
    int32_t* trials_copy;
};

// one wave per triple: (u, i) from the columns or the drawn entries; j, N and w from the search, or N = 1 with the
// caller's negative
void launch_warp_sample(const WarpSampleArgs& a, hipStream_t s);

}  // namespace tfr
