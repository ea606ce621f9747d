// fm_fit.h - the FM trainer's data side on gfx950: minibatches gathered on the device from a resident CSR row store, and the
// binary metrics of resident predictions.  Argument blocks and launchers shared by fm_fit.hip and the tfr_fm entry points
// built on them (fm_fit_api.inc.h).  DESIGN §16.
//
// A minibatch is rows ids[0..B) of the store, in id order, duplicates repeated: what scipy's X[ids] / y[ids] give.  The
// kernels never touch V, so they are not compiled per row width.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

constexpr int FM_SCAN_CHUNK = 2048;                    // rows per block of the length scan (256 threads x 8 rounds)
constexpr int FM_WIDE_ROUNDS = 4;                      // a row longer than this many turns of its lane group goes to the whole wave

struct FmGatherArgs {
    const int64_t* ids;                                // [B] store rows, device; the host has checked them against [0, n_rows)
    const int64_t* sp; const int32_t* si; const float* sx; const float* sy;   // the store: indptr, indices, data, targets
    int64_t* indptr; int32_t* indices; float* data; float* y;                 // the minibatch: [B + 1], [nnz], [nnz], [B]
    int64_t* blk;                                      // [ceil(B / FM_SCAN_CHUNK)] scratch: chunk totals, then their exclusive scan
    int64_t B, nnz;                                    // nnz: the outputs' size, summed by the host from its copy of the row lengths
};

// lanes per row of the copy for a batch of B rows with nnz entries: the power of two in [4, 64] that covers the mean row
int fm_gather_group(int64_t B, int64_t nnz);
// row lengths -> int64 exclusive scan (indptr, y) -> the copy (indices, data): four launches on s, no atomics
void launch_fm_gather(const FmGatherArgs& a, hipStream_t s);

// per-block {count of round(sigmoid(logit)) == y, summed sigmoid cross-entropy} of n predictions, by the formulas the SVD
// forward's evaluation mode uses; partials holds fm_metrics_grid(n) * 2
int fm_metrics_grid(int64_t n);
void launch_fm_binary_metrics(const float* logits, const float* y, int64_t n, float* partials, hipStream_t s);

}  // namespace tfr
