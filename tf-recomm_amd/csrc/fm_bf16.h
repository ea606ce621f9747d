// fm_bf16.h - the FM second-order forward on the bf16 snapshot's rows (fm_bf16.hip): inference only.
// V is the snapshot's copy of the feature rows (bf16_rows.h: stride DP, pads +0), W and mu the float32 copies taken at the
// same moment.  G = bf16_geometry(D) lanes own one CSR row, one 16-byte fragment of 8 elements per lane and non-zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

struct FmBf16Args {
    const uint16_t* V; const float* W; const float* mu;
    const int64_t* indptr; const int32_t* indices; const float* data;
    float* out; int32_t* err;
    int64_t n_rows, F;
    int32_t DP;
};

int fm_bf16_grid(int64_t n_rows, int G);
// ntv: V rows by non-temporal loads
void launch_fm_bf16(const FmBf16Args& a, int G, int grid, bool ntv, hipStream_t s);

}  // namespace tfr
