// finetune.h - batched per-user fine-tuning (tfr_finetune_users): launch plan, argument block and launcher shared by
// finetune.hip and api.hip.
//
// One wave per user runs that user's whole schedule: for each round, the pre-training logit of the asked item, then
// nsteps steps on the round's prefix of the user's rows.  The user row, its bias and (lazy Adam) their slots stay in
// registers, lane f holding features f, f + 64, ...; the item rows of the user's training rows are staged in the wave's
// slice of LDS when they fit (FT_WAVE_LDS), and read from global memory otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

constexpr int FT_WAVES = 4;                            // waves (users) per block; the waves never wait for each other
constexpr int64_t FT_WAVE_LDS = 16 * 1024;             // LDS budget of one wave: a block stays within 64 KiB

// per-wave LDS layout, in floats: p [dpad] | asked row [dpad] | dlogit [64] | loss [64] | bi [rows] | rate [rows] |
// item rows [rows][stride].  The odd row stride keeps the row-per-lane reads of the logit phase conflict-free.
__host__ __device__ inline int ft_dpad(int D) { return (D + 3) & ~3; }
__host__ __device__ inline int ft_stride(int D) { return D | 1; }
inline int64_t ft_fixed_floats(int D) { return 2 * (int64_t)ft_dpad(D) + 128; }
inline int64_t ft_wave_floats(int D, int64_t rows) { return (ft_fixed_floats(D) + rows * (ft_stride(D) + 2) + 3) & ~(int64_t)3; }

struct FtPlan {
    int32_t rows_staged;                               // users with at most this many rows are staged in LDS
    int64_t wave_floats;                               // LDS floats per wave
    size_t lds_bytes;                                  // dynamic LDS per block
};

// the plan for a call whose largest user has max_rows rows (dim checked by the caller)
inline FtPlan ft_plan(int D, int64_t max_rows) {
    int64_t cap = (FT_WAVE_LDS / 4 - ft_fixed_floats(D) - 3) / (ft_stride(D) + 2);
    if (cap < 0) cap = 0;
    FtPlan p;
    p.rows_staged = (int32_t)(max_rows < cap ? max_rows : cap);
    p.wave_floats = ft_wave_floats(D, p.rows_staged);
    p.lds_bytes = (size_t)p.wave_floats * 4 * FT_WAVES;
    return p;
}

struct FtArgs {
    float* P; float* bu; float* Pm; float* Pv; float* bum; float* buv;   // the user tables and their Adam slots
    const float* Q; const float* bi; const float* mu;
    const int32_t* users; const int64_t* row_ptr; const int32_t* items; const float* rates;
    const int64_t* round_ptr; const int32_t* ask; const int32_t* prefix;
    const float* bpow;                                 // [2 * n_rounds]: beta1 / beta2 power at each round's first step
    const int32_t* order;                              // [n_users]: schedule users by descending work
    float* ask_out; float* loss_out; float* final_out; // [n_rounds], [n_rounds] or NULL, [n_rows] or NULL
    int64_t n_users, wave_floats;
    int32_t D, nsteps, loss, item_abs, reg_bias, adam, frozen_rows, frozen_bias, rows_staged;
    float lam, lr, b1, b2, eps;
};

void launch_finetune(const FtArgs& a, const FtPlan& p, hipStream_t s);

}  // namespace tfr
