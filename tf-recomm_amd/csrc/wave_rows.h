// wave_rows.h - what the wave-per-run kernels share (svdpp.hip, bpr.hip, finetune.hip).  DESIGN §18.
//
// One wave owns a row or a run of a sorted column.  Features lie across the lanes, f = lane + 64 j, NJ = ceil(D / 64)
// registers per lane (registers past D hold 0).  ROW_WAVES independent waves share a block: no block barrier, no atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "svd_kernels.h"

namespace tfr {

constexpr int ROW_WAVES = 4;                           // = PP_WAVES = BPR_WAVES = FT_WAVES (asserted where wave_slot is used)

// the unit of work of this wave
__device__ __forceinline__ int64_t wave_slot() { return (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6); }

// butterfly sum: every lane ends with the same bits (svd_kernels.hip wave_sum is the other one: valid in lane 0 only)
__device__ __forceinline__ float wave_sum_all(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// first sorted position past the run of key at p (ks sorted: the equal keys are a prefix of every 64-entry window)
__device__ __forceinline__ int64_t sorted_run_end(const int32_t* ks, int64_t p, int64_t n, int lane) {
    const int32_t key = ks[p];
    int64_t q = p + 1;
    for (;;) {
        const int64_t e = q + lane;
        const unsigned long long same = __ballot(e < n && ks[e] == key);
        if (same == ~0ull) { q += 64; continue; }
        return q + (__ffsll((long long)~same) - 1);
    }
}

// body(j, f) for this lane's features f = lane + 64 j < D, fully unrolled
template <int NJ, typename F>
__device__ __forceinline__ void each_feature(int lane, int D, F&& body) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int f = lane + 64 * j;
        if (f < D) body(j, f);
    }
}

// one value: SGD, or lazy Adam in the pinned order of adam_sparse (svd_kernels.h); update_at is either on element x of a table
// (the slots pass through registers: to the compiler a store to m[x] may alias v[x] or w[x])
__device__ __forceinline__ void sgd_step(float& w, float g, float lr) { w = w - lr * g; }
__device__ __forceinline__ void update_at(float* w, float* m, float* v, int64_t x, float g, bool adam, const AdamC& c, float lr) {
    if (adam) {
        float mm = m[x], vv = v[x];
        adam_sparse(w[x], mm, vv, g, c);
        m[x] = mm;
        v[x] = vv;
    } else {
        sgd_step(w[x], g, lr);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// NJ from D, once: f(std::integral_constant<int, NJ>) with NJ = ceil(D / 64) in 1..4 (the entry points hold D <= 256)
template <typename F>
inline void with_nj(int D, F&& f) { with_one_of<1, 2, 3, 4>(D > 0 && D <= 192 ? (D + 63) / 64 : 4, f); }

inline dim3 wave_grid(int64_t waves) { return dim3((unsigned)((waves + ROW_WAVES - 1) / ROW_WAVES)); }
inline dim3 wave_block() { return dim3(64 * ROW_WAVES); }

}  // namespace tfr
