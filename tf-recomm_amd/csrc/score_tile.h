// score_tile.h - the pieces topk.hip, rank.hip and neighbours.hip share: the 64-bit ordering key of a scored pair, the one-wave
// bitonic sort of keys in LDS, the queue compaction built on it, and the MFMA tile that scores 32 items against 32 user
// columns.
//
// key(s, item) = (order-preserving uint32 of s) << 32 | ~item: one 64-bit compare orders by score descending, then item id
// ascending; every non-NaN score gives a key above 0, so key 0 marks an empty slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svd_kernels.h"

namespace tfr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint64_t topk_key(float s, int64_t item) {
    const uint32_t b = __float_as_uint(s);
    const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)o << 32) | (uint32_t)~(uint32_t)item;
}

__device__ __forceinline__ float topk_key_score(uint64_t key) {
    const uint32_t o = (uint32_t)(key >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// descending bitonic sort of q[0..CAP) by one wave
template <int CAP>
__device__ __forceinline__ void wave_sort_desc(uint64_t* q, int lane) {
    for (int size = 2; size <= CAP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
            for (int t0 = 0; t0 < CAP / 2; t0 += 64) {
                const int t = t0 + lane;
                const int i = 2 * t - (t & (stride - 1));
                const int j = i + stride;
                const uint64_t x = q[i], y = q[j];
                const bool desc = (i & size) == 0;
                if ((x < y) == desc) { q[i] = y; q[j] = x; }
            }
            wave_lds_sync();
        }
    }
}

// sort user u's queue, keep its k best, raise its threshold (one wave; cnt / thr / queue are LDS)
template <int CAP>
__device__ __forceinline__ void topk_compact(uint64_t* q, int32_t* cnt, uint64_t* thr, int k, int lane) {
    const int n = *cnt;
    for (int t = n + lane; t < CAP; t += 64) q[t] = 0;
    wave_lds_sync();
    wave_sort_desc<CAP>(q, lane);
    const int keep = n < k ? n : k;
    if (lane == 0) {
        *cnt = keep;
        *thr = keep == k ? q[k - 1] : 0;
    }
    wave_lds_sync();
}

// item in the sorted (non-decreasing) x[lo, hi)
__device__ __forceinline__ bool topk_excluded(const int32_t* x, int64_t lo, int64_t hi, int32_t item) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (x[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo < end && x[lo] == item;
}

template <bool V4>
__device__ __forceinline__ float4 topk_load4(const float* row, int t, int D) {
    if (V4) return *reinterpret_cast<const float4*>(row + 4 * t);
    const int f = 4 * t;
    float4 v;
    v.x = f < D ? row[f] : 0.f;
    v.y = f + 1 < D ? row[f + 1] : 0.f;
    v.z = f + 2 < D ? row[f + 2] : 0.f;
    v.w = f + 3 < D ? row[f + 3] : 0.f;
    return v;
}

// The dot products of one 32 x 32 tile: lane (c, h) = (lane & 31, lane >> 5) gives A[item c][f] from qrow (Q' = |Q| with
// item_abs) and B[f][column c] from prow for f = 2s + h of step s, k ascending from a zero accumulator, odd dims zero-padded.
// On return the lane holds column c against items (r & 3) + 8 (r >> 2) + 4 h, r = 0..15.  Every element of the tile goes
// through the same instruction sequence, so a pair's dot has the same bits whichever tile, row or column scored it.
// ABS_B (neighbours.hip: both operands are rows of the one table): item_abs takes |.| of the B rows too.
template <bool V4, bool ABS_B = false>
__device__ __forceinline__ f32x16 mfma_tile_dot(const float* qrow, const float* prow, int D, int item_abs, int h) {
    const int DP4 = (D + 3) >> 2;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int t0 = 0; t0 < DP4; t0 += 4) {
        float4 qa[4], pb[4];
#pragma unroll
        for (int z = 0; z < 4; ++z)
            if (t0 + z < DP4) { qa[z] = topk_load4<V4>(qrow, t0 + z, D); pb[z] = topk_load4<V4>(prow, t0 + z, D); }
#pragma unroll
        for (int z = 0; z < 4; ++z) {
            if (t0 + z < DP4) {
                float4 q = qa[z];
                if (item_abs) { q.x = fabsf(q.x); q.y = fabsf(q.y); q.z = fabsf(q.z); q.w = fabsf(q.w); }
                const float a0 = h ? q.y : q.x, a1 = h ? q.w : q.z;
                float b0 = h ? pb[z].y : pb[z].x, b1 = h ? pb[z].w : pb[z].z;
                if (ABS_B && item_abs) { b0 = fabsf(b0); b1 = fabsf(b1); }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
            }
        }
    }
    return acc;
}

}  // namespace tfr
