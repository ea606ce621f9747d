// fm_fit.hip - minibatch gather from the FM trainer's resident row store, and the binary metrics of resident predictions
// (fm_fit.h).
//
// The gather of B store rows is four launches on one stream:
//   k_fm_len_sums    per chunk of FM_SCAN_CHUNK batch rows: the sum of their lengths
//   k_fm_chunk_scan  one block: exclusive scan of the chunk sums, indptr[B] = the total
//   k_fm_indptr      per chunk: exclusive scan of the lengths behind the chunk's offset -> indptr, and y
//   k_fm_gather_copy one lane group per batch row: indices and data from the store to [indptr[r], indptr[r + 1])
// All sums are int64 and integer, so the result does not depend on the order they are taken in; nothing is atomic.  The copy
// is bandwidth: consecutive rows land back to back in the outputs, so a wave's lane groups store one contiguous span.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fm_fit.h"
#include "svd_kernels.h"

namespace tfr {

__device__ __forceinline__ int64_t fm_row_len(const FmGatherArgs& a, int64_t r) {
    const int64_t id = a.ids[r];
    return a.sp[id + 1] - a.sp[id];
}

__device__ __forceinline__ int64_t wave_incl_scan(int64_t x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t u = __shfl_up(x, o, 64);
        if (lane >= o) x += u;
    }
    return x;
}

// exclusive scan of one value per thread over the 256-thread block; *total = the block's sum.  wt: 4 words of LDS.
// Every thread of the block must call it (two barriers).
__device__ __forceinline__ int64_t block_excl_scan(int64_t v, int64_t* wt, int64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t inc = wave_incl_scan(v, lane);
    if (lane == 63) wt[wave] = inc;
    __syncthreads();
    const int64_t w0 = wt[0], w1 = wt[1], w2 = wt[2], w3 = wt[3];
    __syncthreads();
    const int64_t before = wave == 0 ? 0 : wave == 1 ? w0 : wave == 2 ? w0 + w1 : w0 + w1 + w2;
    *total = (w0 + w1) + (w2 + w3);
    return before + inc - v;
}

__global__ __launch_bounds__(256) void k_fm_len_sums(FmGatherArgs a) {
    __shared__ int64_t wt[4];
    const int64_t base = (int64_t)blockIdx.x * FM_SCAN_CHUNK;
    int64_t t = 0;
#pragma unroll
    for (int j = 0; j < FM_SCAN_CHUNK / 256; ++j) {
        const int64_t r = base + j * 256 + threadIdx.x;
        if (r < a.B) t += fm_row_len(a, r);
    }
    int64_t total;
    (void)block_excl_scan(t, wt, &total);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_fm_chunk_scan(FmGatherArgs a, int64_t nchunks) {
    __shared__ int64_t wt[4];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nchunks; b0 += 256) {          // block-uniform trip count
        const int64_t i = b0 + threadIdx.x;
        const int64_t v = i < nchunks ? a.blk[i] : 0;
        int64_t total;
        const int64_t ex = block_excl_scan(v, wt, &total);
        if (i < nchunks) a.blk[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a.indptr[a.B] = carry;
}

__global__ __launch_bounds__(256) void k_fm_indptr(FmGatherArgs a) {
    __shared__ int64_t wt[4];
    const int64_t base = (int64_t)blockIdx.x * FM_SCAN_CHUNK;
    int64_t carry = a.blk[blockIdx.x];
#pragma unroll 1
    for (int j = 0; j < FM_SCAN_CHUNK / 256; ++j) {
        const int64_t r = base + j * 256 + threadIdx.x;
        const bool ok = r < a.B;
        int64_t id = 0, v = 0;
        if (ok) {
            id = a.ids[r];
            v = a.sp[id + 1] - a.sp[id];
        }
        int64_t total;
        const int64_t ex = block_excl_scan(v, wt, &total);
        if (ok) {
            a.indptr[r] = carry + ex;
            a.y[r] = a.sy[id];
        }
        carry += total;
    }
}

// G lanes per batch row; rows longer than FM_WIDE_ROUNDS * G entries are left to the whole wave afterwards
template <int G>
__global__ __launch_bounds__(256) void k_fm_gather_copy(FmGatherArgs a) {
    constexpr int RPB = 256 / G;
    const int lane = threadIdx.x & 63, gl = lane % G;
    const int grp = threadIdx.x / G;
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < a.B; base += (int64_t)gridDim.x * RPB) {   // block-uniform trip count
        const int64_t r = base + grp;
        int64_t src = 0, dst = 0, len = 0;
        if (r < a.B) {
            const int64_t id = a.ids[r];
            src = a.sp[id];
            len = a.sp[id + 1] - src;
            dst = a.indptr[r];
        }
        if (dst + len > a.nnz) len = 0;                  // never past the outputs: the host sized them from the same lengths
        const bool wide = G < 64 && len > (int64_t)FM_WIDE_ROUNDS * G;
        if (!wide) {
            for (int64_t k = gl; k < len; k += G) {
                a.indices[dst + k] = a.si[src + k];
                a.data[dst + k] = a.sx[src + k];
            }
        }
        if constexpr (G < 64) {
            uint64_t todo = __ballot(wide && gl == 0);
            while (todo) {                               // wave-uniform
                const int l = __ffsll((unsigned long long)todo) - 1;
                todo &= todo - 1;
                const int64_t ws = __shfl(src, l, 64), wd = __shfl(dst, l, 64), wl = __shfl(len, l, 64);
                for (int64_t k = lane; k < wl; k += 64) {
                    a.indices[wd + k] = a.si[ws + k];
                    a.data[wd + k] = a.sx[ws + k];
                }
            }
        }
    }
}

int fm_gather_group(int64_t B, int64_t nnz) {
    const int64_t mean = B > 0 ? (nnz + B - 1) / B : 0;
    int g = 4;
    while (g < 64 && g < mean) g <<= 1;
    return g;
}

void launch_fm_gather(const FmGatherArgs& a, hipStream_t s) {
    const int64_t nchunks = (a.B + FM_SCAN_CHUNK - 1) / FM_SCAN_CHUNK;
    hipLaunchKernelGGL(k_fm_len_sums, dim3((unsigned)nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_fm_chunk_scan, dim3(1), dim3(256), 0, s, a, nchunks);
    hipLaunchKernelGGL(k_fm_indptr, dim3((unsigned)nchunks), dim3(256), 0, s, a);
    if (a.nnz == 0) return;
    const int G = fm_gather_group(a.B, a.nnz);
    const dim3 grid(blocks_for(a.B, 256 / G, 16384));    // (nnz > 0: at least one row)
    with_one_of<4, 8, 16, 32, 64>(G, [&](auto g) { hipLaunchKernelGGL((k_fm_gather_copy<g.value>), grid, dim3(256), 0, s, a); });
}

// ---- binary metrics of n resident predictions: per block {count of infer == y, summed cross-entropy}, by the formulas of
// the SVD forward's evaluation mode (svd_kernels.h: binary_infer, sigmoid_xent)
__global__ __launch_bounds__(256) void k_fm_binary_metrics(const float* __restrict__ logits, const float* __restrict__ y, int64_t n,
                                                           float* __restrict__ partials) {
    float acc[2] = {0.f, 0.f};
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        const float logit = logits[k], r = y[k];
        acc[0] += (binary_infer(logit) == r) ? 1.f : 0.f;
        acc[1] += sigmoid_xent(logit, r);
    }
    __shared__ float red[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float t = acc[c];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) t += __shfl_down(t, o, 64);
        if (lane == 0) red[wave][c] = t;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int c = threadIdx.x;
        partials[(size_t)blockIdx.x * 2 + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

int fm_metrics_grid(int64_t n) {
    // a block's count of equal predictions is summed in float: keep it far below 2^24
    return blocks_for(n, 256, 8192);
}

void launch_fm_binary_metrics(const float* logits, const float* y, int64_t n, float* partials, hipStream_t s) {
    hipLaunchKernelGGL(k_fm_binary_metrics, dim3(fm_metrics_grid(n)), dim3(256), 0, s, logits, y, n, partials);
}

}  // namespace tfr
