// fm_bf16.hip - k_fm_forward (fm_kernels.hip) in its inference form on the bf16 snapshot's rows (bf16_rows.h):
//     y(x) = mu + x.W + 0.5 * ( ||x V||^2 - sum_j x_j^2 ||V_j||^2 ),   V widened from bf16, everything else float32.
// One lane group of G = bf16_geometry(D) lanes per CSR row; a lane owns one 16-byte fragment (8 elements) of every V row
// the CSR row names, and the row's non-zeros are walked four at a time, so four 2*DP-byte row gathers are in flight per
// group.  A non-zero then costs 2 * DP bytes of row instead of 4 * D.  The arithmetic per element, the order of the
// reductions and the output expression are k_fm_forward's; only the lane geometry differs (8 elements per lane).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svd_kernels.h"
#include "bf16_rows.h"
#include "fm_bf16.h"

namespace tfr {
namespace {

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// A group wider than the row (G * 8 > DP: lanes 13..15 at D = 100) has lanes without a fragment.  Their loads are aimed at
// the row's first fragment - an address that exists, so no load is guarded - and their share of the sum is replaced by 0
// before the group's reduction (Bf16Rows::load, bf16_rows.hip).
// Eight waves per SIMD, k_fm_forward's inference occupancy: s and q are 16 registers here against its 8.
template <int G, bool NTV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fm_forward_bf16(FmBf16Args a) {
    warm_args(a);
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int DP = a.DP;
    const bool live = gl * 8 < DP;
    const int d0 = live ? gl * 8 : 0;
    const float mu = *a.mu;
    bool oob = false;
    for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < a.n_rows;
         row += (int64_t)gridDim.x * GPB) {
        const int64_t lo = a.indptr[row], hi = a.indptr[row + 1];
        float s[8], q[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
        float lin = 0.f;
        for (int64_t p = lo; p < hi; p += 4) {
            int32_t f[4];
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                // branch-free: an address that is there, the value dropped below
                const int64_t pj = p + j < hi ? p + j : hi - 1;
                f[j] = a.indices[pj];
                x[j] = a.data[pj];
            }
            // Two fences for the scheduler: the eight loads above issue together, and so do the eight below.  Held to 64
            // VGPRs without them it issued the index / value pairs one after the other, a round trip each (ISA:
            // global_load_dword x2 / s_waitcnt vmcnt(0), four times); free of the bound it took 73-83 VGPRs, 5-6 waves.
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!(p + j < hi)) { f[j] = 0; x[j] = 0.f; }
                if ((uint64_t)(int64_t)f[j] >= (uint64_t)a.F) { oob = true; f[j] = 0; x[j] = 0.f; }
            }
            float w[4];
            uintx4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = a.W[f[j]];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uintx4* vr = reinterpret_cast<const uintx4*>(a.V + (size_t)f[j] * DP + d0);
                if constexpr (NTV) v[j] = __builtin_nontemporal_load(vr);
                else v[j] = *vr;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t vw[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // element e of the fragment: the low (even e) or high half of word e / 2, widened by a shift - exact
                    const float ve = __uint_as_float((e & 1) ? (vw[e >> 1] & 0xffff0000u) : (vw[e >> 1] << 16));
                    const float xv = x[j] * ve;          // a pad: x * (+0), fma(0, 0, q) == q
                    s[e] += xv;
                    q[e] = fmaf(xv, xv, q[e]);
                }
                lin = fmaf(x[j], w[j], lin);
            }
        }
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += s[e] * s[e] - q[e];
        acc = live ? acc : 0.f;
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
        const float yhat = (mu + lin) + 0.5f * acc;
        if (gl == 0) a.out[row] = yhat;
    }
    if (oob) atomicOr(a.err, 1);
}

}  // namespace

int fm_bf16_grid(int64_t n_rows, int G) { return blocks_for(n_rows, 256 / G, 8192); }     // fm_grid's inference cap

void launch_fm_bf16(const FmBf16Args& a, int G, int grid, bool ntv, hipStream_t s) {
    with_one_of<1, 2, 4, 8, 16, 32>(G, [&](auto g) {
        with_bool(ntv, [&](auto nt) {
            hipLaunchKernelGGL((k_fm_forward_bf16<g.value, nt.value>), dim3(grid), dim3(256), 0, s, a);
        });
    });
}

}  // namespace tfr
