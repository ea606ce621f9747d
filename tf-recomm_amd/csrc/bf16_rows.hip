// bf16_rows.hip - gfx950 kernels of the bf16 table snapshot (format and layout: bf16_rows.h): the conversion of a
// float32 table, and the snapshot's row type for the gather-dot forward (forward_body.h, the body the float32
// forward runs) with its INFER and EVAL kernels.  A rating then costs 2 * DP * 2 bytes of rows instead of 2 * D * 4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svd_kernels.h"
#include "forward_body.h"
#include "bf16_rows.h"

namespace tfr {
namespace {

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// the rule of bf16_rows.h on one float32 bit pattern
__device__ __forceinline__ uint32_t bf16_bits(float x) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (b >> 16) | 0x40u;
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

// One thread converts one 8-element group: 32 bytes in (two 16-byte loads where D % 4 == 0), one 16-byte store out.
// Elements at and past D are the row's pad: +0.
__global__ __launch_bounds__(256) void k_rows_to_bf16(const float* __restrict__ src, uint16_t* __restrict__ dst,
                                                      int64_t rows, int D, int DP) {
    const int gpr = DP / 8;
    const int64_t total = rows * gpr;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t row = g / gpr;
        const int c = (int)(g - row * gpr) * 8;
        const float* in = src + (size_t)row * D + c;
        float v[8];
        if (D % 4 == 0) {
            const float4 lo = *reinterpret_cast<const float4*>(in);                       // c < D: the group exists
            const float4 hi = (c + 4 < D) ? *reinterpret_cast<const float4*>(in + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
            v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (c + e < D) ? in[e] : 0.f;
        }
        uintx4 o;
        o.x = bf16_bits(v[0]) | (bf16_bits(v[1]) << 16);
        o.y = bf16_bits(v[2]) | (bf16_bits(v[3]) << 16);
        o.z = bf16_bits(v[4]) | (bf16_bits(v[5]) << 16);
        o.w = bf16_bits(v[6]) | (bf16_bits(v[7]) << 16);
        *reinterpret_cast<uintx4*>(dst + (size_t)g * 8) = o;
    }
}

// Snapshot rows for forward_body: a lane owns one 16-byte fragment of 8 bf16 elements of either row, widened by a shift
// and multiplied in float32 - the products are exact.  A group wider than the row (G * 8 > DP: lanes 13..15 at
// D = 100) has lanes without a fragment.  Their load is not skipped but aimed at the row's first fragment - a valid
// address, so the load needs no guard and its registers no merge with zeros - and their chain's result is replaced by
// 0 before the group's sum.
struct Bf16Rows {
    typedef Bf16FwdArgs Args;
    typedef uintx4 Fragment;
    static constexpr int EPL = 8;
    static constexpr bool STEP_ARGS = false;         // Bf16FwdArgs: no training arguments, so INFER keeps eight waves per SIMD
    static __device__ __forceinline__ int width(const Args& a) { return a.DP; }
    template <bool NT>
    static __device__ __forceinline__ Fragment load(const uint16_t* __restrict__ row, int d0, int DP) {
        const uintx4* p = reinterpret_cast<const uintx4*>(row + (d0 < DP ? d0 : 0));
        if constexpr (NT) return __builtin_nontemporal_load(p);
        else return *p;
    }
    // the 8 elements ascending; item_abs on the widened item value
    template <int MODE>
    static __device__ __forceinline__ float chain(const Fragment& p, const Fragment& q, int item_abs, bool live, float&) {
        const uint32_t pw[4] = {p.x, p.y, p.z, p.w};
        const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            // elements 2w (low half) and 2w + 1 (high half) of the fragment, widened
            const float p0 = __uint_as_float(pw[w] << 16), p1 = __uint_as_float(pw[w] & 0xffff0000u);
            const float q0 = __uint_as_float(qw[w] << 16), q1 = __uint_as_float(qw[w] & 0xffff0000u);
            s = fmaf(p0, item_abs ? fabsf(q0) : q0, s);
            s = fmaf(p1, item_abs ? fabsf(q1) : q1, s);
        }
        return live ? s : 0.f;
    }
};

// K1 (forward_body.h) on snapshot rows, INFER and EVAL
template <int G, int MODE, int UNR, bool PNT>
__global__ __launch_bounds__(256) void k_forward_bf16(Bf16FwdArgs a) {
    warm_args(a);
    forward_body<Bf16Rows, G, MODE, UNR, 4, PNT>(a, blockIdx.x, gridDim.x);
}

template <int MODE>
void launch_forward_bf16_mode(const Bf16FwdArgs& a, int G, int grid, bool pnt, hipStream_t s) {
    with_one_of<1, 2, 4, 8, 16, 32>(G, [&](auto g) {
        with_bool(pnt, [&](auto nt) {
            hipLaunchKernelGGL((k_forward_bf16<g.value, MODE, bf16_unroll(g.value), nt.value>), dim3(grid), dim3(256), 0, s, a);
        });
    });
}

}  // namespace

void launch_forward_bf16(const Bf16FwdArgs& a, int mode, int G, int grid, bool pnt, hipStream_t s) {
    if (mode == MODE_INFER) launch_forward_bf16_mode<MODE_INFER>(a, G, grid, pnt, s);
    else launch_forward_bf16_mode<MODE_EVAL>(a, G, grid, pnt, s);
}

void launch_rows_to_bf16(const float* src, uint16_t* dst, int64_t rows, int D, hipStream_t s) {
    const int DP = bf16_row_stride(D);
    const int64_t total = rows * (DP / 8);
    hipLaunchKernelGGL(k_rows_to_bf16, dim3(blocks_for(total, 256, 65536)), dim3(256), 0, s, src, dst, rows, D, DP);
}

}  // namespace tfr
