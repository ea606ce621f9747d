// bf16_rows.hip - gfx950 kernels of the bf16 table snapshot (format and layout: bf16_rows.h): the conversion of a
// float32 table and the gather-dot forward that scores from the converted rows (INFER and EVAL).  A rating then
// costs 2 * DP * 2 bytes of rows instead of 2 * D * 4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svd_kernels.h"
#include "bf16_rows.h"

namespace tfr {
namespace {

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(4))) * cfloat_p;

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

// group_sum, wave_sum and block_sum_store as svd_kernels.hip has them (they are private to that unit): same orders,
// so the EVAL partials are summed as the float32 forward sums its own
template <int G>
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
    return x;   // valid in lane 0
}

template <int NV, int NW>
__device__ __forceinline__ void block_sum_store(float (&val)[NV], float* out) {
    __shared__ float red[NW][NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const float s = wave_sum(val[c]);
        if (lane == 0) red[wave][c] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NW; w += 4) t += (red[w][c] + red[w + 1][c]) + (red[w + 2][c] + red[w + 3][c]);
            out[c] = t;
        }
    }
}

template <bool NT>
__device__ __forceinline__ uintx4 load_frag8(const uint16_t* __restrict__ p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(p));
    else return *reinterpret_cast<const uintx4*>(p);
}

// K1 (svd_kernels.hip forward_body, INFER / EVAL) on snapshot rows.  What differs is the row: a lane group of G lanes
// owns a rating, each lane one 16-byte fragment of 8 bf16 elements of either row, widened by a shift and multiplied
// in float32 - the products are exact, the chain and everything behind it are forward_body's: ids checked into the
// error word and clamped to 0, scalar-path bias loads where a wave holds at most four ratings and the wave-wide
// vector load otherwise, item_abs on the widened item value, the in-lane fmaf chain over the 8 elements ascending,
// group_sum<G>, ((s + mu) + bu) + bi, the EVAL epilogue with its three partials.
// A group wider than the row (G * 8 > DP: lanes 13..15 at D = 100) has lanes without a fragment.  Their load is not
// skipped but aimed at the row's first fragment - a valid address, so the load needs no guard and its registers no
// merge with zeros - and their chain's result is replaced by 0 before the group's sum.
template <int G, int MODE, int UNR, bool PNT>
__global__ __launch_bounds__(256) void k_forward_bf16(Bf16FwdArgs a) {
    warm_args(a);
    constexpr int NW = 4;
    constexpr int SPW = 64 / G;        // ratings per wave per pass; UNR passes in flight
    constexpr bool SBIAS = SPW <= 4;
    constexpr int SPI = SPW * UNR;     // ratings per wave-iteration
    static_assert(SPI <= 64, "the wave-wide bias load holds one rating per lane");
    const int lane = threadIdx.x & 63;
    const int sub = lane / G;
    const int gl = lane % G;
    const int DP = a.DP;
    const bool live = gl * 8 < DP;
    const int d0 = live ? gl * 8 : 0;
    const int Bn = (int)a.B;           // batch positions fit 32 bits (the workspace caps a batch at 2^30 ratings)
    const int wave_id = blockIdx.x * NW + (threadIdx.x >> 6);
    const int stride = gridDim.x * NW * SPI;
    const float mu = *a.mu;

    float acc[3] = {0.f, 0.f, 0.f};    // EVAL: sse, n_equal, nll
    bool oob = false;

    for (int base = wave_id * SPI; base < Bn; base += stride) {
        int k[UNR];
        int32_t u[UNR], it[UNR];
        bool ok[UNR];
        float rr[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            k[j] = base + j * SPW + sub;
            ok[j] = k[j] < Bn;
            u[j] = ok[j] ? a.u[k[j]] : 0;
            it[j] = ok[j] ? a.it[k[j]] : 0;
            rr[j] = (MODE != MODE_INFER && ok[j]) ? a.r[k[j]] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            if ((uint64_t)(int64_t)u[j] >= (uint64_t)a.U) { oob = true; u[j] = 0; }
            if ((uint64_t)(int64_t)it[j] >= (uint64_t)a.I) { oob = true; it[j] = 0; }
        }
        uintx4 p[UNR], q[UNR];
        float bu_[UNR], bi_[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            p[j] = load_frag8<PNT>(a.P + (size_t)u[j] * DP + d0);
            q[j] = load_frag8<false>(a.Q + (size_t)it[j] * DP + d0);
        }
        if constexpr (SBIAS) {
            const cfloat_p cbu = (cfloat_p)(uintptr_t)a.bu;
            const cfloat_p cbi = (cfloat_p)(uintptr_t)a.bi;
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                float xs[SPW], ys[SPW];
#pragma unroll
                for (int s2 = 0; s2 < SPW; ++s2) {
                    xs[s2] = cbu[__builtin_amdgcn_readlane(u[j], s2 * G)];
                    ys[s2] = cbi[__builtin_amdgcn_readlane(it[j], s2 * G)];
                }
                bu_[j] = xs[0]; bi_[j] = ys[0];
#pragma unroll
                for (int s2 = 1; s2 < SPW; ++s2) { if (sub == s2) { bu_[j] = xs[s2]; bi_[j] = ys[s2]; } }
            }
        } else {
            // lane l = j * SPW + s holds rating (j, s) of this iteration (SPI <= 64 ratings): one load per table
            int32_t mu_ = 0, mi_ = 0;
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                const int src = ((lane - j * SPW) & (SPW - 1)) * G;
                const int32_t su = __shfl(u[j], src, 64), si = __shfl(it[j], src, 64);
                if (lane / SPW == j) { mu_ = su; mi_ = si; }
            }
            float wx = 0.f, wy = 0.f;
            if (lane < SPI) { wx = a.bu[mu_]; wy = a.bi[mi_]; }
#pragma unroll
            for (int j = 0; j < UNR; ++j) { bu_[j] = __shfl(wx, j * SPW + sub, 64); bi_[j] = __shfl(wy, j * SPW + sub, 64); }
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const uint32_t pw[4] = {p[j].x, p[j].y, p[j].z, p[j].w};
            const uint32_t qw[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                // elements 2w (low half) and 2w + 1 (high half) of the fragment, widened
                const float p0 = __uint_as_float(pw[w] << 16), p1 = __uint_as_float(pw[w] & 0xffff0000u);
                const float q0 = __uint_as_float(qw[w] << 16), q1 = __uint_as_float(qw[w] & 0xffff0000u);
                s = fmaf(p0, a.item_abs ? fabsf(q0) : q0, s);
                s = fmaf(p1, a.item_abs ? fabsf(q1) : q1, s);
            }
            if (!live) s = 0.f;
            s = group_sum<G>(s);
            const float logit = ((s + mu) + bu_[j]) + bi_[j];      // ops.py:45-47 order
            if (gl == 0 && ok[j]) {
                if constexpr (MODE == MODE_INFER) {
                    a.logits[k[j]] = logit;
                } else {
                    const float r = rr[j];
                    float inf = logit;                 // canonical infer = logits (README.md:33)
                    if (a.loss != 0) inf = binary_infer(logit);       // ops.py:77-78, half-to-even
                    const float d = inf - r;
                    acc[0] += d * d;
                    acc[1] += (inf == r) ? 1.f : 0.f;
                    if (a.loss != 0) acc[2] += sigmoid_xent(logit, r);
                }
            }
        }
    }
    if (oob) atomicOr(a.err, 1);
    if constexpr (MODE != MODE_INFER) block_sum_store<3, NW>(acc, a.partials + (size_t)blockIdx.x * 4);
}

template <int MODE>
void launch_forward_bf16_mode(const Bf16FwdArgs& a, int G, int grid, bool pnt, hipStream_t s) {
#define TFR_BF16_CASE(g, unr)                                                                              \
    if (G == g) {                                                                                          \
        if (pnt) hipLaunchKernelGGL((k_forward_bf16<g, MODE, unr, true>), dim3(grid), dim3(256), 0, s, a); \
        else hipLaunchKernelGGL((k_forward_bf16<g, MODE, unr, false>), dim3(grid), dim3(256), 0, s, a);    \
        return;                                                                                            \
    }
    TFR_BF16_CASE(1, 1) TFR_BF16_CASE(2, 2) TFR_BF16_CASE(4, 4) TFR_BF16_CASE(8, 4) TFR_BF16_CASE(16, 4) TFR_BF16_CASE(32, 4)
#undef TFR_BF16_CASE
}

}  // namespace

int bf16_forward_grid(int64_t B, int G, int mode) {
    const int64_t per_block = 4 * (64 / G) * bf16_unroll(G);   // waves * SPW * UNR
    int64_t nb = (B + per_block - 1) / per_block;
    const int64_t cap = (mode == MODE_INFER) ? 8192 : 2048;    // EVAL: fewer partials to add up
    if (nb > cap) nb = cap;                                    // then grid-stride
    if (nb < 1) nb = 1;
    return (int)nb;
}

void launch_forward_bf16(const Bf16FwdArgs& a, int mode, int G, int grid, bool pnt, hipStream_t s) {
    if (mode == MODE_INFER) launch_forward_bf16_mode<MODE_INFER>(a, G, grid, pnt, s);
    else launch_forward_bf16_mode<MODE_EVAL>(a, G, grid, pnt, s);
}

void launch_rows_to_bf16(const float* src, uint16_t* dst, int64_t rows, int D, hipStream_t s) {
    const int DP = bf16_row_stride(D);
    const int64_t total = rows * (DP / 8);
    int64_t nb = (total + 255) / 256;
    if (nb > 65536) nb = 65536;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_rows_to_bf16, dim3((int)nb), dim3(256), 0, s, src, dst, rows, D, DP);
}

}  // namespace tfr
