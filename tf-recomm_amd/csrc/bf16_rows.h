// bf16_rows.h - the bf16 snapshot of the two factor tables: format, row layout, lane geometry and launchers
// (bf16_rows.hip).  The Python restatement is tfrecomm_amd/bf16.py.
//
// Element: the upper 16 bits of the float32, rounded to nearest, ties to even.
//   not NaN : (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 - overflow past the largest finite value rounds to +-inf,
//             subnormals round like any other value (no flush)
//   NaN     : (bits >> 16) | 0x40 - sign kept, quiet, never inf
// Widening is bits << 16 and exact; the product of two widened values is exact in float32 (8 + 8 significand bits).
//
// Row: D elements at a stride of DP = 8 * ceil(D / 8) elements, pad elements +0.  Every row is 16-byte aligned and a
// lane's fragment is one 16-byte load of 8 elements; a pad contributes fma(0, 0, x) == x.  Element k of a lane's
// fragment is feature 8 * lane + k: the operand fragment of v_mfma_f32_32x32x16_bf16.  The layout is the library's own.
//
// Geometry: lanes per rating G = the smallest power of two >= DP / 8 (1 ... 32 for D <= 256), a function of D alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

inline int bf16_row_stride(int D) { return 8 * ((D + 7) / 8); }

inline int bf16_geometry(int D) {
    int g = 1;
    while (g * 8 < bf16_row_stride(D)) g <<= 1;
    return g;
}

// ratings in flight per lane group: the forward's 4, held to G so that a wave-iteration's 64 / G * UNR ratings fit the
// 64 lanes of the wave-wide bias load
constexpr int bf16_unroll(int G) { return G < 4 ? G : 4; }

// the forward's argument block without what only training reads; P and Q are snapshot rows of stride DP
struct Bf16FwdArgs {
    const uint16_t* P; const uint16_t* Q; const float* bu; const float* bi; const float* mu;
    const int32_t* u; const int32_t* it; const float* r;
    float* logits; float* partials; int32_t* err;
    int64_t B, U, I;
    int32_t DP, loss, item_abs;
};

// mode: MODE_INFER or MODE_EVAL; grid: forward_grid at bf16_unroll(G); pnt: user rows by non-temporal loads
void launch_forward_bf16(const Bf16FwdArgs& a, int mode, int G, int grid, bool pnt, hipStream_t s);
// float32 [rows, D] -> bf16 [rows, DP], pads included
void launch_rows_to_bf16(const float* src, uint16_t* dst, int64_t rows, int D, hipStream_t s);

}  // namespace tfr
