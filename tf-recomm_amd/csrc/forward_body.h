// forward_body.h - K1, the gather-dot forward, written once for every row format (private to svd_kernels.hip and
// bf16_rows.hip), with the fragment and the reductions it is built on.  A row type supplies what differs between
// formats - the argument block, the elements per lane, the fragment with its load and the in-lane chain; float32 rows
// are Float32Rows below, snapshot rows Bf16Rows in bf16_rows.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svd_kernels.h"

namespace tfr {

template <int VEC> struct Frag { float v[VEC]; };

typedef float floatx4 __attribute__((ext_vector_type(4)));

// NT: non-temporal (streaming) load - rows that are read once should not displace the
// small, re-used tables (biases, ids) from L2 / Infinity Cache.
template <int VEC, bool NT = false>
__device__ __forceinline__ Frag<VEC> load_frag(const float* __restrict__ row, int d0, int D) {
    Frag<VEC> f;
    if constexpr (VEC == 4) {
        if (d0 < D) {
            floatx4 t;
            if constexpr (NT) t = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(row + d0));
            else t = *reinterpret_cast<const floatx4*>(row + d0);
            f.v[0] = t.x; f.v[1] = t.y; f.v[2] = t.z; f.v[3] = t.w;
        } else {
            f.v[0] = f.v[1] = f.v[2] = f.v[3] = 0.f;
        }
    } else {
        if constexpr (NT) f.v[0] = (d0 < D) ? __builtin_nontemporal_load(row + d0) : 0.f;
        else f.v[0] = (d0 < D) ? row[d0] : 0.f;
    }
    return f;
}

template <int G>
__device__ __forceinline__ float group_sum(float x) {
    // butterfly over the G lanes of a group (G is a power of two <= 64); every lane of the
    // group ends with the same sum, in a fixed order -> deterministic.
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// The same reduction staged through LDS memory instead of the cross-lane network: every lane
// parks its partial in LDS, the group's first lane reads the G values back as 16-byte vectors and
// adds them in lane order.  Kept for the A/B recorded in DESIGN.md (the butterfly is the default).
template <int G>
__device__ __forceinline__ float group_sum_lds(float x, float* wave_slot /* 64 floats of this wave */, int lane) {
    wave_slot[lane] = x;
    __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0): the wave's own LDS writes have landed
    const int g0 = lane & ~(G - 1);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < G; q += 4) {
        const float4 v = *reinterpret_cast<const float4*>(wave_slot + g0 + q);
        s += (v.x + v.y) + (v.z + v.w);
    }
    return s;
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
    return x;   // valid in lane 0
}

// block-level sum of NV values per thread -> out[NV] written by thread 0.  NW waves per block.
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

// float32 rows, VEC floats per lane (svd_kernels.hip: the row geometry)
template <int VEC>
struct Float32Rows {
    typedef FwdArgs Args;
    typedef Frag<VEC> Fragment;
    static constexpr int EPL = VEC;                  // elements per lane
    static constexpr bool STEP_ARGS = true;          // Args carries what the training steps add (forward_body)
    static __device__ __forceinline__ int width(const Args& a) { return a.D; }
    template <bool NT>
    static __device__ __forceinline__ Fragment load(const float* __restrict__ row, int d0, int D) {
        return load_frag<VEC, NT>(row, d0, D);
    }
    // the lane's share of the dot product; TRAIN: + its share of the regulariser's squares in sq
    template <int MODE>
    static __device__ __forceinline__ float chain(const Fragment& p, const Fragment& q, int item_abs, bool, float& sq) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float qv = q.v[e];
            s = fmaf(p.v[e], item_abs ? fabsf(qv) : qv, s);
            if constexpr (MODE == MODE_TRAIN) sq = fmaf(p.v[e], p.v[e], fmaf(qv, qv, sq));
        }
        return s;
    }
};

// ------------------------------------------------------------------------------------
// K1  gather-dot forward (ops.py:13-14,37-38 embedding_lookup x4; ops.py:44-47 dot + biases)
//     MODE_INFER: logits only                          (svd_train_val.py:120-122)
//     MODE_TRAIN: + g = dcost/dlogit, per-block partial {data loss, regulariser, sum g}
//                 (ops.py:81-89 regulariser over gathered rows; ops.py:124 / 125-126 loss)
//     MODE_EVAL : per-block partial {sum (infer-rate)^2, count infer==rate}
//                 (svd_train_val.py:144-149)
// A lane group owns one rating at a time; UNR ratings are in flight per group so each
// lane has 2*UNR independent 16-byte loads outstanding.
// Bias gathers take the SCALAR path where a wave holds few ratings (SPW <= 4, i.e. D >= 64): the ids come
// out of the lanes by v_readlane and the 4-byte loads go through the scalar cache, so they do not queue
// behind the row gathers in the vector memory pipeline.  Measured on the north-star shape
// (tools/probes/fwd_shape.hip): per-group vector loads 45.6 us, scalar 42.9 us per 262144 ratings.  The
// arrays are read-only for the whole launch (constant address space = s_load).  Narrow rows (SPW >= 8) use
// one wave-wide vector load per table instead: lane j fetches the bias of the wave's j-th rating.
//
// Row::STEP_ARGS is the one switch between the two argument blocks.  What only FwdArgs has - the store gather with
// u_out / it_out, dB, qstride, bistride, lds_reduce, the kept EVAL logits and all of TRAIN - is compiled behind it, so
// an instantiation on the snapshot's block reads none of it and keeps its argument SGPRs.
typedef const float __attribute__((address_space(4))) * cfloat_p;

template <class Row, int G, int MODE, int UNR, int NW, bool PNT = false>
__device__ __forceinline__ void forward_body(const typename Row::Args& a, int block, int nblocks) {
    constexpr bool STEP = Row::STEP_ARGS;
    static_assert(STEP || MODE != MODE_TRAIN, "TRAIN reads the training steps' arguments");
    constexpr int SPW = 64 / G;        // ratings per wave per pass; UNR passes in flight
    constexpr bool SBIAS = SPW <= 4;
    constexpr int SPI = SPW * UNR;     // ratings per wave-iteration
    static_assert(SPI <= 64, "the wave-wide bias load holds one rating per lane");
    const int lane = threadIdx.x & 63;
    const int sub = lane / G;
    const int gl = lane % G;
    const int d0 = gl * Row::EPL;
    const int D = Row::width(a);
    // batch positions fit 32 bits (the workspace caps a batch at 2^30 ratings)
    int Bn, bis;
    size_t qs;
    if constexpr (STEP) {
        Bn = a.dB ? *a.dB : (int)a.B;                   // row-sharded step: the local batch size lives on the device
        qs = a.qstride ? (size_t)a.qstride : (size_t)D; // item rows may sit in a packed exchange buffer
        bis = a.bistride ? a.bistride : 1;
    } else {
        Bn = (int)a.B; qs = (size_t)D; bis = 1;
    }
    const int wave_id = block * NW + (threadIdx.x >> 6);
    const int stride = nblocks * NW * SPI;
    const float mu = *a.mu;

    float acc[3] = {0.f, 0.f, 0.f};    // TRAIN: loss, reg, sum g | EVAL: sse, n_equal, nll
    bool oob = false, oob_store = false;

    // TRAIN (few, fat blocks: k_front, the sharded step): the ids of iteration n+1 are fetched while the rows
    // of iteration n are in flight, so the only exposed round trip per iteration is the row gather itself.
    // INFER / EVAL fetch them at the top of the iteration instead: without the second id set the kernel fits
    // 64 VGPRs = 8 waves per SIMD, and the extra waves hide that round trip better than the prefetch did
    // (north-star shape, one 262144-rating batch per launch: 51.0 -> 43.4 us together with the scalar-path
    // bias loads and the non-temporal user rows; holding the kernel to 80 SGPRs for an eighth wave per SIMD
    // changed nothing - gpurun_out/ns_s80_*.json; tools/probes/fwd_shape.hip).
    constexpr bool PF = MODE == MODE_TRAIN;
    int32_t u_n[UNR], it_n[UNR];
    float rr_n[UNR];
    auto fetch_ids = [&](int base) {
        if constexpr (STEP) {
            if (a.ids) {
                // fused ShuffleIterator gather (dataio.py:115-117): id -> (user, item, rate) from the
                // HBM-resident store
                int64_t id[UNR];
#pragma unroll
                for (int j = 0; j < UNR; ++j) {
                    const int k = base + j * SPW + sub;
                    id[j] = (k < Bn) ? a.ids[k] : 0;
                    if ((uint64_t)id[j] >= (uint64_t)a.N) { oob_store = true; id[j] = 0; }
                }
#pragma unroll
                for (int j = 0; j < UNR; ++j) {
                    const int4 rec = a.store[id[j]];          // one 16-byte record: {user, item, rate bits, -}
                    u_n[j] = rec.x;
                    it_n[j] = rec.y;
                    rr_n[j] = __int_as_float(rec.z);
                }
                return;
            }
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int k = base + j * SPW + sub;
            const bool ok = k < Bn;
            u_n[j] = ok ? a.u[k] : 0;
            it_n[j] = ok ? a.it[k] : 0;
            rr_n[j] = (MODE != MODE_INFER && ok) ? a.r[k] : 0.f;
        }
    };

    int base = wave_id * SPI;
    if (PF && base < Bn) fetch_ids(base);
    for (; base < Bn; base += stride) {
        if (!PF) fetch_ids(base);
        int k[UNR];
        int32_t u[UNR], it[UNR];
        bool ok[UNR];
        float rr[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            k[j] = base + j * SPW + sub;
            ok[j] = k[j] < Bn;
            u[j] = u_n[j]; it[j] = it_n[j]; rr[j] = rr_n[j];
            if constexpr (STEP) {
                if (a.ids && a.u_out && gl == 0 && ok[j]) { a.u_out[k[j]] = u[j]; a.it_out[k[j]] = it[j]; }   // kept for the backward
            }
            if ((uint64_t)(int64_t)u[j] >= (uint64_t)a.U) { oob = true; u[j] = 0; }
            if ((uint64_t)(int64_t)it[j] >= (uint64_t)a.I) { oob = true; it[j] = 0; }
        }
        typename Row::Fragment p[UNR], q[UNR];
        float bu_[UNR], bi_[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            p[j] = Row::template load<PNT>(a.P + (size_t)u[j] * D, d0, D);
            q[j] = Row::template load<false>(a.Q + (size_t)it[j] * qs, d0, D);
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
                    ys[s2] = cbi[(size_t)__builtin_amdgcn_readlane(it[j], s2 * G) * bis];
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
            if (lane < SPI) { wx = a.bu[mu_]; wy = a.bi[(size_t)mi_ * bis]; }
#pragma unroll
            for (int j = 0; j < UNR; ++j) { bu_[j] = __shfl(wx, j * SPW + sub, 64); bi_[j] = __shfl(wy, j * SPW + sub, 64); }
        }
        if (PF && base + stride < Bn) fetch_ids(base + stride);      // next iteration's ids, behind the rows
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            float sq = 0.f;
            float s = Row::template chain<MODE>(p[j], q[j], a.item_abs, d0 < D, sq);
            bool via_lds = false;
            if constexpr (STEP) via_lds = a.lds_reduce;
            if (via_lds) {
                __shared__ float stage[NW][64];
                s = group_sum_lds<G>(s, stage[threadIdx.x >> 6], lane);
            } else {
                s = group_sum<G>(s);
            }
            const float logit = ((s + mu) + bu_[j]) + bi_[j];      // ops.py:45-47 order
            if (gl == 0 && ok[j]) {
                if constexpr (MODE == MODE_INFER) {
                    a.logits[k[j]] = logit;
                } else if constexpr (MODE == MODE_TRAIN) {
                    if (a.logits) a.logits[k[j]] = logit;
                    const float r = rr[j];
                    float g, l;
                    if (a.loss == 0) {                 // ops.py:124  l2_loss(infer - rate)
                        g = logit - r;
                        l = 0.5f * g * g;
                    } else {                           // ops.py:125-126 sigmoid cross-entropy
                        g = sigmoidf_(logit) - r;
                        l = fmaxf(logit, 0.f) - logit * r + log1pf(__expf(-fabsf(logit)));
                    }
                    a.g[k[j]] = g;
                    acc[0] += l;
                    acc[2] += g;
                    if (a.reg_bias) sq = fmaf(bu_[j], bu_[j], fmaf(bi_[j], bi_[j], sq));
                } else {
                    const float r = rr[j];
                    float inf = logit;                 // canonical infer = logits (README.md:33)
                    if (a.loss != 0) inf = binary_infer(logit);       // ops.py:77-78, half-to-even
                    const float d = inf - r;
                    acc[0] += d * d;
                    acc[1] += (inf == r) ? 1.f : 0.f;
                    // svd_train_val.py:94,170-178: the epoch line's mean NLL (ops.py:125-126 on the fed logits)
                    if (a.loss != 0) acc[2] += sigmoid_xent(logit, r);
                    if constexpr (STEP) {
                        if (a.logits) a.logits[k[j]] = logit;            // kept for the AUC (rank sum over the sorted logits)
                    }
                }
            }
            if constexpr (MODE == MODE_TRAIN) {
                if (ok[j]) acc[1] += 0.5f * sq;        // tf.nn.l2_loss = sum(x^2)/2
            }
        }
    }
    if (oob) atomicOr(a.err, 1);
    if (oob_store) atomicOr(a.err, 2);
    if constexpr (MODE != MODE_INFER) block_sum_store<3, NW>(acc, a.partials + (size_t)block * 4);
}

}  // namespace tfr
