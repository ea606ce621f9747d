// score_tile.h - the pieces topk.hip, rank.hip and neighbours.hip share: the 64-bit ordering key of a scored pair, the one-wave
// bitonic sort of keys in LDS, the queue compaction built on it, the MFMA tile that scores 32 items against 32 user
// columns (on float32 rows, and on the bf16 snapshot's), and sliced_topk_block, the whole scoring block of k_topk_score,
// k_nb_score, k_topk_score_bf16 and k_nb_score_bf16, which differ only in their scorer.
// The rank kernels' bodies, generic over a scorer in the same way, are in rank_body.h.
//
// key(s, item) = (order-preserving uint32 of s) << 32 | ~item: one 64-bit compare orders by score descending, then item id
// ascending; every non-NaN score gives a key above 0, so key 0 marks an empty slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svd_kernels.h"
#include "topk.h"

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

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The same tile on rows of the bf16 snapshot (bf16_rows.h: uint16_t rows at a stride of DP = 8 * ceil(D / 8), 16-byte aligned,
// pads +0), with the same return contract.  A row is NF = DP / 8 fragments of 8 elements, each the operand fragment of
// v_mfma_f32_32x32x16_bf16 as it stands: step s = 0 .. ceil(NF / 2) - 1 gives fragment 2 s + h of the candidate row as A
// (sign bits cleared with item_abs: the bits of fabsf on the widened value) and of the query row as B, one 16-byte load each,
// steps ascending from a zero accumulator, loaded in groups of four steps ahead of their MFMAs.  With NF odd the upper
// half-wave has no fragment in the last step: its loads are aimed at the row's first fragment - a valid address, no load
// is guarded - and both operands are replaced by zero afterwards; one side alone would leave 0 * inf = NaN from
// the redirected fragment in every score of the tile.
// ABS_B (bf16_neighbours.hip: both operands are rows of the one snapshot table): item_abs clears the sign bits of the B
// fragments too; the zeroing of the missing half-fragment stays on both sides.
template <bool ABS_B = false>
__device__ __forceinline__ f32x16 mfma_tile_dot_bf16(const uint16_t* qrow, const uint16_t* prow, int DP, int item_abs, int h) {
    const int NF = DP >> 3, steps = (NF + 1) >> 1;
    const u32x4* qf = reinterpret_cast<const u32x4*>(qrow);
    const u32x4* pf = reinterpret_cast<const u32x4*>(prow);
    const uint32_t keep = item_abs ? 0x7fff7fffu : 0xffffffffu;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int s0 = 0; s0 < steps; s0 += 4) {
        u32x4 qa[4], pb[4];
#pragma unroll
        for (int z = 0; z < 4; ++z)
            if (s0 + z < steps) {
                const int f = 2 * (s0 + z) + h;
                const int at = f < NF ? f : 0;
                qa[z] = qf[at];
                pb[z] = pf[at];
            }
#pragma unroll
        for (int z = 0; z < 4; ++z) {
            if (s0 + z < steps) {
                const bool has = 2 * (s0 + z) + h < NF;
                const u32x4 a = has ? qa[z] & keep : (u32x4)0u;
                const u32x4 b = has ? (ABS_B ? pb[z] & keep : pb[z]) : (u32x4)0u;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc,
                                                              0, 0, 0);
            }
        }
    }
    return acc;
}

// The scoring block of "the best k candidates by a tile score" (k_topk_score, k_nb_score and their bf16 twins).  A block owns a
// tile of UPB query rows (the 32 columns of a 32x32 MFMA tile) and one slice of the candidates [cand_lo, cand_hi).  Every
// round each of its 4 waves scores a 32-candidate sub-tile against the tile's queries and appends the keys that beat its query's running k-th key
// (and are eligible, not NaN and not excluded, tested in that order) to that query's LDS queue.  Between rounds a queue that
// could not take another round is sorted (bitonic, one wave), cut to k and its threshold raised.  At the end every queue is
// sorted and its first k keys go to part[row, slice].  Query ids outside [0, id_rows) set err bit 0 and score nothing.
// Scorer(a, qid) is built once per lane: tile<V4>(cand, h) (the tile of the lane's candidate row against its query row: the
// scorer picks the row format and with it the MFMA), eligible(cand), score(dot, cand).
template <int UPB, int CAP, bool V4, class Scorer, class Args>
__device__ __forceinline__ void sliced_topk_block(const Args& a, int64_t id_rows, int64_t cand_lo, int64_t cand_hi) {
    __shared__ uint64_t queue[UPB * CAP];
    __shared__ uint64_t thr[UPB];
    __shared__ int32_t cnt[UPB];
    static_assert(sizeof(queue) + sizeof(thr) + sizeof(cnt) == topk_score_static_lds(UPB, CAP),
                  "topk_plan reports a different LDS size than the block declares");
    static_assert(CAP - TOPK_ROUND >= (CAP == 256 ? 128 : TOPK_KMAX), "a queue must hold k plus one round of appends");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int j = c & (UPB - 1);                       // query of this lane's accumulator column
    const bool own_col = c < UPB;                      // UPB 16: columns 16..31 repeat 0..15 and select nothing
    const int64_t row = (int64_t)blockIdx.x * UPB + j;
    const int slice = blockIdx.y;
    const int k = a.k;

    int32_t qid = -1;
    if (row < a.n_rows) {
        qid = a.rows[row];
        if (qid < 0 || (int64_t)qid >= id_rows) {
            if (own_col && h == 0) atomicOr(a.err, 1);
            qid = -1;
        }
    }
    const bool live = own_col && qid >= 0;
    int64_t xlo = 0, xhi = 0;
    if (live && a.indptr && *a.excl_bad == 0) { xlo = a.indptr[row]; xhi = a.indptr[row + 1]; }
    const Scorer sc(a, qid);
    for (int t = threadIdx.x; t < UPB; t += 256) { cnt[t] = 0; thr[t] = 0; }
    __syncthreads();

    const int64_t n_cand = cand_hi - cand_lo;
    const int64_t per = ((n_cand + a.slices - 1) / a.slices + TOPK_ROUND - 1) / TOPK_ROUND * TOPK_ROUND;
    const int64_t s_lo = cand_lo + (int64_t)slice * per;
    const int64_t s_hi = s_lo + per < cand_hi ? s_lo + per : cand_hi;
    const int64_t rounds = s_hi > s_lo ? (s_hi - s_lo + TOPK_ROUND - 1) / TOPK_ROUND : 0;

    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t base = s_lo + rd * TOPK_ROUND + wave * TOPK_SUB;
        int64_t my_cand = base + c;                    // A row = candidate; past the slice: a row inside it, result dropped
        if (my_cand >= s_hi) my_cand = s_hi - 1;
        const f32x16 acc = sc.template tile<V4>(my_cand, h);
        // C[candidate row][query column]: this lane holds query j, candidates base + (r&3) + 8(r>>2) + 4h
        const uint64_t th = thr[j];
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t cand = base + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (cand < s_hi && sc.eligible(cand)) {
                    const float s = sc.score(acc[r], cand);
                    if (!__builtin_isnan(s)) {
                        const uint64_t key = topk_key(s, cand);
                        if (key > th && !(xhi > xlo && topk_excluded(a.excl, xlo, xhi, (int32_t)cand))) {
                            const int pos = atomicAdd(&cnt[j], 1);
                            queue[j * CAP + pos] = key;
                        }
                    }
                }
            }
        }
        __syncthreads();
        for (int u = wave; u < UPB; u += TOPK_WAVES)
            if (cnt[u] > CAP - TOPK_ROUND) topk_compact<CAP>(queue + u * CAP, cnt + u, thr + u, k, lane);
        __syncthreads();
    }
    for (int u = wave; u < UPB; u += TOPK_WAVES) {
        const int64_t rw = (int64_t)blockIdx.x * UPB + u;
        if (rw >= a.n_rows) continue;
        if (cnt[u] > 0) topk_compact<CAP>(queue + u * CAP, cnt + u, thr + u, k, lane);
        const int n = cnt[u];
        uint64_t* dst = a.part + ((size_t)rw * a.slices + slice) * k;
        for (int q = lane; q < k; q += 64) dst[q] = q < n ? queue[u * CAP + q] : 0;
    }
}

// launches the instantiation of a score kernel that the plan's queue capacity and the row width pick
template <class Args>
static void launch_score_kernel(void (*k32v)(Args), void (*k32)(Args), void (*k16v)(Args), void (*k16)(Args), const Args& a,
                                const TopkPlan& p, hipStream_t s) {
    const dim3 g((unsigned)((a.n_rows + p.upb - 1) / p.upb), (unsigned)p.slices);
    const bool v4 = (a.D & 3) == 0;
    hipLaunchKernelGGL(p.cap == 256 ? (v4 ? k32v : k32) : (v4 ? k16v : k16), g, dim3(256), 0, s, a);
}

}  // namespace tfr
