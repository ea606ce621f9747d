// rank.hip - rank held-out items over the whole catalogue on gfx950.
//
// Every key is scored by the MFMA tile of topk.hip (score_tile.h), so a target, an excluded item and a counted item get the
// same bits for the same pair, and the same bits tfr_topk ranks by.
// k_rank_targets: one wave per piece.  Scores the piece's targets, marks a NaN or excluded target unranked (key 0), sorts
//   the keys descending (bitonic, LDS), records the position of each sorted key's target, and starts the piece's bins at
//   minus the excluded items: every distinct excluded item with a non-NaN score is binned as k_rank_count bins it, and taken
//   off.  Writes -1 to the piece's ranks (the unranked stay so).
// k_rank_count: a block owns 32 pieces (the B columns of v_mfma_f32_32x32x2_f32) and one item slice.  A pair whose key
//   beats the piece's lowest ranked target adds 1 to bin p = #{targets with key >= it} (binary search of the sorted keys in
//   LDS, LDS integer atomic).  The block adds its bins to the piece's with global integer atomics.
// k_rank_finish: one wave per piece: rank of sorted target j = bins[0] + ... + bins[j], scattered to the target's position.
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "rank.h"

namespace tfr {

// first j in [0, nr) with q[j] < key, given q[0..nr) descending and q[nr-1] < key: the number of targets whose key is >= key
__device__ __forceinline__ int rank_bin(const uint64_t* q, int nr, uint64_t key) {
    int lo = 0, hi = nr - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] < key) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <bool V4>
__global__ __launch_bounds__(256) void k_rank_targets(RankArgs a) {
    __shared__ uint64_t keys[RANK_WAVES * RANK_CAP];
    __shared__ int32_t bins[RANK_WAVES * RANK_CAP];
    __shared__ float sc[RANK_WAVES * RANK_SUB];
    static_assert(sizeof(keys) + sizeof(bins) + sizeof(sc) == rank_targets_static_lds(),
                  "tfr_rank_plan reports a different LDS size than k_rank_targets declares");
    static_assert(RANK_CAP % 64 == 0 && RANK_SUB == 32, "a wave sorts RANK_CAP keys and scores 32 items a tile");
    warm_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int64_t pc = (int64_t)blockIdx.x * RANK_WAVES + wave;
    if (pc >= a.n_pieces) return;                      // the whole wave: no block barrier below
    const RankPiece p = a.pieces[pc];
    uint64_t* kq = keys + wave * RANK_CAP;
    int32_t* bq = bins + wave * RANK_CAP;
    float* sq = sc + wave * RANK_SUB;
    const int32_t* tg = a.tgt + p.tlo;
    const float* prow = a.P + (int64_t)p.user * a.D;
    const float mu = *a.mu;
    const float ub = a.bu[p.user];
    for (int t = lane; t < RANK_CAP; t += 64) { kq[t] = 0; bq[t] = 0; }
    for (int t = lane; t < p.nt; t += 64) a.ranks[p.tlo + t] = -1;
    wave_lds_sync();

    for (int t0 = 0; t0 < p.nt; t0 += RANK_SUB) {
        const int ti = t0 + c < p.nt ? t0 + c : p.nt - 1;    // A row = target; past the piece: one inside it, dropped
        const f32x16 acc = mfma_tile_dot<V4>(a.Q + (int64_t)tg[ti] * a.D, prow, a.D, a.item_abs, h);
        if (c == 0) {                                  // every column is the piece's user: column 0 has all 32 rows
#pragma unroll
            for (int r = 0; r < 16; ++r) sq[(r & 3) + 8 * (r >> 2) + 4 * h] = acc[r];
        }
        wave_lds_sync();
        if (lane < RANK_SUB && t0 + lane < p.nt) {
            const int32_t item = tg[t0 + lane];
            const float s = ((sq[lane] + mu) + ub) + a.bi[item];
            const bool out = __builtin_isnan(s) || (p.xhi > p.xlo && topk_excluded(a.excl, p.xlo, p.xhi, item));
            kq[t0 + lane] = out ? 0 : topk_key(s, item);
        }
        wave_lds_sync();
    }
    wave_sort_desc<RANK_CAP>(kq, lane);
    int nz = 0;
    for (int t = lane; t < RANK_CAP; t += 64) nz += kq[t] != 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nz += __shfl_xor(nz, off);
    const int nr = nz;                                 // the ranked targets lead the sorted keys
    uint64_t* gk = a.keys + pc * RANK_CAP;
    int32_t* go = a.order + pc * RANK_CAP;
    for (int t = lane; t < RANK_CAP; t += 64) {
        const uint64_t key = kq[t];
        gk[t] = key;
        if (t < nr) {                                  // the target rows are sorted: find the key's item among them
            const int32_t item = (int32_t)~(uint32_t)key;
            int lo = 0, hi = p.nt - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tg[mid] < item) lo = mid + 1; else hi = mid;
            }
            go[t] = lo;
        }
    }
    if (lane == 0) a.nr[pc] = nr;

    if (nr > 0) {                                      // take the excluded items off, binned as k_rank_count bins them
        const uint64_t lowest = kq[nr - 1];
        for (int64_t e0 = p.xlo; e0 < p.xhi; e0 += RANK_SUB) {
            const int64_t ei = e0 + c < p.xhi ? e0 + c : p.xhi - 1;
            const f32x16 acc = mfma_tile_dot<V4>(a.Q + (int64_t)a.excl[ei] * a.D, prow, a.D, a.item_abs, h);
            if (c == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sq[(r & 3) + 8 * (r >> 2) + 4 * h] = acc[r];
            }
            wave_lds_sync();
            const int64_t e = e0 + lane;
            if (lane < RANK_SUB && e < p.xhi) {
                const int32_t item = a.excl[e];
                if (e == p.xlo || a.excl[e - 1] != item) {   // a repeated id is one item, taken off once
                    const float s = ((sq[lane] + mu) + ub) + a.bi[item];
                    if (!__builtin_isnan(s)) {
                        const uint64_t key = topk_key(s, item);
                        if (key > lowest) atomicSub(&bq[rank_bin(kq, nr, key)], 1);
                    }
                }
            }
            wave_lds_sync();
        }
    }
    int32_t* gb = a.bins + pc * RANK_CAP;
    for (int t = lane; t < RANK_CAP; t += 64) gb[t] = bq[t];
}

template <bool V4>
__global__ __launch_bounds__(256) void k_rank_count(RankArgs a) {
    __shared__ uint64_t keys[RANK_PPB * RANK_CAP];
    __shared__ int32_t bins[RANK_PPB * RANK_CAP];
    static_assert(sizeof(keys) + sizeof(bins) == rank_count_static_lds(),
                  "tfr_rank_plan reports a different LDS size than k_rank_count declares");
    static_assert(RANK_PPB == 32, "a block's pieces are the 32 columns of the MFMA");
    warm_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int64_t p0 = (int64_t)blockIdx.x * RANK_PPB;
    const int64_t pc = p0 + c;                         // the piece of this lane's accumulator column
    int nr = 0;
    int32_t user = 0;                                  // a column past the chunk scores user 0 and bins nothing
    if (pc < a.n_pieces) { nr = a.nr[pc]; user = a.pieces[pc].user; }
    for (int t = threadIdx.x; t < RANK_PPB * RANK_CAP; t += 256) {
        keys[t] = p0 + t / RANK_CAP < a.n_pieces ? a.keys[p0 * RANK_CAP + t] : 0;
        bins[t] = 0;
    }
    __syncthreads();
    const uint64_t* kq = keys + c * RANK_CAP;
    const uint64_t lowest = nr > 0 ? kq[nr - 1] : ~0ull;
    const float* prow = a.P + (int64_t)user * a.D;
    const float mu = *a.mu;
    const float ub = a.bu[user];

    const int64_t per = ((a.n_items + a.slices - 1) / a.slices + RANK_ROUND - 1) / RANK_ROUND * RANK_ROUND;
    const int64_t s_lo = (int64_t)blockIdx.y * per;
    const int64_t s_hi = s_lo + per < a.n_items ? s_lo + per : a.n_items;
    const int64_t rounds = s_hi > s_lo ? (s_hi - s_lo + RANK_ROUND - 1) / RANK_ROUND : 0;
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t base = s_lo + rd * RANK_ROUND + wave * RANK_SUB;
        int64_t my_item = base + c;                    // A row = item; past the slice: a row inside it, result dropped
        if (my_item >= s_hi) my_item = s_hi - 1;
        const f32x16 acc = mfma_tile_dot<V4>(a.Q + my_item * a.D, prow, a.D, a.item_abs, h);
        if (nr > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t item = base + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (item < s_hi) {
                    const float s = ((acc[r] + mu) + ub) + a.bi[item];
                    if (!__builtin_isnan(s)) {
                        const uint64_t key = topk_key(s, item);
                        if (key > lowest) atomicAdd(&bins[c * RANK_CAP + rank_bin(kq, nr, key)], 1);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < RANK_PPB * RANK_CAP; t += 256) {
        const int32_t v = bins[t];
        if (v && p0 + t / RANK_CAP < a.n_pieces) atomicAdd(&a.bins[p0 * RANK_CAP + t], v);   // integer sums: the result does not depend on the order
    }
}

__global__ __launch_bounds__(256) void k_rank_finish(RankArgs a) {
    static_assert(RANK_CAP == 128, "a lane scans two bins");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pc = (int64_t)blockIdx.x * RANK_WAVES + wave;
    if (pc >= a.n_pieces) return;
    const int nr = a.nr[pc];
    const int32_t* b = a.bins + pc * RANK_CAP;
    const int j0 = 2 * lane, j1 = 2 * lane + 1;
    const int32_t v0 = j0 < nr ? b[j0] : 0, v1 = j1 < nr ? b[j1] : 0;
    int32_t s = v0 + v1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t o = __shfl_up(s, off);
        if (lane >= off) s += o;
    }
    const int32_t r0 = s - v1, r1 = s;                 // inclusive sums through bins j0 and j1
    const int32_t* go = a.order + pc * RANK_CAP;
    int32_t* out = a.ranks + a.pieces[pc].tlo;
    if (j0 < nr) out[go[j0]] = r0;
    if (j1 < nr) out[go[j1]] = r1;
}

template <bool V4>
static void launch_rank_v(const RankArgs& a, const RankPlan& p, hipStream_t s) {
    const unsigned per_wave = (unsigned)((a.n_pieces + RANK_WAVES - 1) / RANK_WAVES);
    hipLaunchKernelGGL((k_rank_targets<V4>), dim3(per_wave), dim3(256), 0, s, a);
    const dim3 g((unsigned)((a.n_pieces + p.ppb - 1) / p.ppb), (unsigned)p.slices);
    hipLaunchKernelGGL((k_rank_count<V4>), g, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_rank_finish, dim3(per_wave), dim3(256), 0, s, a);
}

void launch_rank(const RankArgs& a, const RankPlan& p, hipStream_t s) {
    if (a.n_pieces < 1) return;
    if ((a.D & 3) == 0) launch_rank_v<true>(a, p, s);
    else launch_rank_v<false>(a, p, s);
}

}  // namespace tfr
