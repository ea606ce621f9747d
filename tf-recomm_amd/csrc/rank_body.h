// rank_body.h - the bodies of k_rank_targets and k_rank_count, generic over a scorer, as sliced_topk_block is (score_tile.h):
// rank.hip runs them on the float32 tables (RankScorer), bf16_rank.hip on the bf16 snapshot (Bf16RankScorer).  DESIGN §13, §26.
//
// Scorer(a, user) is built once per lane for the user of the lane's accumulator column: tile(row, h) is the MFMA tile of item
// row `row` (the A row of this lane) against that user's row, score(dot, item) adds the biases.  Everything else - pieces,
// keys, the sort, the bins, every clamp to a valid row - is here, once, so both row formats rank by the same rules.  The clamps
// are what makes the bf16 tile's unguarded 16-byte loads safe: a lane past the piece, the exclusions or the slice
// loads a row inside it, and a column past the chunk loads user 0.
#pragma once
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

// one wave per piece (k_rank_targets of rank.hip's header comment)
template <class Scorer, class Args>
__device__ __forceinline__ void rank_targets_block(const Args& a) {
    __shared__ uint64_t keys[RANK_WAVES * RANK_CAP];
    __shared__ int32_t bins[RANK_WAVES * RANK_CAP];
    __shared__ float sc[RANK_WAVES * RANK_SUB];
    static_assert(sizeof(keys) + sizeof(bins) + sizeof(sc) == rank_targets_static_lds(),
                  "tfr_rank_plan reports a different LDS size than k_rank_targets declares");
    static_assert(RANK_CAP % 64 == 0 && RANK_SUB == 32, "a wave sorts RANK_CAP keys and scores 32 items a tile");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int64_t pc = (int64_t)blockIdx.x * RANK_WAVES + wave;
    if (pc >= a.n_pieces) return;                      // the whole wave: no block barrier below
    const RankPiece p = a.pieces[pc];
    uint64_t* kq = keys + wave * RANK_CAP;
    int32_t* bq = bins + wave * RANK_CAP;
    float* sq = sc + wave * RANK_SUB;
    const int32_t* tg = a.tgt + p.tlo;
    const Scorer scr(a, p.user);
    for (int t = lane; t < RANK_CAP; t += 64) { kq[t] = 0; bq[t] = 0; }
    for (int t = lane; t < p.nt; t += 64) a.ranks[p.tlo + t] = -1;
    wave_lds_sync();

    for (int t0 = 0; t0 < p.nt; t0 += RANK_SUB) {
        const int ti = t0 + c < p.nt ? t0 + c : p.nt - 1;    // A row = target; past the piece: one inside it, dropped
        const f32x16 acc = scr.tile((int64_t)tg[ti], h);
        if (c == 0) {                                  // every column is the piece's user: column 0 has all 32 rows
#pragma unroll
            for (int r = 0; r < 16; ++r) sq[(r & 3) + 8 * (r >> 2) + 4 * h] = acc[r];
        }
        wave_lds_sync();
        if (lane < RANK_SUB && t0 + lane < p.nt) {
            const int32_t item = tg[t0 + lane];
            const float s = scr.score(sq[lane], item);
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
            const f32x16 acc = scr.tile((int64_t)a.excl[ei], h);
            if (c == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sq[(r & 3) + 8 * (r >> 2) + 4 * h] = acc[r];
            }
            wave_lds_sync();
            const int64_t e = e0 + lane;
            if (lane < RANK_SUB && e < p.xhi) {
                const int32_t item = a.excl[e];
                if (e == p.xlo || a.excl[e - 1] != item) {   // a repeated id is one item, taken off once
                    const float s = scr.score(sq[lane], item);
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

// a block owns 32 pieces and one item slice (k_rank_count of rank.hip's header comment)
template <class Scorer, class Args>
__device__ __forceinline__ void rank_count_block(const Args& a) {
    __shared__ uint64_t keys[RANK_PPB * RANK_CAP];
    __shared__ int32_t bins[RANK_PPB * RANK_CAP];
    static_assert(sizeof(keys) + sizeof(bins) == rank_count_static_lds(),
                  "tfr_rank_plan reports a different LDS size than k_rank_count declares");
    static_assert(RANK_PPB == 32, "a block's pieces are the 32 columns of the MFMA");
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
    const Scorer scr(a, user);

    const int64_t per = ((a.n_items + a.slices - 1) / a.slices + RANK_ROUND - 1) / RANK_ROUND * RANK_ROUND;
    const int64_t s_lo = (int64_t)blockIdx.y * per;
    const int64_t s_hi = s_lo + per < a.n_items ? s_lo + per : a.n_items;
    const int64_t rounds = s_hi > s_lo ? (s_hi - s_lo + RANK_ROUND - 1) / RANK_ROUND : 0;
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t base = s_lo + rd * RANK_ROUND + wave * RANK_SUB;
        int64_t my_item = base + c;                    // A row = item; past the slice: a row inside it, result dropped
        if (my_item >= s_hi) my_item = s_hi - 1;
        const f32x16 acc = scr.tile(my_item, h);
        if (nr > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t item = base + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (item < s_hi) {
                    const float s = scr.score(acc[r], item);
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

}  // namespace tfr
