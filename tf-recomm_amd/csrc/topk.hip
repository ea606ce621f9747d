// topk.hip - top-K recommendation on gfx950 (forward.py:47-61 get_ranking, als3.py:110-113 predict-then-rank).
//
// k_topk_score: a block owns a tile of users (the 32 columns of a 32x32x2 f32 MFMA) and a slice of the items.  Every round
//   each of its 4 waves scores a 32-item sub-tile against the tile's users with v_mfma_f32_32x32x2_f32, k ascending from a
//   zero accumulator (bit for bit the fmaf chain of the contract), adds mu, bu and bi in that order, and appends the keys
//   that beat its user's running k-th key (and are not excluded) to that user's LDS queue.  Between rounds a queue that
//   could not take another round is sorted (bitonic, one wave), cut to k and its threshold raised.  At the end every queue
//   is sorted and its first k keys go to part[row, slice].
// k_topk_merge: one wave per row merges the slices' sorted lists (tournament over the list heads in LDS) into the output.
// k_topk_check_excl: the device entry's range / order check of the exclusion CSR.
#include <hip/hip_runtime.h>
#include "svd_kernels.h"
#include "score_tile.h"
#include "topk.h"

namespace tfr {

template <int UPB, int CAP, bool V4>
__global__ __launch_bounds__(256) void k_topk_score(TopkArgs a) {
    __shared__ uint64_t queue[UPB * CAP];
    __shared__ uint64_t thr[UPB];
    __shared__ int32_t cnt[UPB];
    static_assert(sizeof(queue) + sizeof(thr) + sizeof(cnt) == topk_score_static_lds(UPB, CAP),
                  "tfr_topk_plan reports a different LDS size than the kernel declares");
    static_assert(CAP - TOPK_ROUND >= (CAP == 256 ? 128 : TOPK_KMAX), "a queue must hold k plus one round of appends");
    warm_args(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, c = lane & 31;
    const int j = c & (UPB - 1);                       // user of this lane's accumulator column
    const bool own_col = c < UPB;                      // UPB 16: columns 16..31 repeat 0..15 and select nothing
    const int64_t row = (int64_t)blockIdx.x * UPB + j;
    const int slice = blockIdx.y;
    const int k = a.k;

    int32_t user = -1;
    if (row < a.n_rows) {
        user = a.users[row];
        if (user < 0 || (int64_t)user >= a.U) {
            if (own_col && h == 0) atomicOr(a.err, 1);
            user = -1;
        }
    }
    const bool live = own_col && user >= 0;
    int64_t xlo = 0, xhi = 0;
    if (live && a.indptr && *a.excl_bad == 0) { xlo = a.indptr[row]; xhi = a.indptr[row + 1]; }
    const float* prow = a.P + (int64_t)(user < 0 ? 0 : user) * a.D;
    const float mu = *a.mu;
    const float ub = user >= 0 ? a.bu[user] : 0.f;
    for (int t = threadIdx.x; t < UPB; t += 256) { cnt[t] = 0; thr[t] = 0; }
    __syncthreads();

    const int64_t per = ((a.n_items + a.slices - 1) / a.slices + TOPK_ROUND - 1) / TOPK_ROUND * TOPK_ROUND;
    const int64_t s_lo = (int64_t)slice * per;
    const int64_t s_hi = s_lo + per < a.n_items ? s_lo + per : a.n_items;
    const int64_t rounds = s_hi > s_lo ? (s_hi - s_lo + TOPK_ROUND - 1) / TOPK_ROUND : 0;

    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t base = s_lo + rd * TOPK_ROUND + wave * TOPK_SUB;
        int64_t my_item = base + c;                    // A row = item; past the slice: a row inside it, result dropped
        if (my_item >= s_hi) my_item = s_hi - 1;
        const float* qrow = a.Q + my_item * a.D;
        const f32x16 acc = mfma_tile_dot<V4>(qrow, prow, a.D, a.item_abs, h);
        // C[item row][user column]: this lane holds user j, items base + (r&3) + 8(r>>2) + 4h
        const uint64_t th = thr[j];
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t item = base + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (item < s_hi) {
                    const float s = ((acc[r] + mu) + ub) + a.bi[item];
                    if (!__builtin_isnan(s)) {
                        const uint64_t key = topk_key(s, item);
                        if (key > th && !(xhi > xlo && topk_excluded(a.excl, xlo, xhi, (int32_t)item))) {
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

__global__ __launch_bounds__(64) void k_topk_merge(TopkMergeArgs a) {
    extern __shared__ uint64_t keys[];
    warm_args(a);
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int k = a.k, S = a.slices;
    const uint64_t* src = a.part + (size_t)row * S * k;
    for (int t = lane; t < S * k; t += 64) keys[t] = src[t];
    __syncthreads();
    // lane holds the heads of lists lane, lane + 64, lane + 128, lane + 192
    int hd[4];
    uint64_t cur[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        const int s = lane + 64 * z;
        hd[z] = 0;
        cur[z] = s < S ? keys[s * k] : 0;
    }
    int32_t* io = a.items_out + (size_t)row * k;
    float* so = a.scores_out ? a.scores_out + (size_t)row * k : nullptr;
    int q = 0;
    for (; q < k; ++q) {
        uint64_t best = cur[0];
        int bz = 0;
#pragma unroll
        for (int z = 1; z < 4; ++z) if (cur[z] > best) { best = cur[z]; bz = z; }
        uint64_t m = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(m, off);
            m = o > m ? o : m;
        }
        if (m == 0) break;                             // every list is exhausted
        if (best == m) {                               // keys are distinct: exactly one lane
            io[q] = (int32_t)~(uint32_t)m;
            if (so) so[q] = topk_key_score(m);
#pragma unroll
            for (int z = 0; z < 4; ++z)
                if (z == bz) {
                    ++hd[z];
                    cur[z] = hd[z] < k ? keys[(lane + 64 * z) * k + hd[z]] : 0;
                }
        }
    }
    for (int t = q + lane; t < k; t += 64) {
        io[t] = -1;
        if (so) so[t] = -INFINITY;
    }
}

__global__ __launch_bounds__(256) void k_topk_check_excl(const int64_t* indptr, const int32_t* x, int64_t n_rows,
                                                         int64_t n_items, int32_t* bad, int32_t* err) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_rows; row += (int64_t)gridDim.x * 4) {
        const int64_t lo = indptr[row], hi = indptr[row + 1];
        int32_t f = 0;
        if (lo < 0 || hi < lo) {
            f = 16;                                    // the items of a malformed row are not read
        } else {
            for (int64_t t = lo + lane; t < hi; t += 64) {
                const int32_t v = x[t];
                if (v < 0 || (int64_t)v >= n_items) f |= 1;
                if (t > lo && x[t - 1] > v) f |= 16;
            }
        }
        if (f) { atomicOr(bad, 1); atomicOr(err, f); }
    }
}

template <int UPB, int CAP>
static void launch_score_v(const TopkArgs& a, dim3 g, hipStream_t s) {
    if ((a.D & 3) == 0) hipLaunchKernelGGL((k_topk_score<UPB, CAP, true>), g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_topk_score<UPB, CAP, false>), g, dim3(256), 0, s, a);
}

void launch_topk_score(const TopkArgs& a, const TopkPlan& p, hipStream_t s) {
    const dim3 g((unsigned)((a.n_rows + p.upb - 1) / p.upb), (unsigned)p.slices);
    if (p.cap == 256) launch_score_v<32, 256>(a, g, s);
    else launch_score_v<16, 512>(a, g, s);
}

void launch_topk_merge(const TopkMergeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)a.n_rows), dim3(64), topk_merge_lds(a.slices, a.k), s, a);
}

void launch_topk_check_excl(const int64_t* indptr, const int32_t* excl, int64_t n_rows, int64_t n_items, int32_t* bad,
                            int32_t* err, hipStream_t s) {
    int64_t nb = (n_rows + 3) / 4;
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_topk_check_excl, dim3((unsigned)nb), dim3(256), 0, s, indptr, excl, n_rows, n_items, bad, err);
}

}  // namespace tfr
