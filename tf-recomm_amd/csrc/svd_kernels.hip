// svd_kernels.hip - gfx950 kernels of the SVD minibatch step (wave64, no MFMA: this is a
// batched gather-dot and a segmented scatter, HBM-bound).
//
// Row geometry: one table row of D floats is spread over a lane group of G lanes, VEC
// floats per lane (G*VEC >= D), so a wave64 holds 64/G rows at once and a full group
// reads its row as one contiguous, 16-byte-per-lane burst (D=128: 32 lanes x float4 =
// 512 B).  D % 4 == 0 -> VEC=4 (global_load_dwordx4); otherwise VEC=1 (rows are then not
// 16-byte aligned; correctness path for the reference's dim=5/15).
//
// Reference semantics restated per kernel; file:line into the reference tree.  The row fragment, the group / wave /
// block sums and K1 itself, the gather-dot forward, are in forward_body.h, which the bf16 snapshot's forward
// (bf16_rows.hip) shares; k_forward and k_front instantiate it on float32 rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "svd_kernels.h"
#include "forward_body.h"
#include "finalize.inc.h"

namespace tfr {

// ------------------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void store_frag(float* __restrict__ row, int d0, int D, const Frag<VEC>& f) {
    if (d0 < D) {
        if constexpr (VEC == 4) {
            *reinterpret_cast<float4*>(row + d0) = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
        } else {
            row[d0] = f.v[0];
        }
    }
}

// a lane's VEC floats of a row known to be G * VEC wide: no `d0 < D` guard, so the loaded registers are not merged with a
// zero-initialised copy afterwards (that merge is a register move behind a full wait for the load)
template <int VEC, bool NT>
__device__ __forceinline__ Frag<VEC> load_full(const float* __restrict__ p) {
    Frag<VEC> f;
    if constexpr (VEC == 4) {
        floatx4 t;
        if constexpr (NT) t = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(p));
        else t = *reinterpret_cast<const floatx4*>(p);
        f.v[0] = t.x; f.v[1] = t.y; f.v[2] = t.z; f.v[3] = t.w;
    } else {
        if constexpr (NT) f.v[0] = __builtin_nontemporal_load(p);
        else f.v[0] = *p;
    }
    return f;
}

// cache-policy experiments on the big-table step (RedArgs::nt bits; A/B by TFR_NT): runtime-selected hints
template <int VEC>
__device__ __forceinline__ Frag<VEC> load_frag_h(const float* __restrict__ row, int d0, int D, bool nt) {
    return nt ? load_frag<VEC, true>(row, d0, D) : load_frag<VEC, false>(row, d0, D);
}
template <int VEC>
__device__ __forceinline__ void store_frag_h(float* __restrict__ row, int d0, int D, const Frag<VEC>& f, bool nt) {
    if (!nt) { store_frag<VEC>(row, d0, D, f); return; }
    if (d0 < D) {
        if constexpr (VEC == 4) {
            floatx4 t; t.x = f.v[0]; t.y = f.v[1]; t.z = f.v[2]; t.w = f.v[3];
            __builtin_nontemporal_store(t, reinterpret_cast<floatx4*>(row + d0));
        } else {
            __builtin_nontemporal_store(f.v[0], row + d0);
        }
    }
}

// write-through (sc1) vector stores for bytes whose only reader is the next dependent launch: the line is written
// on to memory and dropped from the XCD's L2 instead of being left dirty there, so the kernel boundary has less
// to write back (TFR_WT bits, A/B).  Through a buffer resource on a block-uniform base; `off` counts floats from
// it and stays below 2^29 (small tables: at most 16384 rows / 16 tiles of 1024 entries, D <= 256).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);   // 32-bit data format
}
template <int VEC>
__device__ __forceinline__ void store_frag_wt(__amdgpu_buffer_rsrc_t r, size_t off, int d0, int D, const Frag<VEC>& f) {
    if (d0 < D) {
        if constexpr (VEC == 4) {
            typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
            uintx4 t;
            t.x = __float_as_uint(f.v[0]); t.y = __float_as_uint(f.v[1]); t.z = __float_as_uint(f.v[2]); t.w = __float_as_uint(f.v[3]);
            __builtin_amdgcn_raw_buffer_store_b128(t, r, (int)((off + d0) * 4), 0, 16);      // aux 16: sc1
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(f.v[0]), r, (int)((off + d0) * 4), 0, 16);
        }
    }
}
template <int VEC>
__device__ __forceinline__ void store_frag_p(float* base, size_t off, int d0, int D, const Frag<VEC>& f, bool wt) {
    if (wt) store_frag_wt<VEC>(wt_rsrc(base), off, d0, D, f);
    else store_frag<VEC>(base + off, d0, D, f);
}
__device__ __forceinline__ void store_word_p(void* base, size_t idx, uint32_t x, bool wt) {
    if (wt) __builtin_amdgcn_raw_buffer_store_b32(x, wt_rsrc(base), (int)(idx * 4), 0, 16);
    else reinterpret_cast<uint32_t*>(base)[idx] = x;
}

// loads through the same kind of resource (k_dense_tiles' full-width form): one VGPR of byte offset per address, and a load
// predicated without a branch - an offset past the resource's 2^31 - 1 bytes is answered with zeros and goes to no
// cache (unlike a dummy address, which would be one hot L2 line), so a row of loads is one basic block
constexpr int BUF_NONE = (int)0x80000000u;
__device__ __forceinline__ uint32_t buf_load_word(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0);
}
template <int VEC>
__device__ __forceinline__ Frag<VEC> buf_load_frag(__amdgpu_buffer_rsrc_t r, int byte_off) {
    Frag<VEC> f;
    if constexpr (VEC == 4) {
        typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
        const uintx4 t = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
        f.v[0] = __uint_as_float(t.x); f.v[1] = __uint_as_float(t.y); f.v[2] = __uint_as_float(t.z); f.v[3] = __uint_as_float(t.w);
    } else {
        f.v[0] = __uint_as_float(buf_load_word(r, byte_off));
    }
    return f;
}

// x of lane L (a constant) of the caller's lane group - of its own 16-lane row where a group spans several - in every lane:
// one DPP move where a group is one row or more (row_newbcast) or a quad (quad_perm), a bpermute otherwise.  No lane is
// read that the caller's group does not own, so groups that have left the kernel as a whole are never looked at.
template <int G, int L>
__device__ __forceinline__ uint32_t group_bcast(uint32_t x) {
    static_assert(L < G && L < 16, "group_bcast: L is a lane of the group's 16-lane row");
    if constexpr (G >= 16) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x150 + L, 0xf, 0xf, false);
    else if constexpr (G == 4) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, L * 0x55, 0xf, 0xf, false);
    else return (uint32_t)__shfl((int)x, L, G);
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in that order
template <int... K, typename F>
__device__ __forceinline__ void unrolled(std::integer_sequence<int, K...>, F&& f) { (f(std::integral_constant<int, K>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void unrolled(F&& f) { unrolled(std::make_integer_sequence<int, N>{}, f); }

// per-piece {loss, reg, sum g} for k_tile_step without a cross-lane reduction in every wave: lane
// group leaders park the entry's loss and g, every lane its share of the regulariser, in LDS;
// after the barrier wave (h, c) alone adds piece h's values of kind c in a fixed order.
// stage: EPG * (2 * EPB + 1024) floats.  16 waves; has one barrier.
template <int G, int EPG>
__device__ __forceinline__ void block_sum_pieces(const float (&val)[3 * EPG], float* stage, float* out) {
    constexpr int EPB = 1024 / G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = tid / G, gl = tid % G;
    float* sl = stage;                                   // [EPG][EPB]   loss per entry
    float* sg = stage + EPG * EPB;                       // [EPG][EPB]   g per entry
    float* sr = stage + 2 * EPG * EPB;                   // [EPG][1024]  regulariser share per lane
#pragma unroll
    for (int h = 0; h < EPG; ++h) {
        if (gl == 0) { sl[h * EPB + grp] = val[3 * h + 0]; sg[h * EPB + grp] = val[3 * h + 2]; }
        sr[h * 1024 + tid] = val[3 * h + 1];
    }
    __syncthreads();
    if (wave < 3 * EPG) {
        const int h = wave / 3, c = wave % 3;
        float x = 0.f;
        if (c == 1) {
#pragma unroll
            for (int k = 0; k < 16; ++k) x += sr[h * 1024 + k * 64 + lane];
        } else {
            const float* src = (c == 0 ? sl : sg) + h * EPB;
            for (int k = lane; k < EPB; k += 64) x += src[k];
        }
        x = wave_sum(x);
        if (lane == 0) out[h * 4 + c] = x;
    }
}

// ------------------------------------------------------------------------------------
// K1 on float32 rows (forward_body.h).
// PNT: user rows by non-temporal loads - set when the user table cannot stay in the 256 MB Infinity Cache
// anyway (stream_user_rows), so that it does not evict the item rows and the bias arrays, which can
// (tools/probes/fwd_policy.hip: 48.3 -> 46.0 us per 262144 ratings at 10M x 1M rows)
template <int G, int VEC, int MODE, int UNR, bool PNT>
__global__ __launch_bounds__(256) void k_forward(FwdArgs a) {
    warm_args(a);
    forward_body<Float32Rows<VEC>, G, MODE, UNR, 4, PNT>(a, blockIdx.x, gridDim.x);
}
// In-LDS exclusive scan of a tile's nb bin counts into the packed form (count << 16) | start.
// Thread t owns bins t, t + 1024, ... (bank-conflict free) and those bins are CONSECUTIVE in the
// tile's sorted order (order index of bin q * 1024 + t is t * per + q): equal ids stay contiguous,
// which is all the reduce and the sweep need - the order of distinct ids inside a tile is free.
// wtot: 16 ints of scratch.  All 1024 threads call; ends with a barrier.  nb <= 16384.
__device__ __forceinline__ void tile_scan_pack(int32_t* cnt, int nb, int32_t* wtot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (nb + 1023) / 1024;                  // <= 16
    int32_t sum = 0;
    for (int q = 0; q < per; ++q) { const int b = q * 1024 + tid; if (b < nb) sum += cnt[b]; }
    int32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t t2 = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t2;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int32_t run = incl - sum;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    for (int q = 0; q < per; ++q) {
        const int b = q * 1024 + tid;
        if (b < nb) { const int32_t c2 = cnt[b]; cnt[b] = (c2 << 16) | run; run += c2; }
    }
    __syncthreads();
}

// Small-table training: the forward and the counting sort's rank pass do not depend on each other,
// so they share one launch - blocks [0, nfwd) run the forward (16 waves each), the rest rank one
// (tile, column) each.  In fused-gather mode the rank blocks read the store records themselves and
// publish the gathered ids for the later passes.
template <int G, int VEC>
__global__ __launch_bounds__(1024) void k_front(FrontArgs fa) {
    warm_args(fa);
    if ((int)blockIdx.x < fa.nfwd) {
        forward_body<Float32Rows<VEC>, G, MODE_TRAIN, 2, 16>(fa.f, blockIdx.x, fa.nfwd);
        return;
    }
    extern __shared__ int32_t cnt[];
    const CSortArgs& a = fa.c;
    const int rb = blockIdx.x - fa.nfwd;
    const int col = rb / a.ntiles, tile = rb % a.ntiles, tid = threadIdx.x;
    const int nb = a.nbins[col];
    for (int b = tid; b < nb; b += CSORT_TILE) cnt[b] = 0;
    __syncthreads();
    const int64_t k = (int64_t)tile * CSORT_TILE + tid;
    const bool valid = k < a.B;
    int32_t key = 0, fullkey = 0;
    if (valid) {
        if (fa.f.ids) {
            int64_t id = fa.f.ids[k];
            if ((uint64_t)id >= (uint64_t)fa.f.N) id = 0;          // flagged by the forward blocks
            const int4 rec = fa.f.store[id];
            fullkey = col == 0 ? rec.x : rec.y;
            fa.key_out[col][k] = fullkey;
        } else {
            fullkey = a.keys[col][k];
        }
        key = fullkey & (nb - 1);
    }
    unsigned long long mask = __ballot(valid);
    for (int bit = 1; bit < nb; bit <<= 1) {
        const unsigned long long m = __ballot((key & bit) != 0);
        mask &= (key & bit) ? m : ~m;
    }
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int rank_in_wave = __popcll(below);
    const int group_size = __popcll(mask);
    int base = 0;
    for (int w = 0; w < CSORT_TILE / 64; ++w) {
        if (wave == w && valid) {
            base = cnt[key];
            if (below == 0) cnt[key] = base + group_size;
        }
        __syncthreads();
    }
    if (!fa.tile_local) {
        if (valid) a.lrank[col][k] = base + rank_in_wave;
        for (int b = tid; b < nb; b += CSORT_TILE) a.hist[col][(size_t)tile * nb + b] = cnt[b];
        return;
    }
    // tile-local sort: the tile's entries are put in key order right here (no global scan / scatter
    // launches).  hist[tile][bin] = (entries of the tile with that key) << 16 | (where they start inside
    // the tile's sorted list); the sweep finds a row's per-tile runs through this table.
    __shared__ int32_t wtot[256];
    tile_scan_pack(cnt, nb, wtot);
    for (int b = tid; b < nb; b += CSORT_TILE) a.hist[col][(size_t)tile * nb + b] = cnt[b];     // packed lookup table
    if (valid) {
        const int64_t dst = (int64_t)tile * CSORT_TILE + (cnt[key] & 0xffff) + base + rank_in_wave;
        a.ks[col][dst] = fullkey;
        a.ps[col][dst] = (int32_t)k;
    }
}

// ------------------------------------------------------------------------------------
// K1+K2+K3 for small tables in one launch (k_tile_step).
//
// tile_sort: one 1024-thread block gathers a 1024-entry tile of a batch (dataio.py:115-117 when the
// ids index the resident store), range-checks the ids and sorts the tile by one id column with a
// stable counting sort held entirely in LDS (ballot ranks, ordered wave turns, in-LDS scan).  On
// return cnt[] holds the packed lookup table, srt_key / srt_pos the sorted order, rec_* the tile's
// records by batch position.  Ends with a barrier.
struct TileLds {
    int32_t* cnt; int32_t* rec_u; int32_t* rec_i; float* rec_r; int32_t* srt_key; int32_t* srt_pos; int32_t* wtot;
};
__device__ __forceinline__ void tile_sort(int32_t* cnt_, int32_t* rec_u_, int32_t* rec_i_, float* rec_r_, int32_t* srt_key_,
                                          int32_t* srt_pos_, int32_t* wtot_, const int64_t* ids, const int4* store, const int4* recs,
                                          const int32_t* bu_, const int32_t* bi_, const float* br_, int64_t tile0, int nvalid, int side,
                                          int nb, int64_t N, int64_t U, int64_t I, int32_t* err, bool have_rec, int4 rec_in) {
    TileLds L;
    L.cnt = cnt_; L.rec_u = rec_u_; L.rec_i = rec_i_; L.rec_r = rec_r_; L.srt_key = srt_key_; L.srt_pos = srt_pos_; L.wtot = wtot_;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = tid; b < nb; b += 1024) L.cnt[b] = 0;
    const bool valid = tid < nvalid;
    int32_t u = 0, it = 0;
    float r = 0.f;
    if (valid) {
        const int64_t k = tile0 + tid;
        bool oob = false;
        if (have_rec) {                                  // recs[k], requested by the caller already (k_tile_step's look-ahead blocks)
            u = rec_in.x; it = rec_in.y; r = __int_as_float(rec_in.z);
        } else if (recs) {                               // the batch's store records, left beside the ids by the stream that drew
            const int4 rec = recs[k];                    // them (api.hip RecBuf): one round trip instead of ids -> store
            u = rec.x; it = rec.y; r = __int_as_float(rec.z);
        } else if (ids) {
            int64_t id = ids[k];
            if ((uint64_t)id >= (uint64_t)N) { atomicOr(err, 2); id = 0; }
            const int4 rec = store[id];
            u = rec.x; it = rec.y; r = __int_as_float(rec.z);
        } else {
            u = bu_[k]; it = bi_[k]; r = br_[k];
        }
        if ((uint64_t)(int64_t)u >= (uint64_t)U) { oob = true; u = 0; }
        if ((uint64_t)(int64_t)it >= (uint64_t)I) { oob = true; it = 0; }
        if (oob) atomicOr(err, 1);
    }
    L.rec_u[tid] = u; L.rec_i[tid] = it; L.rec_r[tid] = r;
    __syncthreads();
    const int32_t key = side == 0 ? u : it;
    unsigned long long mask = __ballot(valid);
    for (int bit = 1; bit < nb; bit <<= 1) {
        const unsigned long long mm = __ballot((key & bit) != 0);
        mask &= (key & bit) ? mm : ~mm;
    }
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int rank_in_wave = __popcll(below);
    const int group_size = __popcll(mask);
    int base = 0;
    for (int w = 0; w < 16; ++w) {
        if (wave == w && valid) {
            base = L.cnt[key];
            if (below == 0) L.cnt[key] = base + group_size;
        }
        __syncthreads();
    }
    tile_scan_pack(L.cnt, nb, L.wtot);
    if (valid) {
        const int dst = (L.cnt[key] & 0xffff) + base + rank_in_wave;
        L.srt_key[dst] = key;
        L.srt_pos[dst] = tid;
    }
    __syncthreads();
}

// partials[from, to) = 0 by the whole block (k_tile_step: the item side's last block; from = INT32_MAX elsewhere)
__device__ __forceinline__ void zero_tail(float* partials, int from, int to) {
    if (from < to) for (int k = from + (int)threadIdx.x; k < to; k += 1024) partials[k] = 0.f;
}

struct TileStamp {                                       // diagnostic (TFR_TILE_DEBUG): when did this block start, pass its phases, end?
    unsigned long long* p; unsigned long long t0;        // p: none until arm() - a.dbg is a word of the struct, in hand only behind warm_args_land
    __device__ __forceinline__ void arm(unsigned long long* dbg) { p = dbg ? dbg + 8 * (size_t)blockIdx.x : nullptr; }
    __device__ __forceinline__ void mark(int k) const { if (p && threadIdx.x == 0) p[k] = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ ~TileStamp() { if (p && threadIdx.x == 0) { p[0] = t0; p[1] = __builtin_amdgcn_s_memrealtime(); } }
};

template <int G, int VEC, int EPG, bool PRE>
__device__ __forceinline__ void tile_pieces(const TileStepArgs& a, int32_t* dyn, const int32_t* rec_u, const int32_t* rec_i,
                                            const float* rec_r, const int32_t* srt_key, const int32_t* srt_pos, float* lds_gb,
                                            int32_t* lds_key, float* lds_stage, TileStamp& stamp, int side, int bx, int slice,
                                            int64_t tile0, int nvalid, const int4* srt, const WarmLines<TileStepArgs>& warm,
                                            int zero_from, int zero_to);

// grid = nsort + nblk_u + nblk_i, one dimension: the look-ahead sort blocks, then the user side's blocks, then the
// item side's, each side cut to the blocks that hold entries (ceil(B / entries per block)).
//  * blocks [0, nsort): look-ahead - tile_sort one (side, tile) of the NEXT batch and publish its
//    packed table and its sorted records; that work has no dependence on the tables, so it rides
//    here, in the shadow of this step's reduce, instead of heading the next step's critical path.
//  * the other blocks: block (tile, slice, side) owns EPG pieces of 1024/G consecutive entries of the
//    tile's sorted list - read from the records the previous launch published, or, without look-ahead,
//    after repeating the tile's sort itself (every block of a tile does: cheap next to a launch and
//    two more dependent memory round trips).  One lane group per entry loads P[u], Q[i] once, forms
//    the logit and g = dcost/dlogit exactly as K1 does (both sides compute the same g from the same
//    registers), and the runs inside each piece are summed in two levels - inside a wave in registers,
//    across the piece's 16 waves through LDS - always by doubling, i.e. in a fixed tree order (K3).  Piece sums land at the tile-sorted position.  The item side also writes the
//    logits and the per-piece {loss, reg, sum g}.  The user side takes EPG pieces per block, the item
//    side a.epg_item = EPG, or EPG / 2 where the grid has room for it (TFR_ITEM_SPLIT=1, tile_step_item_epg);
//    the grid stays within one block per CU.
//
// The leading scalar parameters are what a block needs to issue its first vector loads - the published records of a step
// block on the presorted path (srt_u / srt_i = a.srt[], B = a.B, epg_item, ntiles), the next batch's store records of a
// look-ahead block (next_recs, next_ntiles, next_B = a.next_*), and whether TFR_TILE_DEBUG wants the block's start stamped
// (stamps = a.dbg != NULL): 14 dwords, all the command processor preloads into user SGPRs, so those loads wait
// for no scalar load.  The struct's lines are requested at once and awaited behind those loads (warm_args_land).  B fits 32
// bits: the tile path takes at most 16 tiles of 1024.
template <int G, int VEC, int EPG>
__global__ __launch_bounds__(1024) void k_tile_step(const int4* srt_u, const int4* srt_i, const int4* next_recs, int B, int nsort, int nblk_u,
                                                    int epg_item, int ntiles, int next_ntiles, int next_B, int stamps, TileStepArgs a) {
    const WarmLines<TileStepArgs> warm = warm_args_issue(a);
    constexpr int EPB = 1024 / G;                        // entries per piece = lane groups per block
    extern __shared__ __attribute__((aligned(16))) int32_t dyn[];   // sort: cnt[nbins]; then the wave-level sums
    __shared__ int32_t rec_u[1024], rec_i[1024], srt_key[1024], srt_pos[1024];
    __shared__ float rec_r[1024];
    __shared__ __attribute__((aligned(16))) float lds_gb[2 * EPG * 16];
    __shared__ __attribute__((aligned(16))) int32_t lds_key[EPG * 16];
    __shared__ float lds_stage[EPG * (2 * EPB + 1024)];
    __shared__ int32_t wtot[16];
    static_assert(sizeof(rec_u) + sizeof(rec_i) + sizeof(srt_key) + sizeof(srt_pos) + sizeof(rec_r) + sizeof(lds_gb) + sizeof(lds_key) +
                  sizeof(lds_stage) + sizeof(wtot) == tile_step_static_lds(G, EPG), "tile_step_static_lds() is out of date");
    static_assert(tile_step_static_lds(G, EPG) + 64 * 1024 <= LDS_PER_CU, "static LDS leaves no room for 16384 sort bins");
    TileStamp stamp = {nullptr, stamps ? __builtin_amdgcn_s_memrealtime() : 0ull};
    const int tid = threadIdx.x;
    const bool ahead = (int)blockIdx.x < nsort;          // look-ahead block: sort (side, tile) of the next batch
    const int b0 = (int)blockIdx.x - nsort;
    const int side = ahead ? (int)blockIdx.x / next_ntiles : (b0 < nblk_u ? 0 : 1);   // 0: user rows, 1: item rows
    const int bx = ahead ? 0 : (side ? b0 - nblk_u : b0);
    const int epg = side ? epg_item : EPG;
    const int EPS = EPB * epg;                           // entries per block
    const int NSL = 1024 / EPS;                          // blocks per tile
    const int tile = ahead ? (int)blockIdx.x % next_ntiles : bx / NSL;
    const int slice = bx % NSL;
    const int64_t tile0 = (int64_t)tile * 1024;
    const int Bt = ahead ? next_B : B;
    const int nvalid = (Bt - (int)tile0 < 1024) ? Bt - (int)tile0 : 1024;
    // the item side's last block: the pieces past the batch's end have no block - their {loss, reg, sum g} are zero.  Which
    // words, decided here from the preloaded scalars; written where a.partials is in hand (zero_tail)
    const int zero_from = (!ahead && side == 1 && (int64_t)(bx + 1) * EPS >= B) ? (bx + 1) * epg * 4 : INT32_MAX;
    const int zero_to = ntiles * G * 4;
    if (!ahead && slice * EPS >= nvalid) {               // a short last tile: nothing in this slice
        stamp.arm(a.dbg);
        zero_tail(a.partials, zero_from, zero_to);
        if (side == 1 && tid < 4 * epg) a.partials[(size_t)bx * epg * 4 + tid] = 0.f;
        return;
    }
    // A step block on the presorted path: a branch of its own, so that nothing the sorting blocks leave pending (their LDS
    // traffic shares a counter with the scalar loads) is waited for in front of the record loads.
    if (!ahead && srt_u != nullptr) {
        const int4* srt = side ? srt_i : srt_u;
        if constexpr (EPG > 1) {
            if (epg != EPG) {
                tile_pieces<G, VEC, EPG / 2, true>(a, dyn, rec_u, rec_i, rec_r, srt_key, srt_pos, lds_gb, lds_key, lds_stage, stamp, side, bx,
                                                   slice, tile0, nvalid, srt, warm, zero_from, zero_to);
                return;
            }
        }
        tile_pieces<G, VEC, EPG, true>(a, dyn, rec_u, rec_i, rec_r, srt_key, srt_pos, lds_gb, lds_key, lds_stage, stamp, side, bx, slice,
                                       tile0, nvalid, srt, warm, zero_from, zero_to);
        return;
    }
    {
        // a look-ahead block's own record, requested from the preloaded scalars before the struct's lines are awaited
        const bool early = ahead && next_recs != nullptr;
        int4 early_rec = make_int4(0, 0, 0, 0);
        if (early) early_rec = next_recs[tile0 + (tid < nvalid ? tid : 0)];     // (unconditional: slot 0 of a tile always exists)
        __builtin_amdgcn_sched_barrier(0);
        warm_args_land(warm);
        stamp.arm(a.dbg);
        zero_tail(a.partials, zero_from, zero_to);
        const int nb = a.nbins[side];
        tile_sort(dyn, rec_u, rec_i, rec_r, srt_key, srt_pos, wtot, ahead ? a.next_ids : a.ids, a.store, ahead ? next_recs : a.recs,
                  a.u, a.it, a.r, tile0, nvalid, side, nb, a.N, a.U, a.I, a.err, early, early_rec);
        const bool wt = a.wt & TFR_WT_PUBLISH;
        if (ahead) {                                     // publish the packed table and the sorted records
            int32_t* nt = a.next_tab[side];
            for (int b = tid; b < nb; b += 1024) store_word_p(nt, (size_t)tile * nb + b, (uint32_t)dyn[b], wt);
            if (tid < nvalid) {
                const int pl = srt_pos[tid];
                const int4 rec = make_int4(rec_u[pl], rec_i[pl], __float_as_int(rec_r[pl]), pl);
                if (wt) {
                    typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
                    uintx4 t; t.x = (unsigned)rec.x; t.y = (unsigned)rec.y; t.z = (unsigned)rec.z; t.w = (unsigned)rec.w;
                    __builtin_amdgcn_raw_buffer_store_b128(t, wt_rsrc(a.next_srt[side]), (int)((tile0 + tid) * 16), 0, 16);
                } else {
                    a.next_srt[side][tile0 + tid] = rec;
                }
            }
            return;
        }
        // the tile's packed lookup table, written once: its bins are dealt round the tile's active blocks
        const int nact = (nvalid + EPS - 1) / EPS;
        for (int b = slice * 1024 + tid; b < nb; b += nact * 1024) store_word_p(a.tab[side], (size_t)tile * nb + b, (uint32_t)dyn[b], wt);
        __syncthreads();                                 // cnt is dead from here: its memory takes the contributions
    }
    if constexpr (EPG > 1) {
        if (epg != EPG) {
            tile_pieces<G, VEC, EPG / 2, false>(a, dyn, rec_u, rec_i, rec_r, srt_key, srt_pos, lds_gb, lds_key, lds_stage, stamp, side, bx, slice,
                                                tile0, nvalid, nullptr, warm, zero_from, zero_to);
            return;
        }
    }
    tile_pieces<G, VEC, EPG, false>(a, dyn, rec_u, rec_i, rec_r, srt_key, srt_pos, lds_gb, lds_key, lds_stage, stamp, side, bx, slice, tile0,
                                    nvalid, nullptr, warm, zero_from, zero_to);
}

// the step part of k_tile_step for one block of EPG pieces (see above)
template <int G, int VEC, int EPG, bool PRE>
__device__ __forceinline__ void tile_pieces(const TileStepArgs& a, int32_t* dyn, const int32_t* rec_u, const int32_t* rec_i,
                                            const float* rec_r, const int32_t* srt_key, const int32_t* srt_pos, float* lds_gb,
                                            int32_t* lds_key, float* lds_stage, TileStamp& stamp, int side, int bx, int slice,
                                            int64_t tile0, int nvalid, const int4* srt, const WarmLines<TileStepArgs>& warm,
                                            int zero_from, int zero_to) {
    constexpr bool presorted = PRE;                      // PRE: the entries come from srt, this side's published records (a preloaded scalar)
    constexpr int EPB = 1024 / G;                        // entries per piece = lane groups per block
    constexpr int EPS = EPB * EPG;                       // entries per block
    const int tid = threadIdx.x;
    // ---- this block's entries (EPG per lane group, one from each piece): forward + contribution
    const int grp = tid / G, gl = tid % G, d0 = gl * VEC;
    int jl[EPG], bpos[EPG];
    int32_t row[EPG], uu[EPG], ii[EPG];
    float rr[EPG];
    bool ev[EPG], pstart[EPG];
    int4 rec_[EPG];
    int32_t prev_[EPG];
#pragma unroll
    for (int h = 0; h < EPG; ++h) {
        jl[h] = slice * EPS + h * EPB + grp;
        ev[h] = jl[h] < nvalid;
        rec_[h] = make_int4(0, 0, 0, 0); prev_[h] = -2;
    }
    if (presorted) {                                     // the published records of all EPG entries in one round trip (see the
#pragma unroll                                           // row gathers below for why they are not written `if (ev) rec = *sr`)
        for (int h = 0; h < EPG; ++h) {
            const int js = ev[h] ? jl[h] : 0;            // slot 0 of the tile always exists
            const int4* sr = srt + tile0 + js;
            rec_[h] = *sr;
            prev_[h] = reinterpret_cast<const int32_t*>(sr - (js > 0 ? 1 : 0))[side];
        }
        __builtin_amdgcn_sched_barrier(0);
        warm_args_land(warm);                            // nothing of the struct was needed up to here
        stamp.arm(a.dbg);
    }
    const int D = a.D;
    const float mu = *a.mu;
    if (presorted) zero_tail(a.partials, zero_from, zero_to);   // (the self-sorting blocks did both in front of their sort)
#pragma unroll
    for (int h = 0; h < EPG; ++h) {
        row[h] = -1; uu[h] = 0; ii[h] = 0; rr[h] = 0.f; bpos[h] = 0;
        int32_t prev = -2;
        if (ev[h]) {
            if (presorted) {
                const int4 rec = rec_[h];
                uu[h] = rec.x; ii[h] = rec.y; rr[h] = __int_as_float(rec.z); bpos[h] = rec.w;
                row[h] = side == 0 ? rec.x : rec.y;
                if (jl[h] > 0) prev = prev_[h];
            } else {
                row[h] = srt_key[jl[h]];
                if (jl[h] > 0) prev = srt_key[jl[h] - 1];
                bpos[h] = srt_pos[jl[h]];
                uu[h] = rec_u[bpos[h]]; ii[h] = rec_i[bpos[h]]; rr[h] = rec_r[bpos[h]];
            }
        }
        pstart[h] = ev[h] && (prev != row[h] || grp == 0);       // run head, or first entry of the piece
    }
    if (a.dbg) { if (row[0] == -12345) return; stamp.mark(2); }       // records have arrived
    // All row and bias gathers of the block's entries in flight together: unconditional loads from addresses that are
    // always valid (entry slots past the tile's end read row 0, lanes past the row's end its first words), a scheduling
    // barrier, and only then the zeroing of what did not count.  Written as `if (ev) p = load_frag(...)` the compiler
    // merged the loaded registers with the zeros of the other path by copies behind an s_waitcnt vmcnt(0), so the P row
    // of an entry had to arrive before its Q row was requested, and entry 0 before entry 1: three memory round trips
    // instead of one (ISA of k_tile_step<16,4,2>).
    Frag<VEC> p[EPG], q[EPG];
    float bu_[EPG], bi_[EPG];
    {
        const bool in = d0 < D;
        const int dd = in ? d0 : 0;
#pragma unroll
        for (int h = 0; h < EPG; ++h) {
            const float* pr = a.P + (size_t)(ev[h] ? uu[h] : 0) * D + dd;
            const float* qr = a.Q + (size_t)(ev[h] ? ii[h] : 0) * D + dd;
            if constexpr (VEC == 4) {
                const floatx4 tp = *reinterpret_cast<const floatx4*>(pr), tq = *reinterpret_cast<const floatx4*>(qr);
                p[h].v[0] = tp.x; p[h].v[1] = tp.y; p[h].v[2] = tp.z; p[h].v[3] = tp.w;
                q[h].v[0] = tq.x; q[h].v[1] = tq.y; q[h].v[2] = tq.z; q[h].v[3] = tq.w;
            } else {
                p[h].v[0] = *pr; q[h].v[0] = *qr;
            }
            bu_[h] = a.bu[ev[h] ? uu[h] : 0];
            bi_[h] = a.bi[ev[h] ? ii[h] : 0];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < EPG; ++h) {
            const bool keep = ev[h] && in;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { p[h].v[e] = keep ? p[h].v[e] : 0.f; q[h].v[e] = keep ? q[h].v[e] : 0.f; }
            bu_[h] = ev[h] ? bu_[h] : 0.f;
            bi_[h] = ev[h] ? bi_[h] : 0.f;
        }
    }
    Frag<VEC> acc[EPG];
    float gb[EPG];
    float facc[3 * EPG];                                 // per piece {loss, reg, sum g}: results do not depend on EPG
#pragma unroll
    for (int h = 0; h < 3 * EPG; ++h) facc[h] = 0.f;
#pragma unroll
    for (int h = 0; h < EPG; ++h) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[h].v[e] = 0.f;
        gb[h] = 0.f;
        float sdot = 0.f, sq = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float qv = q[h].v[e];
            sdot = fmaf(p[h].v[e], a.item_abs ? fabsf(qv) : qv, sdot);
            sq = fmaf(p[h].v[e], p[h].v[e], fmaf(qv, qv, sq));
        }
        sdot = group_sum<G>(sdot);
        if (ev[h]) {
            const float logit = ((sdot + mu) + bu_[h]) + bi_[h];   // ops.py:45-47 order
            float gk, l;
            if (a.loss == 0) {                           // ops.py:124
                gk = logit - rr[h];
                l = 0.5f * gk * gk;
            } else {                                     // ops.py:125-126
                gk = sigmoidf_(logit) - rr[h];
                l = fmaxf(logit, 0.f) - logit * rr[h] + log1pf(__expf(-fabsf(logit)));
            }
            if (side == 1) {
                if (gl == 0) {
                    if (a.logits) a.logits[tile0 + bpos[h]] = logit;
                    facc[3 * h + 0] = l;
                    facc[3 * h + 2] = gk;
                    if (a.reg_bias) sq = fmaf(bu_[h], bu_[h], fmaf(bi_[h], bi_[h], sq));
                }
                facc[3 * h + 1] = 0.5f * sq;             // tf.nn.l2_loss = sum(x^2)/2
            }
            const float ob = side == 0 ? bu_[h] : bi_[h];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float ov = side == 0 ? p[h].v[e] : q[h].v[e];
                float xv = side == 0 ? q[h].v[e] : p[h].v[e];
                if (side == 0) { if (a.item_abs) xv = fabsf(xv); }
                else if (a.item_abs) xv = xv * ((ov > 0.f) ? 1.f : ((ov < 0.f) ? -1.f : 0.f));
                acc[h].v[e] = fmaf(gk, xv, a.lam * ov);
            }
            gb[h] = a.reg_bias ? (gk + a.lam * ob) : gk;
        }
    }
    if (a.dbg) { if (gb[0] == -12345.f) return; stamp.mark(3); }      // rows have arrived, contributions formed
    // ---- K3 inside each piece, in two levels, every sum in a fixed order (bit-identical run to
    //      run however long the runs are):
    //      1. a wave holds GPW consecutive entries of the piece: suffix sums within runs by doubling,
    //         in registers (cross-lane moves, no LDS memory, no barrier);
    //      2. the 16 waves' leading-run sums: the same doubling over 16 values per piece through LDS
    //         (a value whose run ends within reach is final and drops out);
    //      3. an entry whose run reaches the end of its wave adds the next wave's total.
    //      TFR_ONE_BARRIER=1 (A/B, measured slower: DESIGN.md §8): instead of 2 and 3, after the one barrier that
    //      stages the wave values, a run head whose run reaches the end of its wave reads the keys of the piece's
    //      later waves and all their staged sums, and adds those of the waves its run covers, left to right.
    constexpr int GPW = 64 / G;
    const int wv = tid >> 6, gw = grp % GPW;
#pragma unroll
    for (int d = 1; d < GPW; d <<= 1) {
#pragma unroll
        for (int h = 0; h < EPG; ++h) {
            const int32_t krow = __shfl_down(row[h], d * G, 64);
            float xs[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) xs[e] = __shfl_down(acc[h].v[e], d * G, 64);
            const float xg = __shfl_down(gb[h], d * G, 64);
            if (ev[h] && gw + d < GPW && krow == row[h]) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[h].v[e] += xs[e];
                gb[h] += xg;
            }
        }
    }
    float* wbuf[2] = {reinterpret_cast<float*>(dyn), reinterpret_cast<float*>(dyn) + EPG * 16 * G * VEC};
    float* wgb[2] = {lds_gb, lds_gb + EPG * 16};
    bool reach[EPG], live[EPG];
    Frag<VEC> tacc[EPG];
    float tgb[EPG];
#pragma unroll
    for (int h = 0; h < EPG; ++h) {
        reach[h] = ev[h] && __shfl(row[h], (GPW - 1) * G + gl, 64) == row[h];     // run reaches the wave's last entry
        tacc[h] = acc[h];
        tgb[h] = gb[h];
        live[h] = gw == 0;                               // one lane group per wave carries the wave's value
        if (gw == 0) {
            const int w0 = h * 16 + wv;
#pragma unroll
            for (int e = 0; e < VEC; ++e) wbuf[0][(w0 * G + gl) * VEC + e] = tacc[h].v[e];
            if (gl == 0) { wgb[0][w0] = tgb[h]; lds_key[w0] = row[h]; }
        }
    }
    stamp.mark(4);                                       // wave-level sums staged
    if (side == 1) block_sum_pieces<G, EPG>(facc, lds_stage, a.partials + (size_t)bx * EPG * 4);   // has the barrier
    else __syncthreads();
    stamp.mark(5);
    int cur = 0;
    if (a.one_barrier) {
#pragma unroll
        for (int h = 0; h < EPG; ++h) {
            if (pstart[h] && reach[h] && wv + 1 < 16) {  // at most one lane group per wave and piece
                const int32_t* kp = lds_key + h * 16;
                const float* gp = wgb[0] + h * 16;
                int32_t key[16];
                float xgb[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int4 k4 = reinterpret_cast<const int4*>(kp)[q];
                    const float4 g4 = reinterpret_cast<const float4*>(gp)[q];
                    key[4 * q] = k4.x; key[4 * q + 1] = k4.y; key[4 * q + 2] = k4.z; key[4 * q + 3] = k4.w;
                    xgb[4 * q] = g4.x; xgb[4 * q + 1] = g4.y; xgb[4 * q + 2] = g4.z; xgb[4 * q + 3] = g4.w;
                }
                Frag<VEC> x[15];
#pragma unroll
                for (int k = 1; k < 16; ++k) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) x[k - 1].v[e] = wbuf[0][((h * 16 + k) * G + gl) * VEC + e];
                }
                bool run = true;                         // the waves after this one whose leading run is this run
#pragma unroll
                for (int k = 1; k < 16; ++k) {
                    if (k > wv) {
                        run = run && key[k] == row[h];
                        if (run) {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) acc[h].v[e] += x[k - 1].v[e];
                            gb[h] += xgb[k];
                        }
                    }
                }
            }
        }
        stamp.mark(6);                                   // the staged sums added
    } else {
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
#pragma unroll
            for (int h = 0; h < EPG; ++h) {
                if (live[h]) {
                    const int w0 = h * 16 + wv;
                    const bool take = row[h] >= 0 && wv + d < 16 && lds_key[w0 + d] == row[h];
                    if (take) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) tacc[h].v[e] += wbuf[cur][((w0 + d) * G + gl) * VEC + e];
                        tgb[h] += wgb[cur][w0 + d];
                    } else {
                        live[h] = false;
                    }
#pragma unroll
                    for (int e = 0; e < VEC; ++e) wbuf[cur ^ 1][(w0 * G + gl) * VEC + e] = tacc[h].v[e];
                    if (gl == 0) wgb[cur ^ 1][w0] = tgb[h];
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        stamp.mark(6);                                   // the four doubling rounds over the waves
#pragma unroll
        for (int h = 0; h < EPG; ++h) {
            const int w1 = h * 16 + wv + 1;
            if (reach[h] && wv + 1 < 16 && lds_key[w1] == row[h]) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[h].v[e] += wbuf[cur][(w1 * G + gl) * VEC + e];
                gb[h] += wgb[cur][w1];
            }
        }
    }
    const bool wt = a.wt & TFR_WT_PIECES;
#pragma unroll
    for (int h = 0; h < EPG; ++h) {
        if (pstart[h]) {
            const int64_t j = tile0 + jl[h];
            store_frag_p<VEC>(a.grad_rows[side], (size_t)j * D, d0, D, acc[h], wt);
            if (gl == 0) store_word_p(a.grad_bias[side], (size_t)j, __float_as_uint(gb[h]), wt);
        }
    }
}

// K0  triple gather from the HBM-resident (user,item,rate) store: what
//     ShuffleIterator.next does on the host (dataio.py:115-117), ids drawn by the host.
//     (the training path fuses this into K1; this kernel serves forward_resident)
__global__ __launch_bounds__(256) void k_gather_triples(GatherArgs a) {
    bool oob = false;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.B;
         k += (int64_t)gridDim.x * blockDim.x) {
        int64_t id = a.ids ? a.ids[k] : a.lo + k;
        if ((uint64_t)id >= (uint64_t)a.N) { oob = true; id = 0; }
        const int4 rec = a.store[id];
        a.u[k] = rec.x;
        a.it[k] = rec.y;
        a.r[k] = __int_as_float(rec.z);
    }
    if (oob) atomicOr(a.err, 2);
}

// row fetch for a peer shard: rows_out[j] = table[ids[j]], bias_out[j] = bias[ids[j]]
template <int G, int VEC>
__global__ __launch_bounds__(256) void k_gather_rows(GatherRowsArgs a) {
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int d0 = gl * VEC;
    bool oob = false;
    for (int64_t j = (int64_t)blockIdx.x * GPB + threadIdx.x / G; j < a.n; j += (int64_t)gridDim.x * GPB) {
        int32_t id = a.ids[j];
        if ((uint64_t)(int64_t)id >= (uint64_t)a.rows) { oob = true; id = 0; }
        const Frag<VEC> f = load_frag<VEC>(a.table + (size_t)id * a.D, d0, a.D);
        store_frag<VEC>(a.rows_out + (size_t)j * a.D, d0, a.D, f);
        if (gl == 0) a.bias_out[j] = a.bias[id];
    }
    if (oob) atomicOr(a.err, 1);
}

// columns -> 16-byte records of the resident rating store
__global__ __launch_bounds__(256) void k_pack_triples(const int32_t* u, const int32_t* it, const float* r,
                                                     int4* store, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
         k += (int64_t)gridDim.x * blockDim.x)
        store[k] = make_int4(u[k], it[k], __float_as_int(r[k]), 0);
}

// (the optimiser arithmetic, AdamC and adam_sparse, is in svd_kernels.h: the wave-per-run kernels share it)

// ------------------------------------------------------------------------------------
// K3  deterministic segmented reduce over a table's rows (backward of embedding_lookup:
//     IndexedSlices -> unique + unsorted_segment_sum [TF1-lib], ops.py:143-149).
//     Input: batch positions stably sorted by row id (ks = sorted ids, ps = positions).
//     One 1024-thread block owns EPB = 1024/G consecutive sorted entries (a PIECE), one
//     lane group per entry:
//       phase 1 (all groups in parallel, no walk): the entry's contribution
//          user side: t = g_k * Qt[i_k] + lam * P[u]          Qt = |Q| if item_abs
//          item side: t = g_k * P[u_k] * s + lam * Q[i]       s = sign(Q[i]) if item_abs
//          bias     : t = g_k (+ lam * b[row] if reg_bias)          
//        goes to LDS;
//       phase 2: the group at each piece start (run head, or first entry of the block) adds
//        its run's contributions from LDS in entry order = batch order.
//     A run's total is its pieces added in piece order: a fixed order, so results are
//     run-to-run bit-identical, and the work is balanced however skewed the ids are.
//     RMODE_SCRATCH : every piece sum -> scratch[piece start] (+ map[row] = head+1 for tf1)
//     RMODE_ADAM/SGD: a run that lies inside one block is applied in place at once (fused lazy
//                     Adam / SGD); split runs go to scratch and k_apply_rows finishes them.
//     Both sides run fused: the item side goes first and copies each entry's pre-update Q row
//     to own_copy_out[pos]; the user side then takes its partner rows from that copy
//     (partner_by_pos), so neither side sees a row the other has already moved.
//     FAST (full-width rows; the fused big-table step, the row-sharded step's sides and owners' apply, the FM backward -
//     launch_seg_reduce checks the conditions): the same arithmetic with the loads issued in three dependent rounds instead
//     of eight - {sorted id, neighbour, position}, then the words the row id / position alone address (partner id, table
//     selector, rating or g, biases) with the rows the row id alone addresses behind them (m / v, the user side's own row),
//     then the partner row and the item side's own row - so a block spends one HBM latency on its rows, not three in a row.
template <int G, int VEC, int RMODE, bool FWD = false, bool LEAN = true, bool FAST = false>
__global__ __launch_bounds__(1024) void k_seg_reduce(RedPair pr) {
    // (no warm_args here: thousands of workgroups per launch, the lines are in the scalar cache after the first ones - it cost
    // the user side 172 -> 180 us and, at 64 VGPRs, the item side a block per CU)
    constexpr bool MV_BRANCH = FWD;                      // FAST item side: m / v rows loaded under `if (head)` only, never merged with zeros
    constexpr int EPB = 1024 / G;
    __shared__ float lds_t[EPB * G * VEC];
    __shared__ float lds_gb[EPB];
    __shared__ int32_t lds_key[EPB];
    __shared__ float lds_stage[FWD ? 2 * EPB + 1024 : 1];
    // FAST item side with the forward inside: the own row waits in LDS for the update after the walk (it cannot stay in
    // registers - four of them decide whether two blocks fit a CU - and re-reading it from memory is a round trip in every
    // block's tail and, the first read being a streaming one, 118 MB of traffic per launch at C3's shape)
    constexpr bool OWN_LDS = FAST && FWD && LEAN && RMODE == RMODE_ADAM;
    __shared__ float lds_o[OWN_LDS ? EPB * G * VEC : 1];
    static_assert(sizeof(lds_t) + sizeof(lds_gb) + sizeof(lds_key) + sizeof(lds_stage) + (FWD ? 16 * 3 * 4 : 0) + (OWN_LDS ? sizeof(lds_o) : 0)
                      <= seg_reduce_static_lds(G, VEC, FWD), "seg_reduce_static_lds() is out of date");
    const RedArgs& a = pr.a[blockIdx.y];
    const int32_t err = *a.err;
    const int grp = threadIdx.x / G;
    const int gl = threadIdx.x % G;
    const int d0 = gl * VEC;
    const int D = a.D;
    const int64_t blk0 = (int64_t)blockIdx.x * EPB;
    const int64_t j = blk0 + grp;
    const int64_t Bn = a.dB ? (int64_t)*a.dB : a.B;      // row-sharded step: the entry count lives on the device
    const bool valid = j < Bn;
    int32_t row = -1, prev = -2, pos = 0;
    if (valid) {                                         // three independent loads, one round trip
        row = a.ks[j];
        pos = a.ps[j];
        prev = a.ks[j > 0 ? j - 1 : 0];
        if (j == 0) prev = -2;
    }
    if (err || blk0 >= Bn) {                 // an out-of-range id voids the whole step (block-uniform)
        // a grid sized for a capacity (row-sharded step: the entry count lives on the device): the blocks past the
        // entries still owe K4 their - empty - partial sums
        if constexpr (FWD) { if (!err && a.dB && threadIdx.x < 4) a.partials[(size_t)blockIdx.x * 4 + threadIdx.x] = 0.f; }
        return;
    }
    // the key the next block starts with (does this block's last run continue there?): block-uniform, asked for now and not
    // after the walk, where it was one more dependent round trip at the end of every block
    const int32_t nextkey = (blk0 + EPB < Bn) ? a.ks[blk0 + EPB] : -3;
    // tile mode: the sorted order is per 1024-entry tile, so a run also starts at every tile start
    const bool head = valid && (prev != row || (a.tile && (j % a.tile) == 0));
    const bool pstart = valid && (head || grp == 0);
    const AdamC c = {a.alpha, a.b1, a.b2, a.eps, 1.f - a.b1, 1.f - a.b2};
    const size_t roff = (size_t)(valid ? row : 0) * D;
    const size_t ooff = a.ostride ? (size_t)(valid ? row : 0) * a.ostride : roff;     // own rows read from a packed exchange buffer
    const size_t oboff = a.obstride ? (size_t)(valid ? row : 0) * a.obstride : (size_t)(valid ? row : 0);

    Frag<VEC> o, t, mrow, vrow;
    float ob = 0.f, tb = 0.f, mb = 0.f, vb = 0.f;
    int32_t cur = 0;                                     // two-table form: the table this entry's own row is in
    float facc[3] = {0.f, 0.f, 0.f};                     // FWD: this lane's {loss, reg, g} share
#pragma unroll
    for (int q = 0; q < VEC; ++q) { o.v[q] = 0.f; t.v[q] = 0.f; }
    if constexpr (!(FAST && MV_BRANCH)) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) { mrow.v[q] = 0.f; vrow.v[q] = 0.f; }
    }
    bool owner_side = false;
    if constexpr (!FAST) owner_side = valid && a.rows_in;
    // FAST: the loads, branch-free (lanes past the entries and non-head lanes read row / position 0 and drop the result) and in
    // three rounds.  `cond ? a.p : a.q` on two kernel-argument pointers would be compiled into a VECTOR load of the pointer from
    // the argument block at a selected offset - a dependent round trip of its own; the table is chosen by an offset instead.
    Frag<VEC> xf;
    // (lam through a scalar-register read: `ent ? record.z : a.lam` would otherwise become ONE vector load from a selected
    // address - the argument block or the record - with a round trip of its own)
    float pbf = 0.f, rvf = 0.f, gkf = 0.f, lamf = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.lam)));
    int32_t pidf = 0;
    bool fast_owner = false;
    if constexpr (FAST && !FWD) fast_owner = a.rows_in != nullptr;
    if (fast_owner) {
        // owner side of the row-sharded step: the contributions are gradient rows already reduced by the peers (by arrival
        // position); everything is addressed by the row id / position alone - one round
        const int32_t rowh = head ? row : 0;
        const int rstr = a.rstride ? a.rstride : D;
        t = load_full<VEC, true>(a.rows_in + (size_t)pos * rstr + d0);
        tb = a.bias_in[(size_t)pos * (a.rbstride ? a.rbstride : 1)];
        o = load_full<VEC, true>(a.own + roff + d0);
        ob = a.own_bias[valid ? row : 0];
        if constexpr (RMODE == RMODE_ADAM) {
            const size_t mvoff = (head ? roff : 0) + d0;
            mrow = load_full<VEC, true>(a.m + mvoff);
            vrow = load_full<VEC, true>(a.v + mvoff);
            mb = a.bias_m[rowh];
            vb = a.bias_v[rowh];
        }
        if (!valid) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) t.v[q] = 0.f;
            tb = 0.f;
        }
    } else if constexpr (FAST) {
        const int32_t rowc = valid ? row : 0;
        const int32_t rowh = head ? row : 0;
        // round 2: the words the row id / position alone address (ids, selector, rating or g, biases: caches)
        const bool two_p = a.osel_in != nullptr;         // partner ids carry the table bit (two-table form, user side)
        const int32_t* idp = two_p ? a.osel_in : a.other;
        int32_t pidw;
        if constexpr (FWD) {
            pidw = idp[pos];
            rvf = a.r[pos];
        } else if (a.ent) {                              // FM: partner row, g x and the entry's coefficient in one 16-byte record
            const int4 e = a.ent[pos];
            pidw = e.x; gkf = __int_as_float(e.y); lamf = __int_as_float(e.z);
        } else {
            pidw = idp[pos];
            gkf = a.g[pos];
        }
        const int32_t* selp = a.sel ? a.sel : a.ks;      // no selector: a word that is there anyway, dropped
        int32_t curw = selp[a.sel ? rowc : 0];
        if (!a.sel) curw = 0;
        ob = a.own_bias[(size_t)rowc * (a.obstride ? a.obstride : 1)];
        if constexpr (RMODE == RMODE_ADAM) {
            mb = a.bias_m[rowh];
            vb = a.bias_v[rowh];
        }
        // the rows.  What needs the row id only goes out now, BEHIND the words above in issue order (compiler barriers; the
        // counter of outstanding loads retires in order, so the wait for the partner id and the selector leaves these in
        // flight): the side without a selector (user side, FM) asks for its own row and the m / v rows, the item side for the
        // m / v rows of run heads (a fifth of its entries repeat a row and skip them: 190 -> 184 us, Zipf 146 -> 136; the user
        // side - hardly any repeats - reads row 0 for them and stays branch-free, 175.5 against 177.3 us).
        pidf = two_p ? (pidw & 0x7fffffff) : pidw;
        const int ostr = a.ostride ? a.ostride : D, pstr = a.pstride ? a.pstride : D;
        constexpr bool EARLY = !FWD;
        asm volatile("" ::: "memory");
        if constexpr (EARLY) {
            o = load_full<VEC, true>(a.own + ((size_t)rowc * ostr + d0));
            if constexpr (RMODE == RMODE_ADAM) {
                const size_t mvoff = (head ? roff : 0) + d0;
                mrow = load_full<VEC, true>(a.m + mvoff);
                vrow = load_full<VEC, true>(a.v + mvoff);
            }
        } else if constexpr (RMODE == RMODE_ADAM) {
            if (head) {
                mrow = load_full<VEC, true>(a.m + roff + d0);
                vrow = load_full<VEC, true>(a.v + roff + d0);
            }
        }
        asm volatile("" ::: "memory");
        // last round: the partner row (and the item side's own row, whose table the selector names).  `tok` is 0, but the
        // compiler only learns that from an instruction that reads the partner id and the selector: these addresses carry it,
        // so the loads cannot be scheduled ahead of the wait for those two words
        int32_t tok;
        asm volatile("v_mov_b32 %0, 0" : "=v"(tok) : "v"(pidw), "v"(curw));
        cur = EARLY ? 0 : curw;
        const int d0t = d0 + tok;
        const ptrdiff_t oalt = a.own_alt ? a.own_alt - a.own : 0;
        const ptrdiff_t palt = two_p ? a.partner_alt - a.partner : 0;
        xf = load_full<VEC, true>(a.partner + ((ptrdiff_t)((size_t)pidf * pstr + d0t) + ((pidw < 0) ? palt : 0)));
        // (the item side's own rows are the user side's partner rows a moment later: default policy, so that they stay cached)
        if constexpr (!EARLY) o = load_full<VEC, !OWN_LDS>(a.own + ((ptrdiff_t)((size_t)rowc * ostr + d0t) + (cur ? oalt : 0)));
        if constexpr (FWD) pbf = a.partner_bias[pidf];
    }
    if (fast_owner) {
        // loaded above
    } else if (owner_side) {
        // owner side of the sharded step: the contribution is a gradient row already reduced by
        // a peer (it includes that peer's lam * Q[i] terms); just add them up in arrival order
        t = load_frag<VEC>(a.rows_in + (size_t)pos * (a.rstride ? a.rstride : D), d0, D);
        tb = a.bias_in[(size_t)pos * (a.rbstride ? a.rbstride : 1)];
        o = load_frag<VEC>(a.own + roff, d0, D);
        ob = a.own_bias[row];
        if constexpr (RMODE == RMODE_ADAM) {
            if (head) {
                mrow = load_frag<VEC>(a.m + roff, d0, D);
                vrow = load_frag<VEC>(a.v + roff, d0, D);
                mb = a.bias_m[row];
                vb = a.bias_v[row];
            }
        }
    } else if (valid) {
        float gk = 0.f;
        int32_t pid = 0;
        float lam_e;
        const float* ptab = a.partner;
        bool have = false;
        float pb = 0.f, rv = 0.f;                        // FWD: partner bias, rating
        Frag<VEC> x;
      if constexpr (FAST) {
        x = xf; pb = pbf; rv = rvf; gk = gkf; pid = pidf;
        lam_e = lamf;
        if constexpr (FWD) { if (gl == 0 && a.osel_out) a.osel_out[pos] = row | (cur << 31); }
      } else {
        if constexpr (!FWD) {
            if (a.ent) {                                             // FM: one 16-byte record per entry
                const int4 e = a.ent[pos];
                pid = e.x; gk = __int_as_float(e.y); lam_e = __int_as_float(e.z);
                have = true;
            }
        }
        if (!have) {
            if constexpr (!FWD) gk = a.g[pos];
            pid = a.partner_by_pos ? 0 : (a.osel_in ? a.osel_in[pos] : a.other[pos]);   // not needed when the partner row comes by position
            if (a.osel_in) { if (pid < 0) ptab = a.partner_alt; pid &= 0x7fffffff; }   // the table that still holds the pre-update row
            lam_e = a.lam;
        }
        x = a.partner_by_pos ? load_frag_h<VEC>(a.partner_by_pos + (size_t)pos * D, d0, D, a.nt & 8)
                             : load_frag_h<VEC>(ptab + (size_t)pid * (a.pstride ? a.pstride : D), d0, D, a.nt & 1);
        if (a.sel) {                                                 // two-table form: which table holds this row now
            cur = a.sel[row];
            if (gl == 0) a.osel_out[pos] = row | (cur << 31);
        }
        o = load_frag_h<VEC>((cur ? a.own_alt : a.own) + ooff, d0, D, a.nt & 2);
        ob = a.own_bias[oboff];
        if constexpr (RMODE == RMODE_ADAM) {
            if (head) {
                mrow = load_frag_h<VEC>(a.m + roff, d0, D, a.nt & 2);
                vrow = load_frag_h<VEC>(a.v + roff, d0, D, a.nt & 2);
                mb = a.bias_m[row];
                vb = a.bias_v[row];
            }
        }
        // this side updates its table in place before the other side runs: leave the other side the
        // pre-update row it needs, per entry
        if (a.own_copy_out) store_frag_h<VEC>(a.own_copy_out + (size_t)pos * D, d0, D, o, a.nt & 16);
        if constexpr (FWD) { pb = a.partner_bias[pid]; rv = a.r[pos]; }
      }
        if constexpr (FWD) {
            // K1 on the rows already in registers (item side: partner = P[u], own = Q[i]); same
            // arithmetic and order as forward_body
            float sdot = 0.f, sq = 0.f;
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const float qv = o.v[q];
                sdot = fmaf(x.v[q], a.item_abs ? fabsf(qv) : qv, sdot);
                sq = fmaf(x.v[q], x.v[q], fmaf(qv, qv, sq));
            }
            sdot = group_sum<G>(sdot);
            const float logit = ((sdot + *a.mu) + pb) + ob;
            const float r = rv;
            float l;
            if (a.loss == 0) {
                gk = logit - r;
                l = 0.5f * gk * gk;
            } else {
                gk = sigmoidf_(logit) - r;
                l = fmaxf(logit, 0.f) - logit * r + log1pf(__expf(-fabsf(logit)));
            }
            if (gl == 0) {
                a.g_out[pos] = gk;
                if (a.logits_out) a.logits_out[pos] = logit;
                facc[0] = l;
                facc[2] = gk;
                if (a.reg_bias) sq = fmaf(pb, pb, fmaf(ob, ob, sq));
            }
            facc[1] = 0.5f * sq;
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            float xv = x.v[q];
            if (a.side == 0) { if (a.item_abs) xv = fabsf(xv); }
            else if (a.item_abs) xv = xv * ((o.v[q] > 0.f) ? 1.f : ((o.v[q] < 0.f) ? -1.f : 0.f));
            t.v[q] = fmaf(gk, xv, lam_e * o.v[q]);        // pinned: left to the compiler, the fused product differed between instantiations
        }
        tb = a.reg_bias ? (gk + a.lam * ob) : gk;
    }
    // contributions to LDS ([entry][G*VEC], a lane's VEC floats contiguous)
#pragma unroll
    for (int q = 0; q < VEC; ++q) lds_t[(grp * G + gl) * VEC + q] = t.v[q];
    if constexpr (OWN_LDS) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) lds_o[(grp * G + gl) * VEC + q] = o.v[q];
    }
    if (gl == 0) { lds_gb[grp] = tb; lds_key[grp] = row; }
    if constexpr (FWD) {                                 // has the barrier
        if (a.stage_sum) block_sum_pieces<G, 1>(facc, lds_stage, a.partials + (size_t)blockIdx.x * 4);
        else block_sum_store<3, 16>(facc, a.partials + (size_t)blockIdx.x * 4);
    } else __syncthreads();
    if (!pstart) return;

    // where the row is (two-table form: the table sel[row] named) and where its new value goes (the other table)
    const ptrdiff_t walt = a.sel ? a.own_w_alt - a.own_w : 0;
    const float* const wsrc = a.own_w + ((ptrdiff_t)roff + (cur ? walt : 0));
    float* const wdst = a.own_w + ((ptrdiff_t)roff + (cur ? 0 : walt));
    // FWD variant: the own row is re-read (an L2 hit) rather than kept live across the forward and the walk - four registers
    // that decide whether two blocks fit a CU; FAST asks for it before the walk, not after it
    Frag<VEC> wre;
    if constexpr (OWN_LDS) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) wre.v[q] = lds_o[(grp * G + gl) * VEC + q];
    }

    Frag<VEC> acc = t;
    float gb = tb;
    int e = grp + 1;
    for (;;) {                                           // four LDS entries per round trip, added in order
        bool same[4];
        float xv[4][VEC], xb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ee = (e + q < EPB) ? e + q : grp;   // in-bounds address; masked by same[]
            same[q] = (e + q < EPB) && (lds_key[ee] == row);
#pragma unroll
            for (int c2 = 0; c2 < VEC; ++c2) xv[q][c2] = lds_t[(ee * G + gl) * VEC + c2];
            xb[q] = lds_gb[ee];
        }
        bool go = true;
        int taken = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            go = go && same[q];
            if (go) {
#pragma unroll
                for (int c2 = 0; c2 < VEC; ++c2) acc.v[c2] += xv[q][c2];
                gb += xb[q];
                ++taken;
            }
        }
        e += taken;
        if (!go) break;
    }
    bool cont = false;                                   // does the run continue in the next block?
    if (e == EPB && blk0 + EPB < Bn && !(a.tile && ((blk0 + EPB) % a.tile) == 0)) cont = (nextkey == row);
    const bool whole = head && !cont;
    if (RMODE == RMODE_SCRATCH && whole && a.dense_rows) {
        // dense-gradient form (TF1 Adam sweep / data parallel): a run that lies in one block goes
        // straight to its row of the dense buffer - the consumer streams it with no indirection
        store_frag<VEC>(a.dense_rows + (a.dstride ? (size_t)row * a.dstride : roff), d0, D, acc);
        if (gl == 0) a.dense_bias[a.dbstride ? (size_t)row * a.dbstride : (size_t)row] = gb;
    } else if (RMODE == RMODE_SCRATCH || !whole) {
        store_frag<VEC>(a.grad_rows + (size_t)j * D, d0, D, acc);
        if (gl == 0) {
            a.grad_bias[j] = gb;
            if (head && a.map) a.map[row] = (int32_t)j + 1;      // split run: where its pieces start
        }
    } else if constexpr (RMODE == RMODE_ADAM) {
        if (!a.frozen_rows) {
            Frag<VEC> w;
            if constexpr (OWN_LDS) w = wre;
            else w = (FWD && LEAN) ? load_frag<VEC>(wsrc, d0, D) : o;
#pragma unroll
            for (int q = 0; q < VEC; ++q) adam_sparse(w.v[q], mrow.v[q], vrow.v[q], acc.v[q], c);
            // two-table form: the new row goes to the other table (the user side still reads the old one), then the row flips
            const bool nts = FAST || (a.nt & 4);
            store_frag_h<VEC>(wdst, d0, D, w, nts);
            if (a.sel && gl == 0) a.sel[row] = cur ^ 1;
            store_frag_h<VEC>(a.m + roff, d0, D, mrow, nts);
            store_frag_h<VEC>(a.v + roff, d0, D, vrow, nts);
        }
        if (gl == 0 && !a.frozen_bias) {
            float w = ob;
            adam_sparse(w, mb, vb, gb, c);
            a.bias_w[row] = w;
            a.bias_m[row] = mb;
            a.bias_v[row] = vb;
        }
    } else if constexpr (RMODE == RMODE_SGD) {
        if (!a.frozen_rows) {
            Frag<VEC> w = o;
#pragma unroll
            for (int q = 0; q < VEC; ++q) w.v[q] = w.v[q] - a.lr * acc.v[q];
            store_frag<VEC>(wdst, d0, D, w);
            if (a.sel && gl == 0) a.sel[row] = cur ^ 1;
        }
        if (gl == 0 && !a.frozen_bias) a.bias_w[row] = ob - a.lr * gb;
    }
}

// a run's reduced gradient = its pieces added in piece order (head piece first); pieces
// start at the run head and at every multiple of PIECE (= the reduce kernel's block span).
// Continuation pieces are probed and loaded N at a time (independent loads, added in the order walked), so a hot row
// split into a handful of pieces costs two memory round trips, not one per piece.  `step` = distance between the
// pieces this caller walks (PIECE for all of them, a multiple when several lane groups share a run).
template <int VEC, int N>
__device__ __forceinline__ bool add_pieces(Frag<VEC>& t, float& gb, const float* __restrict__ grad_rows,
                                           const float* __restrict__ grad_bias, const int32_t* __restrict__ ks,
                                           int64_t B, int64_t safe, int64_t p, int64_t step, int32_t row, int d0, int D) {
    int32_t key[N];                                      // unconditional loads from in-bounds addresses: a load behind
#pragma unroll                                           // `pp < B &&` is a branch and a full wait per probe
    for (int q = 0; q < N; ++q) {
        const int64_t pp = p + (int64_t)q * step;
        key[q] = ks[pp < B ? pp : safe];
    }
    Frag<VEC> x[N];
    float xb[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const int64_t pp = (p + (int64_t)q * step < B) ? p + (int64_t)q * step : safe;
        x[q] = load_frag<VEC>(grad_rows + (size_t)pp * D, d0, D);
        xb[q] = grad_bias[pp];
    }
    bool go = true;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        go = go && (p + (int64_t)q * step < B) && key[q] == row;     // pieces are contiguous: stop at the first miss
        if (go) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) t.v[e] += x[q].v[e];
            gb += xb[q];
        }
    }
    return go;
}

// the narrow walk (k_adam_dense, where registers decide the sweep's occupancy): eight pieces per round trip
template <int VEC, int PIECE>
__device__ __forceinline__ Frag<VEC> run_total(const float* __restrict__ grad_rows,
                                               const float* __restrict__ grad_bias,
                                               const int32_t* __restrict__ ks, int64_t B, int64_t j,
                                               int32_t row, int d0, int D, float& gb) {
    Frag<VEC> t = load_frag<VEC>(grad_rows + (size_t)j * D, d0, D);
    gb = grad_bias[j];
    int64_t p = (j / PIECE + 1) * PIECE;
    if (p >= B || ks[p] != row) return t;                // the common case: a single piece
    while (add_pieces<VEC, 8>(t, gb, grad_rows, grad_bias, ks, B, j, p, PIECE, row, d0, D)) p += 8 * (int64_t)PIECE;
    return t;
}

// ------------------------------------------------------------------------------------
// K5a  apply reduced gradients held in scratch to the touched rows only: lazy Adam or SGD
//      (ops.py:143-149).  One lane group per sorted entry; only run heads work.
//      only_split: finish the runs k_seg_reduce could not apply in place (cut in >1 piece).
//      A hot row (popularity-skewed ids: under Zipf(1.05) items the top row of a 262144 batch is cut into ~800
//      pieces) is shared by the block: the owner adds the head piece and the next eight as run_total does; if all
//      eight belonged to the run, lane group g of the block adds pieces 9+g, 9+g+GPB, ... (16 in flight each) and the
//      owner adds the GPB partial sums in group order - a fixed order, so results stay bit-identical run to run.
template <int G, int VEC, int OPT>
__global__ __launch_bounds__(256) void k_apply_rows(ApplyPair pr) {
    warm_args(pr.a[blockIdx.y]);
    constexpr int PIECE = 1024 / G;
    constexpr int GPB = 256 / G;
    constexpr int CW = 16;                               // pieces in flight per lane group in the shared walk
    if (pr.with_fin && blockIdx.x == gridDim.x - 1) {    // the extra block column: K4 (block-uniform branch)
        if (blockIdx.y == 0) finalize_body(pr.f);
        return;
    }
    __shared__ float s_part[256 * VEC];
    __shared__ float s_partb[GPB];
    __shared__ long long s_next[GPB];                    // a long run's next piece position, or -1
    __shared__ int32_t s_row[GPB];
    const ApplyArgs& a = pr.a[blockIdx.y];
    const int32_t err = *a.err;
    const int gl = threadIdx.x % G, grp = threadIdx.x / G;
    const int d0 = gl * VEC;
    const int D = a.D;
    const int64_t Bn = a.dB ? (int64_t)*a.dB : a.B;      // row-sharded step: the entry count lives on the device
    int64_t j = (int64_t)blockIdx.x * GPB + grp;
    int32_t row = 0;
    bool own;                                            // this lane group finishes a run (no early exits: barriers below)
    if (a.only_split) {
        // one lane group per piece boundary p: a run is split iff it crosses one.  The first
        // boundary a run crosses owns it; its head then lies in the PIECE entries before p.
        const int64_t p = (j + 1) * PIECE;
        own = !err && p < Bn;
        if (own) {
            row = a.ks[p];
            const int64_t lo = p - PIECE;
            own = a.ks[p - 1] == row && !(lo > 0 && a.ks[lo - 1] == row);   // crossed here, and not an earlier boundary
            if (own) {
                const int sh = ((threadIdx.x % 64) / G) * G;     // this group's lanes within the wave
                j = p - 1;
                for (int k = 0; k < PIECE; k += G) {             // sorted keys: the matches are a suffix of [lo, p)
                    const bool hit = (k + gl < PIECE) && a.ks[lo + k + gl] == row;
                    unsigned long long bits = __ballot(hit) >> sh;
                    if constexpr (G < 64) bits &= (1ull << G) - 1ull;
                    if (bits) { j = lo + k + (__ffsll((long long)bits) - 1); break; }
                }
            }
        }
    } else {
        own = !err && j < Bn;
        if (own) {
            row = a.ks[j];
            own = ((j > 0) ? a.ks[j - 1] : -2) != row;           // run heads only
        }
    }
    const size_t roff = (size_t)row * D;
    Frag<VEC> w, mrow, vrow, gr;
#pragma unroll
    for (int q = 0; q < VEC; ++q) { w.v[q] = 0.f; mrow.v[q] = 0.f; vrow.v[q] = 0.f; gr.v[q] = 0.f; }
    float gb = 0.f;
    long long next = -1;
    float* wtab = a.w;
    if (own) {
        if (a.sel && a.sel[row]) wtab = a.w_alt;          // two-table form: finish the row where it lives
        if (OPT != 2 && !a.frozen_rows) {                // issued before the piece walk
            w = load_frag<VEC>(wtab + roff, d0, D);
            if constexpr (OPT == 0) {
                mrow = load_frag<VEC>(a.m + roff, d0, D);
                vrow = load_frag<VEC>(a.v + roff, d0, D);
            }
        }
        gr = load_frag<VEC>(a.grad_rows + (size_t)j * D, d0, D);
        gb = a.grad_bias[j];
        const int64_t p = (j / PIECE + 1) * PIECE;
        if (p < Bn && a.ks[p] == row &&
            add_pieces<VEC, 8>(gr, gb, a.grad_rows, a.grad_bias, a.ks, Bn, j, p, PIECE, row, d0, D))
            next = p + 8 * (int64_t)PIECE;
    }
    if (gl == 0) { s_next[grp] = next; s_row[grp] = row; }
    if (__syncthreads_or(next >= 0)) {                   // some run of this block is long: share it
        for (int sl = 0; sl < GPB; ++sl) {
            const long long ps = s_next[sl];             // block-uniform
            if (ps < 0) continue;
            const int32_t rs = s_row[sl];
            Frag<VEC> part;
#pragma unroll
            for (int q = 0; q < VEC; ++q) part.v[q] = 0.f;
            float pb = 0.f;
            int64_t pp = ps + (int64_t)grp * PIECE;
            while (add_pieces<VEC, CW>(part, pb, a.grad_rows, a.grad_bias, a.ks, Bn, 0, pp, (int64_t)GPB * PIECE, rs, d0, D))
                pp += (int64_t)CW * GPB * PIECE;
#pragma unroll
            for (int q = 0; q < VEC; ++q) s_part[threadIdx.x * VEC + q] = part.v[q];
            if (gl == 0) s_partb[grp] = pb;
            __syncthreads();
            if (grp == sl) {
                for (int g2 = 0; g2 < GPB; ++g2) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) gr.v[q] += s_part[(g2 * G + gl) * VEC + q];
                    gb += s_partb[g2];
                }
            }
            __syncthreads();
        }
    }
    if (!own) return;
    const AdamC c = {a.alpha, a.b1, a.b2, a.eps, 1.f - a.b1, 1.f - a.b2};
    if constexpr (OPT == 2) {                            // sharded step: emit the reduced gradient row
        store_frag<VEC>(a.w + (a.wstride ? (size_t)row * a.wstride : roff), d0, D, gr);
        if (gl == 0) a.bias_w[a.wbstride ? (size_t)row * a.wbstride : (size_t)row] = gb;
        return;
    }
    if (!a.frozen_rows) {
        if constexpr (OPT == 0) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) adam_sparse(w.v[q], mrow.v[q], vrow.v[q], gr.v[q], c);
            store_frag<VEC>(a.m + roff, d0, D, mrow);
            store_frag<VEC>(a.v + roff, d0, D, vrow);
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) w.v[q] = w.v[q] - a.lr * gr.v[q];
        }
        store_frag<VEC>(wtab + roff, d0, D, w);
    }
    if (gl == 0 && !a.frozen_bias) {
        float bw = a.bias_w[row];
        if constexpr (OPT == 0) {
            float mb = a.bias_m[row], vb = a.bias_v[row];
            adam_sparse(bw, mb, vb, gb, c);
            a.bias_m[row] = mb;
            a.bias_v[row] = vb;
        } else {
            bw = bw - a.lr * gb;
        }
        a.bias_w[row] = bw;
    }
}

// ------------------------------------------------------------------------------------
// K5b  TF1 "sparse" Adam = dense sweep: every row decays m, v and moves;
//      touched rows (map[row] = head+1) add their reduced gradient.  One lane group per
//      row, consecutive groups on consecutive rows -> fully coalesced streaming.  The map
//      entry is cleared by the group that consumed it.
template <int G, int VEC>
__global__ __launch_bounds__(256) void k_adam_dense(DensePair pr) {
    constexpr int PIECE = 1024 / G;
    if (blockIdx.y == 2) {                               // optional: the step's K4 rides in this launch
        if (blockIdx.x == 0) finalize_body(pr.f);
        return;
    }
    warm_args(pr.a[blockIdx.y]);                         // (after the y == 2 exit: pr.a has two entries)
    const DenseArgs& a = pr.a[blockIdx.y];
    if (*a.err) return;
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int d0 = gl * VEC;
    const int D = a.D;
    const AdamC c = {a.alpha, a.b1, a.b2, a.eps, 1.f - a.b1, 1.f - a.b2};
    for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < a.rows;
         row += (int64_t)gridDim.x * GPB) {
        const int32_t slot = a.map ? a.map[row] : 0;
        const size_t roff = (size_t)row * D;
        Frag<VEC> w, mrow, vrow;
#pragma unroll
        for (int q = 0; q < VEC; ++q) { w.v[q] = 0.f; mrow.v[q] = 0.f; vrow.v[q] = 0.f; }
        if (!a.frozen_rows) {                            // independent of the map: issue first
            w = load_frag<VEC>(a.w + roff, d0, D);
            if (a.opt == 0) {
                mrow = load_frag<VEC>(a.m + roff, d0, D);
                vrow = load_frag<VEC>(a.v + roff, d0, D);
            }
        }
        float bw = 0.f, mb = 0.f, vb = 0.f;
        if (gl == 0 && !a.frozen_bias) {
            bw = a.bias_w[row];
            if (a.opt == 0) { mb = a.bias_m[row]; vb = a.bias_v[row]; }
        }
        Frag<VEC> gr;
        float gb = 0.f;
        if (a.dense_grad) {                              // dense gradients (whole runs land here directly)
            gr = load_frag<VEC>(a.dense_grad + roff, d0, D);
            gb = a.dense_gbias[row];
            if (slot) {                                  // a run split over several reduce blocks
                gr = run_total<VEC, PIECE>(a.grad_rows, a.grad_bias, a.ks, a.B, (int64_t)slot - 1, (int32_t)row, d0, D, gb);
                if (gl == 0) a.map[row] = 0;
            }
            Frag<VEC> z;
#pragma unroll
            for (int q = 0; q < VEC; ++q) z.v[q] = 0.f;
            store_frag<VEC>(a.dense_grad + roff, d0, D, z);      // consumed: clean for the next step
            if (gl == 0) a.dense_gbias[row] = 0.f;
        } else if (slot) {
            gr = run_total<VEC, PIECE>(a.grad_rows, a.grad_bias, a.ks, a.B, (int64_t)slot - 1, (int32_t)row, d0, D, gb);
            if (gl == 0) a.map[row] = 0;                 // consumed (after the read above)
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) gr.v[q] = 0.f;
        }
        if (!a.frozen_rows) {
            if (a.opt == 0) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) adam_sparse(w.v[q], mrow.v[q], vrow.v[q], gr.v[q], c);
                store_frag<VEC>(a.m + roff, d0, D, mrow);
                store_frag<VEC>(a.v + roff, d0, D, vrow);
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q) w.v[q] = w.v[q] - a.lr * gr.v[q];
            }
            store_frag<VEC>(a.w + roff, d0, D, w);
        }
        if (gl == 0 && !a.frozen_bias) {
            if (a.opt == 0) {
                adam_sparse(bw, mb, vb, gb, c);
                a.bias_m[row] = mb;
                a.bias_v[row] = vb;
            } else {
                bw = bw - a.lr * gb;
            }
            a.bias_w[row] = bw;
        }
    }
}

// ------------------------------------------------------------------------------------
// K5c  small-table sweep over per-tile partials.  With the tile-local sort (k_front) a row's
//      gradient is spread over the <= 16 tiles of the batch: tab[t][row] packs how many entries tile t
//      has for the row (<< 16) and where its run starts in the tile's sorted list; the run's piece
//      sums (k_seg_reduce) sit at that position and at the following multiples of EPB.  One lane
//      group per row adds them in tile order = batch order (all addresses come from the two lookup
//      tables, so the loads are independent) and then either applies the optimiser (TF1 Adam: every
//      row; lazy Adam / SGD: touched rows) or - data parallel - writes the row into the dense
//      gradient buffer.  blockIdx.y == 2 runs the step's finalize (K4).
//
//      Full-width rows (D == G * VEC) with one lane group per row in the grid take dense_tiles_rounds: the same sums in
//      the same order in three load rounds.  Round 1: the NT table entries, the error word, then w, m, v and the bias
//      words; only the entries and the error word are waited for.  Round 2: every head piece and the first two k = 1
//      continuation pieces of the row (their addresses follow from the entries alone), all in flight together.
//      Round 3: the stores.  A row with more than two k = 1 continuations or a deeper one (a run over three pieces)
//      goes through the round-major loop from k = 1 as in the general form.  Absent pieces are loads past the
//      resource's end (zeros, no memory access) and are added as +0.0f: the sums start at +0.0f and never become
//      -0.0f, so that changes no bit.  A row's 4-byte words - entries, bias sums, its three bias words - come in one
//      request per round: one lane per tile (or per word) fetches, and the group hands them round by cross-lane moves.
//
//      What the chain's head needs - this side's table, its bins and rows, the tile count and the error word's address -
//      comes in DenseHead from preloaded SGPRs (k_dense_tiles' leading scalar parameters), so round 1's entries and
//      error word are requested before any line of the struct has arrived; the struct is awaited behind them
//      (warm_args_land), in front of w, m, v, whose addresses it holds.
struct DenseHead { const int32_t* tab; const int32_t* err; int nbins, rows, ntiles; };
template <int G, int VEC, bool WRITE, int NT>
__device__ __forceinline__ void dense_tiles_rounds(const TileDenseLaunch& L, const DenseHead& h, const WarmLines<TileDenseArgs>& warm) {
    const TileDenseArgs& a = L.a[blockIdx.y];
    constexpr int GPB = 256 / G;
    constexpr int EPB = 1024 / G;
    constexpr int D = G * VEC;
    constexpr int NB = (NT > 12) ? 8 : NT;               // NT = 16: the heads in two batches of eight
    const int gl = threadIdx.x % G;
    const int d0 = gl * VEC;
    const int row = (int)blockIdx.x * GPB + threadIdx.x / G;
    if (row >= h.rows) return;                           // a group leaves together: no cross-lane move below reads a lane that is gone
    // The row's 4-byte words travel one request per round: lane tl of each 16-lane row of the group (of the group itself below
    // 16 lanes) fetches what belongs to tile tl, GE + tl, ..., and group_bcast hands each word round.  Slots NT and NT + 1 of
    // that numbering are the two continuation pieces' bias sums.
    constexpr int GE = G < 16 ? G : 16;
    constexpr int NE = (NT + GE - 1) / GE;               // requests for the NT entries
    constexpr int NS = (NT + 2 + GE - 1) / GE;           // requests for the NT + 2 bias sums of round 2
    const int tl = gl % GE;
    const bool first_row = G <= 16 || gl < 16;           // lane 0 adds the bias sums: its row alone fetches them
    // ---- round 1
    const __amdgpu_buffer_rsrc_t rtab =                  // ends with the last tile's table: entries of tiles past it read as 0
        __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(h.tab), 0, h.ntiles * h.nbins * 4, 0x00020000);
    int32_t own[NS];                                     // lane tl's entries: of tiles tl, GE + tl, ... - one request per GE tiles
#pragma unroll
    for (int i = 0; i < NS; ++i) own[i] = i < NE ? (int32_t)buf_load_word(rtab, ((i * GE + tl) * h.nbins + row) * 4) : 0;
    int32_t err = (int32_t)buf_load_word(wt_rsrc(h.err), 0);
    __builtin_amdgcn_sched_barrier(0);
    warm_args_land(warm);                                // the struct's lines: first needed here
    const int roff = (row * D + d0) * 4;
    Frag<VEC> w, mrow, vrow;
    uint32_t b3 = 0;
    if constexpr (!WRITE) {
        const int ow = a.frozen_rows ? BUF_NONE : roff;
        const int om = (a.frozen_rows || a.opt != 0) ? BUF_NONE : roff;
        w = buf_load_frag<VEC>(wt_rsrc(a.w), ow);
        mrow = buf_load_frag<VEC>(wt_rsrc(a.m), om);
        vrow = buf_load_frag<VEC>(wt_rsrc(a.v), om);
        // the three bias words in one request: lanes 0, 1, 2 of the group read bias_w, bias_m, bias_v (every other lane, and
        // every lane where there are no moments, bias_w again: always a valid address, no branch); lane 0 gets them below
        const bool mom = (a.opt == 0) & !a.frozen_bias;  // the moments are read where they are used, as before
        uint64_t pw = (uint64_t)a.bias_w, pm = (uint64_t)a.bias_m, pv = (uint64_t)a.bias_v;
        asm volatile("" : "+s"(pw), "+s"(pm), "+s"(pv));  // the three pointers as values in SGPRs: a select between them is then
        uint64_t bp = pw;                                //   a select, not a load of the struct at a per-lane address
        bp = (mom & (gl % 3 == 1)) ? pm : bp;
        bp = (mom & (gl % 3 == 2)) ? pv : bp;
        typedef const float __attribute__((address_space(1))) gfloat;   // a global load: counted in order with the buffer loads
        b3 = __float_as_uint(reinterpret_cast<gfloat*>(bp)[row]);
    }
    __builtin_amdgcn_sched_barrier(0);                   // everything above is issued before the error word is looked at
    asm volatile("" : "+v"(err) : : "memory");
    if (err) return;                                     // a voided step: the tables' contents are not to be trusted as addresses
    // ---- round 2: addresses from the entries alone
    int32_t ent[NT];
    unrolled<NT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        ent[t] = (int32_t)group_bcast<G, t % GE>((uint32_t)own[t / GE]);
    });
    int s0 = -1, s1 = -1, nk1 = 0;                       // the first two k = 1 continuation pieces (entry index), how many there are
    bool deep = false, touched = false;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int32_t e = ent[t];
        const int off = e & 0xffff;
        const int pp = t * 1024 + (off / EPB + 1) * EPB;
        const int end = t * 1024 + off + (e >> 16);
        const bool has1 = pp < end;
        deep = deep || pp + EPB < end;
        s1 = (has1 && nk1 == 1) ? pp : s1;
        s0 = (has1 && nk1 == 0) ? pp : s0;
        nk1 += has1 ? 1 : 0;
        touched = touched || (e >> 16);
    }
    const __amdgpu_buffer_rsrc_t rg = wt_rsrc(a.grad_rows), rgb = wt_rsrc(a.grad_bias);
    Frag<VEC> tot, c0, c1;
#pragma unroll
    for (int q = 0; q < VEC; ++q) tot.v[q] = 0.f;
    float gb = 0.f;
    uint32_t sb[NS];                                     // slot i * GE + tl's bias sum, in the first row's lanes
#pragma unroll
    for (int t0 = 0; t0 < NT; t0 += NB) {
        Frag<VEC> x[NB];
        if (t0 == 0) {                                   // the 4-byte request(s) first: the piece adds below then wait load by load
#pragma unroll
            for (int i = 0; i < NS; ++i) {               // own[i] is 0 from tile ntiles on, and there is no own entry past NT
                const int slot = i * GE + tl;
                const int32_t e = own[i];
                int at = (e >> 16) ? slot * 1024 + (e & 0xffff) : -1;
                at = slot == NT ? s0 : slot == NT + 1 ? s1 : at;
                sb[i] = buf_load_word(rgb, (at >= 0 && first_row) ? at * 4 : BUF_NONE);
            }
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int32_t e = ent[t0 + t];
            const int j = (t0 + t) * 1024 + (e & 0xffff);
            x[t] = buf_load_frag<VEC>(rg, (e >> 16) ? (j * D + d0) * 4 : BUF_NONE);
        }
        if (t0 == 0) {
            c0 = buf_load_frag<VEC>(rg, s0 >= 0 ? (s0 * D + d0) * 4 : BUF_NONE);
            c1 = buf_load_frag<VEC>(rg, s1 >= 0 ? (s1 * D + d0) * 4 : BUF_NONE);
        }
        __builtin_amdgcn_sched_barrier(0);               // the batch is in flight before its first piece is added
        unrolled<NT>([&](auto tc) {                      // the heads' bias sums in tile order (lane 0's sum is the one used)
            constexpr int t = decltype(tc)::value;
            if (t >= t0 && t < t0 + NB) gb += __uint_as_float(group_bcast<G, t % GE>(sb[t / GE]));
        });
#pragma unroll
        for (int t = 0; t < NB; ++t) {                   // head pieces, added in tile order
#pragma unroll
            for (int q = 0; q < VEC; ++q) tot.v[q] += x[t].v[q];
        }
    }
    if (nk1 <= 2 && !deep) {                             // round k = 1 by tile, and there is no round k = 2
#pragma unroll
        for (int q = 0; q < VEC; ++q) tot.v[q] += c0.v[q];
        gb += __uint_as_float(group_bcast<G, NT % GE>(sb[NT / GE]));
#pragma unroll
        for (int q = 0; q < VEC; ++q) tot.v[q] += c1.v[q];
        gb += __uint_as_float(group_bcast<G, (NT + 1) % GE>(sb[(NT + 1) / GE]));
    } else {                                             // hot rows: round-major, tile-minor from k = 1 (see the general form)
        for (int k = 1;; ++k) {
            bool more = false;
            uint32_t yb[NE];                             // tile i * GE + tl's k-th continuation bias sum
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int32_t e = own[i];
                const int j = (i * GE + tl) * 1024 + (e & 0xffff);
                const int pp = (j / EPB + k) * EPB;
                yb[i] = buf_load_word(rgb, (pp < j + (e >> 16) && first_row) ? pp * 4 : BUF_NONE);
            }
#pragma unroll
            for (int t0 = 0; t0 < NT; t0 += NB) {
                Frag<VEC> y[NB];
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    const int32_t e = ent[t0 + t];
                    const int j = (t0 + t) * 1024 + (e & 0xffff);
                    const int pp = (j / EPB + k) * EPB;
                    const bool has = pp < j + (e >> 16);
                    y[t] = buf_load_frag<VEC>(rg, has ? (pp * D + d0) * 4 : BUF_NONE);
                    more = more || has;
                }
#pragma unroll
                for (int t = 0; t < NB; ++t) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) tot.v[q] += y[t].v[q];
                }
                unrolled<NT>([&](auto tc) {
                    constexpr int t = decltype(tc)::value;
                    if (t >= t0 && t < t0 + NB) gb += __uint_as_float(group_bcast<G, t % GE>(yb[t / GE]));
                });
            }
            if (!more) break;
        }
    }
    // ---- round 3
    const size_t rfl = (size_t)row * D;
    if constexpr (WRITE) {
        if (touched) {
            store_frag<VEC>(a.out_rows + rfl, d0, D, tot);
            if (gl == 0) a.out_bias[row] = gb;
        }
    } else {
        if (!touched && a.skip_untouched) return;
        const AdamC c = {a.alpha, a.b1, a.b2, a.eps, 1.f - a.b1, 1.f - a.b2};
        const int wt = L.wt;
        if (!a.frozen_rows) {
            if (a.opt == 0) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) adam_sparse(w.v[q], mrow.v[q], vrow.v[q], tot.v[q], c);
                store_frag_p<VEC>(a.m, rfl, d0, D, mrow, wt & TFR_WT_MOMENTS);
                store_frag_p<VEC>(a.v, rfl, d0, D, vrow, wt & TFR_WT_MOMENTS);
            } else {                                     // spelled as the general form is compiled (one fused multiply-add per
#pragma unroll                                           // element; the bias below a product and a difference): bit-identical
                for (int q = 0; q < VEC; ++q) w.v[q] = __builtin_fmaf(-a.lr, tot.v[q], w.v[q]);
            }
            store_frag_p<VEC>(a.w, rfl, d0, D, w, wt & TFR_WT_ROWS);
        }
        float bw = __uint_as_float(b3);                  // lane 0's own word; its neighbours' come while the group is whole
        float mb = __uint_as_float(group_bcast<G, 1>(b3)), vb = __uint_as_float(group_bcast<G, 2>(b3));
        if (gl == 0 && !a.frozen_bias) {
            const bool wb = wt & TFR_WT_BIAS;
            if (a.opt == 0) {
                adam_sparse(bw, mb, vb, gb, c);
                store_word_p(a.bias_m, (size_t)row, __float_as_uint(mb), wb);
                store_word_p(a.bias_v, (size_t)row, __float_as_uint(vb), wb);
            } else {
                bw = bw - __fmul_rn(a.lr, gb);
            }
            store_word_p(a.bias_w, (size_t)row, __float_as_uint(bw), wb);
        }
    }
}

template <int G, int VEC, bool WRITE, int NT>
__global__ __launch_bounds__(256, (NT > 12 && VEC == 4 && !WRITE) ? 2 : 3)                // (the register budget)
void k_dense_tiles(const int32_t* tab0, const int32_t* tab1, const int32_t* errp, int nbins0, int nbins1, int rows0, int rows1, int ntiles,
                   int ncols, int flags, TileDenseLaunch L) {
    // The 13 leading dwords are preloaded into user SGPRs: L.a[y].tab / nbins / rows for y = 0, 1, the tile count
    // and error word both sides share, the block columns that hold rows (gridDim.x - 1, which would be a scalar load too) and
    // DENSE_FLAG_* = L.rounds / L.with_fin.  blockIdx.y picks between the two sets by scalar selects.
    const WarmLines<TileDenseArgs> warm = warm_args_issue(L.a[blockIdx.y]);
    if ((int)blockIdx.x == ncols) {                      // the extra block column: K4 (optional), nothing else
        if (blockIdx.y == 0 && (flags & DENSE_FLAG_FIN)) finalize_body(L.f);
        return;
    }
    const bool users = blockIdx.y != 0;
    const DenseHead h = {users ? tab1 : tab0, errp, users ? nbins1 : nbins0, users ? rows1 : rows0, ntiles};
    if constexpr (VEC == 4) {                            // (VEC == 1 rows are never full width: D % 4 != 0 there)
        if (flags & DENSE_FLAG_ROUNDS) {                 // block-uniform: full-width rows, one lane group per row (launch_dense_tiles)
            dense_tiles_rounds<G, VEC, WRITE, NT>(L, h, warm);
            return;
        }
    }
    const TileDenseArgs& a = L.a[blockIdx.y];
    const int32_t err = *h.err;                          // looked at behind the first round of loads (they need no lookup table):
    warm_args_land(warm);                                // its round trip is then not a round of its own - and runs beside the struct's
    constexpr int GPB = 256 / G;
    constexpr int EPB = 1024 / G;
    const int gl = threadIdx.x % G;
    const int d0 = gl * VEC;
    const int D = a.D;
    const AdamC c = {a.alpha, a.b1, a.b2, a.eps, 1.f - a.b1, 1.f - a.b2};
    for (int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G; row < h.rows;
         row += (int64_t)ncols * GPB) {
        const size_t roff = (size_t)row * D;
        Frag<VEC> w, mrow, vrow;
#pragma unroll
        for (int q = 0; q < VEC; ++q) { w.v[q] = 0.f; mrow.v[q] = 0.f; vrow.v[q] = 0.f; }
        float bw = 0.f, mb = 0.f, vb = 0.f;
        if constexpr (!WRITE) {                          // independent of the lookups: issue first
            if (!a.frozen_rows) {
                w = load_frag<VEC>(a.w + roff, d0, D);
                if (a.opt == 0) {
                    mrow = load_frag<VEC>(a.m + roff, d0, D);
                    vrow = load_frag<VEC>(a.v + roff, d0, D);
                }
            }
            if (gl == 0 && !a.frozen_bias) {
                bw = a.bias_w[row];
                if (a.opt == 0) { mb = a.bias_m[row]; vb = a.bias_v[row]; }
            }
        }
        Frag<VEC> tot;
#pragma unroll
        for (int q = 0; q < VEC; ++q) tot.v[q] = 0.f;
        float gb = 0.f;
        bool touched = false;
        // one round trip for all NT table entries, then the piece heads in batches of NB whose
        // addresses are all known up front (NT <= 12: a single batch)
        constexpr int NB = (NT > 12) ? 8 : NT;
        int32_t ent[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) ent[t] = (t < h.ntiles) ? h.tab[(size_t)t * h.nbins + row] : 0;
        if (err) return;                                 // a voided step: the tables' contents are not to be trusted as addresses
#pragma unroll
        for (int t0 = 0; t0 < NT; t0 += NB) {
            Frag<VEC> x[NB];
            float xb[NB];
#pragma unroll
            for (int t = 0; t < NB; ++t) {               // predicated: a dummy address would be one hot L2 line
                const int32_t e = ent[t0 + t];
#pragma unroll
                for (int q = 0; q < VEC; ++q) x[t].v[q] = 0.f;
                xb[t] = 0.f;
                if (e >> 16) {
                    const int64_t j = (int64_t)(t0 + t) * 1024 + (e & 0xffff);
                    x[t] = load_frag<VEC>(a.grad_rows + (size_t)j * D, d0, D);
                    xb[t] = a.grad_bias[j];
                }
            }
#pragma unroll
            for (int t = 0; t < NB; ++t) {               // head pieces, added in tile order
                if (ent[t0 + t] >> 16) {
                    touched = true;
#pragma unroll
                    for (int q = 0; q < VEC; ++q) tot.v[q] += x[t].v[q];
                    gb += xb[t];
                }
            }
        }
        // hot rows: runs cut into several pieces.  Round k adds the k-th continuation piece of every
        // tile (loads of a round are independent), so the chain is as long as the most-split run of
        // one tile, not the sum over tiles.  Fixed order: round-major, tile-minor.
        for (int k = 1;; ++k) {
            bool more = false;
#pragma unroll
            for (int t0 = 0; t0 < NT; t0 += NB) {
                Frag<VEC> y[NB];
                float yb[NB];
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    const int32_t e = ent[t0 + t];
                    const int64_t j = (int64_t)(t0 + t) * 1024 + (e & 0xffff);
                    const int64_t pp = (j / EPB + k) * EPB;
                    const bool has = (e >> 16) && pp < j + (e >> 16);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) y[t].v[q] = 0.f;
                    yb[t] = 0.f;
                    if (has) {
                        y[t] = load_frag<VEC>(a.grad_rows + (size_t)pp * D, d0, D);
                        yb[t] = a.grad_bias[pp];
                        more = true;
                    }
                }
#pragma unroll
                for (int t = 0; t < NB; ++t) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) tot.v[q] += y[t].v[q];
                    gb += yb[t];
                }
            }
            if (!more) break;
        }
        if constexpr (WRITE) {
            if (touched) {
                store_frag<VEC>(a.out_rows + roff, d0, D, tot);
                if (gl == 0) a.out_bias[row] = gb;
            }
        } else {
            if (!touched && a.skip_untouched) continue;
            const int wt = L.wt;                         // write-through: read only by the next launches (TFR_WT)
            if (!a.frozen_rows) {
                if (a.opt == 0) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) adam_sparse(w.v[q], mrow.v[q], vrow.v[q], tot.v[q], c);
                    store_frag_p<VEC>(a.m, roff, d0, D, mrow, wt & TFR_WT_MOMENTS);
                    store_frag_p<VEC>(a.v, roff, d0, D, vrow, wt & TFR_WT_MOMENTS);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) w.v[q] = w.v[q] - a.lr * tot.v[q];
                }
                store_frag_p<VEC>(a.w, roff, d0, D, w, wt & TFR_WT_ROWS);
            }
            if (gl == 0 && !a.frozen_bias) {
                const bool wb = wt & TFR_WT_BIAS;
                if (a.opt == 0) {
                    adam_sparse(bw, mb, vb, gb, c);
                    store_word_p(a.bias_m, (size_t)row, __float_as_uint(mb), wb);
                    store_word_p(a.bias_v, (size_t)row, __float_as_uint(vb), wb);
                } else {
                    bw = bw - a.lr * gb;
                }
                store_word_p(a.bias_w, (size_t)row, __float_as_uint(bw), wb);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_finalize(FinArgs a) { warm_args(a); finalize_body(a); }

// ------------------------------------------------------------------------------------
// AUC on the device (svd_train_val.py:97,173: sklearn's roc_auc_score(rates, sigmoid(logits)) per batch is the host
// bottleneck SURVEY 8f #1 names).  AUC = (sum of the positives' mid-ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg)
// (Mann-Whitney; equal scores share the mean of their ranks, which is what the ROC trapezoids give).  Scores are
// mapped to 32-bit keys in score order, sorted by the library's radix sort, and every positive finds how many keys
// are smaller / not larger than its own by two binary searches of the sorted keys; twice the mid-rank is the
// integer lo + hi + 1, so the rank sum is exact integer arithmetic (64-bit integer adds: order-independent).
__global__ __launch_bounds__(256) void k_auc_keys(const float* __restrict__ score, int32_t* __restrict__ keys, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        float x = score[k];
        if (x == 0.f) x = 0.f;                           // -0 and +0 are equal scores
        const uint32_t b = __float_as_uint(x);
        keys[k] = (int32_t)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
    }
}

__global__ __launch_bounds__(256) void k_auc_ranksum(const int32_t* __restrict__ ks, const int32_t* __restrict__ ps,
                                                     const float* __restrict__ label, int64_t n, unsigned long long* out /* {2 x rank sum, n_pos} */) {
    unsigned long long s2 = 0, np = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        if (label[ps[j]] > 0.5f) {
            const uint32_t key = (uint32_t)ks[j];
            int64_t lo = 0, hi = n;                      // first index with a key >= mine
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((uint32_t)ks[mid] < key) lo = mid + 1; else hi = mid; }
            const int64_t first = lo;
            hi = n;                                      // first index with a key > mine
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((uint32_t)ks[mid] <= key) lo = mid + 1; else hi = mid; }
            s2 += (unsigned long long)(first + lo + 1);  // 1-based ranks first+1 .. lo: twice their mean
            np += 1;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) { s2 += __shfl_down(s2, o, 64); np += __shfl_down(np, o, 64); }
    if ((threadIdx.x & 63) == 0 && np) { atomicAdd(&out[0], s2); atomicAdd(&out[1], np); }
}

void launch_auc_keys(const float* score, int32_t* keys, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_auc_keys, dim3(blocks_for(n, 256, 2048)), dim3(256), 0, s, score, keys, n);
}
void launch_auc_ranksum(const int32_t* ks, const int32_t* ps, const float* label, int64_t n, unsigned long long* out, hipStream_t s) {
    hipLaunchKernelGGL(k_auc_ranksum, dim3(blocks_for(n, 256, 2048)), dim3(256), 0, s, ks, ps, label, n, out);
}

// ------------------------------------------------------------------------------------
// Variable initialisers (ops.py:8-12,29-32): truncated normal = N(0, s) resampled until
// |x| <= 2 s [TF1-lib].  Counter-based (splitmix64 of seed and element index), so the
// values do not depend on the launch geometry.  TF's Philox stream is not reproducible
// here: initial values are not a parity target.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void k_init_trunc_normal(float* p, int64_t n, float stddev, uint64_t seed) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
         k += (int64_t)gridDim.x * blockDim.x) {
        float z = 0.f;
        for (int attempt = 0; attempt < 16; ++attempt) {
            const uint64_t h = splitmix64(seed ^ splitmix64((uint64_t)k * 16 + attempt));
            const float u1 = ((float)(uint32_t)(h >> 40) + 0.5f) * (1.f / 16777216.f);   // (0,1)
            const float u2 = ((float)(uint32_t)((h >> 16) & 0xFFFFFF) + 0.5f) * (1.f / 16777216.f);
            z = sqrtf(-2.f * __logf(u1)) * __cosf(6.28318530718f * u2);
            if (fabsf(z) <= 2.f) break;
            z = 0.f;
        }
        p[k] = z * stddev;
    }
}

__global__ void k_init_uniform_scalar(float* p, float lo, float hi, uint64_t seed) {
    const uint64_t h = splitmix64(seed ^ 0xABCDEF12345ull);
    const float u = ((float)(uint32_t)(h >> 40) + 0.5f) * (1.f / 16777216.f);
    p[0] = lo + (hi - lo) * u;
}

// ------------------------------------------------------------------------------------
// launch helpers
template <int MODE, int UNR>
static void launch_forward_mode(const FwdArgs& a, int G, int VEC, int grid, hipStream_t s) {
    with_geometry(G, VEC, [&](auto g, auto v) {
        with_bool(forward_pnt(MODE, a.U, a.D), [&](auto pnt) {
            hipLaunchKernelGGL((k_forward<g.value, v.value, MODE, UNR, pnt.value>), dim3(grid), dim3(256), 0, s, a);
        });
    });
}

int forward_grid(int64_t B, int G, int mode, int unr) {
    // waves * SPW * UNR ratings per block; TRAIN/EVAL: fewer partials for K4; then grid-stride
    return blocks_for(B, 4 * (64 / G) * unr, (mode == MODE_INFER) ? 8192 : 2048);
}

int front_forward_blocks(int64_t B, int G) {
    return blocks_for(B, 16 * (64 / G) * 2, 512);        // waves * SPW * UNR of k_front's forward part
}

void launch_front(const FrontArgs& fa, int G, int VEC, hipStream_t s) {
    const int nbmax = fa.c.nbins[0] > fa.c.nbins[1] ? fa.c.nbins[0] : fa.c.nbins[1];
    const dim3 grid(fa.nfwd + 2 * fa.c.ntiles);
    with_geometry(G, VEC, [&](auto g, auto v) {
        static bool attr = false;                        // one per instantiation
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_front<g.value, v.value>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, CSORT_MAX_BINS * 4);
            attr = true;
        }
        hipLaunchKernelGGL((k_front<g.value, v.value>), grid, dim3(1024), (size_t)nbmax * 4, s, fa);
    });
}

int tile_step_epg(int ntiles, int G, int VEC) {
    // smallest EPG in {1, 2, 4} that brings the grid (two sides) down to one block per CU (256 CUs), as far
    // as LDS allows: the wave-level ping-pong buffers (2 * EPG * 16 * G * VEC floats) share the 64 KB dynamic
    // region with the sort's bins; static arrays take another ~40 KB of the CU's 160 KB
    auto fits = [&](int e) {
        return (size_t)2 * e * 16 * G * VEC * 4 <= (size_t)64 * 1024 && tile_step_static_lds(G, e) + (size_t)64 * 1024 <= LDS_PER_CU;
    };
    static const int forced = (int)env_int("TFR_EPG", 0);   // TFR_EPG=1|2|4: A/B override
    if (forced == 1 || ((forced == 2 || forced == 4) && forced <= G && fits(forced))) return forced;
    int epg = 1;
    while (epg < 4 && epg < G && ntiles * (G / epg) * 2 > 256 && fits(2 * epg)) epg *= 2;
    return epg;
}

// the item side's pieces per block: half the user side's where the grid - look-ahead sort blocks, the user side's
// blocks and the item side's, each side cut to the blocks that hold entries - still fits one block per CU (256 CUs).
// At the headline shape (B = 10000, G = 16, 20 sort blocks) that is 20 + 79 + 157 = 256 blocks.  Measured no faster
// than one EPG for both sides: off unless TFR_ITEM_SPLIT=1 (A/B).
int tile_step_item_epg(int64_t B, int G, int VEC, int nsort) {
    const int epg = tile_step_epg((int)((B + 1023) / 1024), G, VEC);
    static const bool split = env_default_off("TFR_ITEM_SPLIT");
    if (!split || epg < 2) return epg;
    const int64_t epb = 1024 / G;
    const int64_t nu = (B + epb * epg - 1) / (epb * epg), ni = (B + epb * (epg / 2) - 1) / (epb * (epg / 2));
    return nsort + nu + ni <= 256 ? epg / 2 : epg;
}
int tile_step_one_barrier() {                            // TFR_ONE_BARRIER=1: A/B switch, measured slower
    static const bool on = env_default_off("TFR_ONE_BARRIER");
    return on;
}
int tile_step_wt() {                                     // TFR_WT=<bits>: A/B switch (TFR_WT_* in svd_kernels.h)
    static_assert((TFR_WT_DEFAULT & 31) == TFR_WT_DEFAULT, "five bits");
    static const int wt = (int)env_int("TFR_WT", TFR_WT_DEFAULT) & 31;
    return wt;
}

void launch_tile_step(const TileStepArgs& a0, int G, int VEC, hipStream_t s) {
    const int nbmax = a0.nbins[0] > a0.nbins[1] ? a0.nbins[0] : a0.nbins[1];
    const int epg = tile_step_epg(a0.ntiles, G, VEC);
    size_t dyn = (size_t)nbmax * 4;                       // bins during the sort, contributions afterwards
    if (dyn < (size_t)2 * epg * 16 * G * VEC * 4) dyn = (size_t)2 * epg * 16 * G * VEC * 4;   // wave-level ping-pong buffers of the reduce
    if (tile_step_static_lds(G, epg) + dyn > LDS_PER_CU) return;  // cannot happen for a shape tile_step_epg() admits (tests/test_lds_budget.py)
    const int nsort = a0.next_ids ? 2 * a0.next_ntiles : 0;       // look-ahead sort blocks come first
    TileStepArgs a = a0;
    a.epg_item = tile_step_item_epg(a.B, G, VEC, nsort);  // <= epg: the LDS above covers it
    a.one_barrier = tile_step_one_barrier();
    a.wt = tile_step_wt();
    const int64_t epb = 1024 / G;
    const int nblk_u = (int)((a.B + epb * epg - 1) / (epb * epg)), nblk_i = (int)((a.B + epb * a.epg_item - 1) / (epb * a.epg_item));
    const dim3 grid(nsort + nblk_u + nblk_i);
    with_geometry(G, VEC, [&](auto g, auto v) {
        with_one_of<1, 2, 4>(epg, [&](auto e) {
            static size_t attr = 0;                      // one per instantiation; static + dynamic LDS must stay within 160 KB: ask for what is needed
            if (dyn > attr) {
                if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_tile_step<g.value, v.value, e.value>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess)
                    return;                              // no launch: leaves the error for the caller's hipGetLastError()
                attr = dyn;
            }
            // the first round's operands lead as scalars (preloaded SGPRs); the struct keeps its copies for everything later
            hipLaunchKernelGGL((k_tile_step<g.value, v.value, e.value>), grid, dim3(1024), dyn, s, a.srt[0], a.srt[1], a.next_recs, (int)a.B, nsort,
                               nblk_u, a.epg_item, a.ntiles, a.next_ntiles, (int)a.next_B, a.dbg ? 1 : 0, a);
        });
    });
}

void launch_forward(const FwdArgs& a, int mode, int G, int VEC, int grid, hipStream_t s) {
    if (mode == MODE_INFER) launch_forward_mode<MODE_INFER, 4>(a, G, VEC, grid, s);
    else if (mode == MODE_TRAIN) launch_forward_mode<MODE_TRAIN, 4>(a, G, VEC, grid, s);
    else launch_forward_mode<MODE_EVAL, 4>(a, G, VEC, grid, s);
}

static int entry_grid(int64_t B, int G) { return blocks_for(B, 256 / G); }

template <typename F, size_t... K>
static bool with_red_pick(const RedPick& p, F&& f, std::index_sequence<K...>) {
    return (... || ((p.rmode == RED_PICKS[K].rmode && p.fwd == RED_PICKS[K].fwd && p.lean == RED_PICKS[K].lean && p.fast == RED_PICKS[K].fast)
                        ? (f(int_c<RED_PICKS[K].rmode>{}, bool_c<RED_PICKS[K].fwd>{}, bool_c<RED_PICKS[K].lean>{}, bool_c<RED_PICKS[K].fast>{}), true)
                        : false));
}

void launch_seg_reduce(const RedPair& p, int n, int rmode, int G, int VEC, hipStream_t s, bool fwd) {
    int64_t B = p.a[0].B;
    if (n > 1 && p.a[1].B > B) B = p.a[1].B;
    const dim3 grid(blocks_for(B, 1024 / G), n);
    const RedPick pick = seg_reduce_pick(p.a[0], n, rmode, fwd, G, VEC);
    with_geometry(G, VEC, [&](auto g, auto v) {
        with_red_pick(pick, [&](auto rm, auto fw, auto lean, auto fast) {
            hipLaunchKernelGGL((k_seg_reduce<g.value, v.value, rm.value, fw.value, lean.value, fast.value>), grid, dim3(1024), 0, s, p);
        }, std::make_index_sequence<sizeof(RED_PICKS) / sizeof(RED_PICKS[0])>{});
    });
}

void launch_apply_rows(const ApplyPair& p, int n, int opt, int G, int VEC, hipStream_t s) {
    int64_t B = p.a[0].B;
    if (n > 1 && p.a[1].B > B) B = p.a[1].B;
    bool all_split = p.a[0].only_split != 0;
    if (n > 1 && !p.a[1].only_split) all_split = false;
    if (all_split) B = (B + 1024 / G - 1) / (1024 / G);      // one lane group per piece boundary
    const dim3 grid(entry_grid(B, G) + (p.with_fin ? 1 : 0), n);
    with_geometry(G, VEC, [&](auto g, auto v) {
        with_one_of<0, 1, 2>(opt == 0 || opt == 1 ? opt : 2, [&](auto o) {
            hipLaunchKernelGGL((k_apply_rows<g.value, v.value, o.value>), grid, dim3(256), 0, s, p);
        });
    });
}

int sweep_rounds() {                                     // TFR_SWEEP_ROUNDS=0: A/B switch, the general form of k_dense_tiles everywhere
    static const bool on = env_default_on("TFR_SWEEP_ROUNDS");
    return on;
}

int dense_tiles_grid(int64_t rows, int G) {              // block columns that hold rows (the launch adds one for K4)
    return blocks_for(rows, 256 / G, 4096);
}

// the three-round form has no row loop and no width guards: full-width rows, one lane group per row in the grid
bool dense_tiles_rounds_taken(int64_t rows, int D, int G, int VEC) {
    return sweep_rounds() && VEC == 4 && D == G * VEC && rows <= (int64_t)dense_tiles_grid(rows, G) * (256 / G);
}

// f(the k_dense_tiles instantiation for this geometry, mode and tile count): the launcher and dense_tiles_kernel pick by this
template <typename F>
static bool with_dense_tiles(bool write, int G, int VEC, int ntiles, F&& f) {
    return with_geometry(G, VEC, [&](auto g, auto v) {
        with_bool(write, [&](auto wr) {
            with_one_of<4, 8, 10, 12, 16>(dense_tiles_nt(ntiles), [&](auto nt) { f(k_dense_tiles<g.value, v.value, wr.value, nt.value>); });
        });
    });
}

const void* dense_tiles_kernel(bool write, int G, int VEC, int ntiles) {
    const void* k = nullptr;
    with_dense_tiles(write, G, VEC, ntiles, [&](auto* kernel) { k = reinterpret_cast<const void*>(kernel); });
    return k;
}

void launch_dense_tiles(const TileDenseLaunch& L, bool write, bool with_fin, int G, int VEC, hipStream_t s) {
    const int64_t rows = L.a[0].rows > L.a[1].rows ? L.a[0].rows : L.a[1].rows;
    const dim3 grid(dense_tiles_grid(rows, G) + 1, 2);   // + one block column for K4
    TileDenseLaunch LL = L;
    LL.with_fin = with_fin ? 1 : 0;
    LL.wt = tile_step_wt() & (TFR_WT_ROWS | TFR_WT_MOMENTS | TFR_WT_BIAS);
    LL.rounds = (L.a[0].D == L.a[1].D && dense_tiles_rounds_taken(rows, L.a[0].D, G, VEC)) ? 1 : 0;
    // the chain's head as leading scalars (preloaded SGPRs); both sides share the tile count and the error word (api.hip tile_dense)
    const TileDenseArgs &i = LL.a[0], &u = LL.a[1];
    if (i.err != u.err || i.ntiles != u.ntiles || rows > INT32_MAX) return;   // cannot happen for a launch tile_dense builds: no launch
    const int flags = (LL.rounds ? DENSE_FLAG_ROUNDS : 0) | (LL.with_fin ? DENSE_FLAG_FIN : 0);
    with_dense_tiles(write, G, VEC, i.ntiles, [&](auto* kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, i.tab, u.tab, i.err, i.nbins, u.nbins, (int)i.rows, (int)u.rows, i.ntiles, (int)grid.x - 1,
                           flags, LL);
    });
}

void launch_adam_dense(DensePair& p, int n, int G, int VEC, hipStream_t s, const FinArgs* fin) {
    if (fin) { p.f = *fin; n = 3; }
    int64_t rows = p.a[0].rows;
    if (n > 1 && p.a[1].rows > rows) rows = p.a[1].rows;
    const dim3 grid(blocks_for(rows, 256 / G, 4096), n);
    with_geometry(G, VEC, [&](auto g, auto v) { hipLaunchKernelGGL((k_adam_dense<g.value, v.value>), grid, dim3(256), 0, s, p); });
}

static int flat_grid(int64_t n) { return blocks_for(n, 256, 2048); }

void launch_gather_rows(const GatherRowsArgs& a, int G, int VEC, hipStream_t s) {
    const dim3 grid(blocks_for(a.n, 256 / G, 8192));
    with_geometry(G, VEC, [&](auto g, auto v) { hipLaunchKernelGGL((k_gather_rows<g.value, v.value>), grid, dim3(256), 0, s, a); });
}

void launch_gather(const GatherArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_triples, dim3(flat_grid(a.B)), dim3(256), 0, s, a);
}

void launch_pack_triples(const int32_t* u, const int32_t* it, const float* r, void* store, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_triples, dim3(flat_grid(n)), dim3(256), 0, s, u, it, r, reinterpret_cast<int4*>(store), n);
}

void launch_init_trunc_normal(float* p, int64_t n, float stddev, uint64_t seed, hipStream_t s) {
    hipLaunchKernelGGL(k_init_trunc_normal, dim3(flat_grid(n)), dim3(256), 0, s, p, n, stddev, seed);
}

void launch_init_uniform_scalar(float* p, float lo, float hi, uint64_t seed, hipStream_t s) {
    hipLaunchKernelGGL(k_init_uniform_scalar, dim3(1), dim3(1), 0, s, p, lo, hi, seed);
}

// the store records of a run of drawn ids, left beside the ids (api.hip RecBuf; runs on the stream that drew them)
__global__ __launch_bounds__(256) void k_gather_recs(const int64_t* __restrict__ ids, const int4* __restrict__ store, int4* __restrict__ recs,
                                                     int64_t n, int64_t N) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t id = ids[k];
        if ((uint64_t)id >= (uint64_t)N) id = 0;         // (drawn ids are in range by construction)
        recs[k] = store[id];
    }
}

void launch_gather_recs(const int64_t* ids, const void* store, void* recs, int64_t n, int64_t N, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_recs, dim3(blocks_for(n, 256, 1024)), dim3(256), 0, s, ids, reinterpret_cast<const int4*>(store), reinterpret_cast<int4*>(recs), n, N);
}

// two-table form of the big-table step: bring every row that currently lives in the alternate table back to the main
// one (one wave per row; run before anything but the fused step looks at the item table)
__global__ __launch_bounds__(256) void k_settle_alt(float* __restrict__ main_t, const float* __restrict__ alt_t,
                                                    int32_t* __restrict__ sel, int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        if (!sel[r]) continue;                            // wave-uniform
        for (int d = lane; d < D; d += 64) main_t[(size_t)r * D + d] = alt_t[(size_t)r * D + d];
        if (lane == 0) sel[r] = 0;
    }
}

void launch_settle_alt(float* main_t, const float* alt_t, int32_t* sel, int64_t rows, int D, hipStream_t s) {
    hipLaunchKernelGGL(k_settle_alt, dim3(blocks_for(rows, 4, 16384)), dim3(256), 0, s, main_t, alt_t, sel, rows, D);
}

void launch_finalize(const FinArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), 0, s, a);
}

}  // namespace tfr
