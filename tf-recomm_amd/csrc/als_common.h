// als_common.h - what the two Cholesky ALS solvers share (als_kernels.hip: explicit ALS, d <= 32; ials.hip: implicit ALS,
// d <= 64): the one-wave Cholesky solve of a d x d SPD system held in LDS, the chunk tables for long lists with the kernel
// argument that carries them, and the bookkeeping of a thread's slots of the normal equations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "devbuf.h"

namespace tfr {

// Cholesky A = L L^T (in place, lower triangle) and the two triangular solves, by ONE wave: lane r owns row r, a column
// step is j LDS reads of row j (broadcast) and of the lane's own row - no block barrier (a wave's LDS accesses are made
// in program order; volatile keeps the compiler from moving a read of another lane's element over the write it follows).
// The block-wide version (thread 0 alone on the diagonal and in the substitutions, a barrier pair per column) cost
// ~50 us per entity, most of the sweep.  Same operations in the same order per element.
// Called by the 64 threads tid < 64 of a block, all of them; d <= 64; LD is the LDS row stride of A in doubles.
template <int LD>
__device__ __forceinline__ void chol_wave_solve(double (*A)[LD], const double* bvec, double* xvec, int d) {
    const int r = threadIdx.x;
    volatile double (*L)[LD] = A;
    for (int j = 0; j < d; ++j) {
        double s = 0.0;
        if (r >= j && r < d) {
            s = L[r][j];
            for (int k = 0; k < j; ++k) s -= L[r][k] * L[j][k];
        }
        const double piv = sqrt(__shfl(s, j, 64));
        if (r == j) L[j][j] = piv;
        else if (r > j && r < d) L[r][j] = s / piv;
    }
    // L y = b, column by column: lane i finishes y_i, the lanes below take it off their right-hand sides
    double y = (r < d) ? bvec[r] : 0.0;
    for (int i = 0; i < d; ++i) {
        const double yi = __shfl(y / ((r == i) ? L[i][i] : 1.0), i, 64);
        if (r == i) y = yi;
        else if (r > i && r < d) y -= L[r][i] * yi;
    }
    // L^T x = y, from the last column up: column i of L^T is row i of L
    for (int i = d - 1; i >= 0; --i) {
        const double xi = __shfl(y / ((r == i) ? L[i][i] : 1.0), i, 64);
        if (r == i) y = xi;
        else if (r < i) y -= L[i][r] * xi;
    }
    if (r < d) xvec[r] = y;
}

// Long lists (a blockbuster item can hold a few per cent of all pairs) would leave one block working long after the
// rest of the half-sweep has finished: a list of more than CH entries is cut into chunks of CH, whose partial sums other
// blocks build first and the entity's block adds in list order.  cfirst[entity] = its first chunk or -1, ccount[entity]
// chunks; chunk c covers [lo[c], hi[c]) of entity ent[c].
struct ChunkPlan {
    std::vector<int32_t> cfirst, ccount, ent;
    std::vector<int64_t> lo, hi;
};

inline ChunkPlan plan_chunks(const std::vector<int64_t>& ptr, int64_t rows, int64_t CH) {
    ChunkPlan p;
    p.cfirst.assign((size_t)rows, -1);
    p.ccount.assign((size_t)rows, 0);
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t lo = ptr[(size_t)r], hi = ptr[(size_t)r + 1];
        if (hi - lo <= CH) continue;
        p.cfirst[(size_t)r] = (int32_t)p.ent.size();
        for (int64_t s0 = lo; s0 < hi; s0 += CH) {
            p.ent.push_back((int32_t)r); p.lo.push_back(s0); p.hi.push_back(std::min(hi, s0 + CH));
            p.ccount[(size_t)r]++;
        }
    }
    return p;
}

// what a kernel sees of one side's chunk tables, and where the chunks' partial sums go
struct ChunkArgs {
    const int32_t* cfirst; const int32_t* ccount;                  // per entity
    const int32_t* ent; const int64_t* lo; const int64_t* hi;      // per chunk
    int64_t n;                                                     // chunks
    double* partial;                                               // [n][d*d + d]: a chunk's A entries, then its b
};

// one side's chunk tables on the device
struct DevChunks {
    DevBuf<int32_t> cfirst, ccount, ent;
    DevBuf<int64_t> lo, hi;
    int64_t n = 0;

    ChunkArgs args(double* partial) const { return ChunkArgs{cfirst.get(), ccount.get(), ent.get(), lo.get(), hi.get(), n, partial}; }

    hipError_t upload(const ChunkPlan& p, int64_t rows, hipStream_t s) {
        n = 0;
        hipError_t e = cfirst.reserve(rows, s);
        if (e == hipSuccess) e = ccount.reserve(rows, s);
        if (e == hipSuccess) e = hipMemcpy(cfirst, p.cfirst.data(), (size_t)rows * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(ccount, p.ccount.data(), (size_t)rows * 4, hipMemcpyHostToDevice);
        const size_t nc = p.ent.size();
        if (nc) {
            if (e == hipSuccess) e = ent.reserve((int64_t)nc, s);
            if (e == hipSuccess) e = lo.reserve((int64_t)nc, s);
            if (e == hipSuccess) e = hi.reserve((int64_t)nc, s);
            if (e == hipSuccess) e = hipMemcpy(ent, p.ent.data(), nc * 4, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(lo, p.lo.data(), nc * 8, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(hi, p.hi.data(), nc * 8, hipMemcpyHostToDevice);
        }
        if (e == hipSuccess) n = (int64_t)nc;
        return e;
    }
};

// A 256-thread block keeps the normal equations of one entity in registers: thread tid the A entries t = tid + 256 q,
// q < SLOTS (row t / d, column t % d), and thread tid < d the b entry tid.  SLOTS = 4 serves d <= 32, 16 serves d <= 64.
template <int SLOTS>
__device__ __forceinline__ void zero_slots(double (&acc)[SLOTS], double& accb) {
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) acc[q] = 0.0;
    accb = 0.0;
}

// a long list: adds the partial sums of entity e's nch = ccount[e] > 0 chunks, in list order
template <int SLOTS>
__device__ __forceinline__ void add_chunk_partials(const ChunkArgs& ch, int64_t e, int32_t nch, int d, double (&acc)[SLOTS], double& accb) {
    const int tid = threadIdx.x, dd = d * d;
    const int32_t c0 = ch.cfirst[e];
    for (int32_t k = 0; k < nch; ++k) {
        const double* pp = ch.partial + (size_t)(c0 + k) * (dd + d);
#pragma unroll
        for (int q = 0; q < SLOTS; ++q) { const int t = tid + 256 * q; if (t < dd) acc[q] += pp[t]; }
        if (tid < d) accb += pp[dd + tid];
    }
}

template <int SLOTS>
__device__ __forceinline__ void store_chunk_partial(const ChunkArgs& ch, int64_t c, int d, const double (&acc)[SLOTS], double accb) {
    const int tid = threadIdx.x, dd = d * d;
    double* pp = ch.partial + (size_t)c * (dd + d);
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) { const int t = tid + 256 * q; if (t < dd) pp[t] = acc[q]; }
    if (tid < d) pp[dd + tid] = accb;
}

// A[r][c] = entry(t, acc[q], r == c) for every slot t = r d + c: the caller adds its diagonal term (and whatever else
// belongs to entry t) to the sum it is handed
template <int SLOTS, int LD, class Entry>
__device__ __forceinline__ void slots_to_matrix(const double (&acc)[SLOTS], int d, double (*A)[LD], Entry entry) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
        const int t = tid + 256 * q;
        if (t < d * d) {
            const int r = t / d, c = t % d;
            A[r][c] = entry(t, acc[q], r == c);
        }
    }
}

}  // namespace tfr
