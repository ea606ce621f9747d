// arg_preload.hip - does gfx950's kernel-argument preload (the first dwords of the argument block placed in user SGPRs by the
// command processor) shorten the head of a latency-bound kernel?  Both launches of the headline step begin: argument block
// (one cold scalar trip, merged by warm_args) -> first vector load -> dependent vector load.  Here the same head is built twice
// in one binary: arguments in one by-value struct with warm_args (what every kernel of the library takes; a struct first is
// never preloaded), and the first round's operands as leading scalar parameters with the struct behind them (preloaded).
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 -o arg_preload arg_preload.hip && ./arg_preload
// 200 pairs of dependent launches on one stream, ~180 x 1024 threads then ~760 x 256 (the headline's k_tile_step and
// k_dense_tiles geometry); each kernel reads 16 bytes per thread from the buffer its predecessor stored write-through, reads a
// second record at an index taken from the first, and stores.  Reported: us per pair for both forms, alternating three times,
// and from s_memrealtime stamps (100 MHz; a diagnostic instantiation, the timed one has none) the time from a workgroup's
// first instruction to the arrival of its first vector load.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

typedef unsigned long long u64;
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

struct ProbeArgs {                                       // six 64-byte lines, as TileStepArgs; the head's operands lie in the second
    const float* tables[12];
    const int4* src[2]; int4* dst[2];
    const float* more[16];
    int32_t mask, nblk_u, bias, pad;
    u64* stamps;                                         // [grid][2]: first instruction, first load in hand
    long long tail[7];
};
static_assert(sizeof(ProbeArgs) > 320 && sizeof(ProbeArgs) <= 384, "six lines");

// svd_kernels.h's warm_args in two halves: every line of the block in flight at once (issue), and the point where they must
// have landed (land).  The struct form lands them at once, as the library does; the preloaded form after its first vector load.
constexpr int NL = (int)((sizeof(ProbeArgs) + 63) / 64);
struct Warm { int32_t w[NL]; };
__device__ __forceinline__ Warm warm_issue(const ProbeArgs& args) {
    const char* base = reinterpret_cast<const char*>(&args);
    Warm x;
#pragma unroll
    for (int k = 0; k < NL; ++k) x.w[k] = *reinterpret_cast<const int32_t*>(base + (k * 64 < (int)sizeof(ProbeArgs) - 4 ? k * 64 : (int)sizeof(ProbeArgs) - 4));
    return x;
}
__device__ __forceinline__ void warm_land(const Warm& x) {
#pragma unroll
    for (int k = 0; k < NL; ++k) asm volatile("" :: "s"(x.w[k]));
}

// the head both forms share: s0/s1/d0/d1/mask/nblk_u are the first round's operands, `a` is touched only after the loads
template <int THREADS, bool STAMP>
__device__ __forceinline__ void head(const int4* s0, const int4* s1, int4* d0, int4* d1, int mask, int nblk_u, const ProbeArgs& a, u64 t0,
                                     const Warm& warm) {
    const bool side = (int)blockIdx.x >= nblk_u;
    const int4* s = side ? s1 : s0;
    int4* d = side ? d1 : d0;
    const int idx = (int)(blockIdx.x * THREADS + threadIdx.x) & mask;       // mask = entries - 1: every index is in range
    int4 r = s[idx];
    asm volatile("" : "+v"(r.x));                        // the load is issued here ...
    __builtin_amdgcn_sched_barrier(0);
    warm_land(warm);                                     // ... in front of the wait for the struct's lines
    u64 t1 = 0;
    if constexpr (STAMP) asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1) : "v"(r.x) : "memory");
    const int4 r2 = s[(r.x ^ idx) & mask];
    uintx4 o; o.x = (unsigned)(r2.x + r.y + a.bias); o.y = (unsigned)r2.y; o.z = (unsigned)r.z; o.w = (unsigned)idx;
    __builtin_amdgcn_raw_buffer_store_b128(o, __builtin_amdgcn_make_buffer_rsrc(d, 0, 0x7fffffff, 0x00020000), idx * 16, 0, 16);   // sc1
    if constexpr (STAMP) if (threadIdx.x == 0) { a.stamps[2 * blockIdx.x] = t0; a.stamps[2 * blockIdx.x + 1] = t1; }
}

template <int THREADS, bool STAMP>
__global__ __launch_bounds__(THREADS) void k_struct(ProbeArgs a) {
    u64 t0 = 0;
    if constexpr (STAMP) t0 = __builtin_amdgcn_s_memrealtime();
    const Warm warm = warm_issue(a);
    warm_land(warm);
    head<THREADS, STAMP>(a.src[0], a.src[1], a.dst[0], a.dst[1], a.mask, a.nblk_u, a, t0, warm);
}
template <int THREADS, bool STAMP>
__global__ __launch_bounds__(THREADS) void k_preload(const int4* s0, const int4* s1, int4* d0, int4* d1, int mask, int nblk_u, ProbeArgs a) {
    u64 t0 = 0;
    if constexpr (STAMP) t0 = __builtin_amdgcn_s_memrealtime();
    const Warm warm = warm_issue(a);                     // its trip runs beside the record loads
    head<THREADS, STAMP>(s0, s1, d0, d1, mask, nblk_u, a, t0, warm);
}

int main() {
    const int N = 1 << 18, NA = 180, NB = 760, pairs = 200;      // 180 * 1024 and 760 * 256 threads < N entries of 16 bytes
    int4* buf[2]; u64* stamps;
    for (int k = 0; k < 2; ++k) CHK(hipMalloc(&buf[k], (size_t)N * 16));
    CHK(hipMalloc(&stamps, (size_t)2 * (NA + NB) * 8)); CHK(hipMemset(stamps, 0, (size_t)2 * (NA + NB) * 8));
    { std::vector<int> h((size_t)N * 4); unsigned x = 12345u; for (auto& v : h) { x = x * 1664525u + 1013904223u; v = (int)(x >> 8); }
      for (int k = 0; k < 2; ++k) CHK(hipMemcpy(buf[k], h.data(), (size_t)N * 16, hipMemcpyHostToDevice)); }
    hipStream_t s; CHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    // kernel A reads buf[0] and writes buf[1], kernel B the reverse; each side of a launch takes one half of the entries' range
    ProbeArgs aA = {}, aB = {};
    aA.src[0] = buf[0]; aA.src[1] = buf[0]; aA.dst[0] = buf[1]; aA.dst[1] = buf[1]; aA.mask = N - 1; aA.nblk_u = NA / 2; aA.bias = 1;
    aB = aA; aB.src[0] = buf[1]; aB.src[1] = buf[1]; aB.dst[0] = buf[0]; aB.dst[1] = buf[0]; aB.nblk_u = NB / 2;
    aA.stamps = stamps; aB.stamps = stamps + 2 * NA;

    auto chain = [&](bool pre, bool stamp, int n) {
        for (int k = 0; k < n; ++k) {
            if (!pre && !stamp) { k_struct<1024, false><<<NA, 1024, 0, s>>>(aA); k_struct<256, false><<<NB, 256, 0, s>>>(aB); }
            if (!pre && stamp)  { k_struct<1024, true><<<NA, 1024, 0, s>>>(aA);  k_struct<256, true><<<NB, 256, 0, s>>>(aB); }
            if (pre && !stamp)  { k_preload<1024, false><<<NA, 1024, 0, s>>>(aA.src[0], aA.src[1], aA.dst[0], aA.dst[1], aA.mask, aA.nblk_u, aA);
                                  k_preload<256, false><<<NB, 256, 0, s>>>(aB.src[0], aB.src[1], aB.dst[0], aB.dst[1], aB.mask, aB.nblk_u, aB); }
            if (pre && stamp)   { k_preload<1024, true><<<NA, 1024, 0, s>>>(aA.src[0], aA.src[1], aA.dst[0], aA.dst[1], aA.mask, aA.nblk_u, aA);
                                  k_preload<256, true><<<NB, 256, 0, s>>>(aB.src[0], aB.src[1], aB.dst[0], aB.dst[1], aB.mask, aB.nblk_u, aB); }
        }
    };
    for (int pre = 0; pre < 2; ++pre) for (int st = 0; st < 2; ++st) chain(pre, st, 20);      // load every code object
    CHK(hipStreamSynchronize(s));

    float t = 0;
    for (int alt = 0; alt < 3; ++alt) {
        float us[2];
        for (int pre = 0; pre < 2; ++pre) {
            float best = 1e9f, sum = 0;
            const int reps = 7;
            for (int rep = 0; rep < reps; ++rep) {
                CHK(hipEventRecord(e0, s)); chain(pre, false, pairs); CHK(hipEventRecord(e1, s)); CHK(hipEventSynchronize(e1));
                CHK(hipEventElapsedTime(&t, e0, e1)); best = std::min(best, t); sum += t;
            }
            us[pre] = best * 1e3f / pairs;
            printf("alternation %d, %-9s: %.3f us per pair of dependent launches (best of %d), %.3f mean\n", alt, pre ? "preloaded" : "struct", us[pre],
                   reps, sum * 1e3f / pairs / reps);
        }
        printf("alternation %d: preloaded form %+.3f us per pair, %+.3f us per launch\n", alt, us[1] - us[0], (us[1] - us[0]) / 2);
    }

    // head times: the stamped instantiations in the same chain; the last pair's stamps stay
    std::vector<u64> h((size_t)2 * (NA + NB));
    for (int alt = 0; alt < 3; ++alt) {
        for (int pre = 0; pre < 2; ++pre) {
            chain(pre, true, 50); CHK(hipStreamSynchronize(s));
            CHK(hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost));
            for (int kern = 0; kern < 2; ++kern) {
                const int nb = kern ? NB : NA, off = kern ? 2 * NA : 0;
                std::vector<long long> d(nb);
                for (int b = 0; b < nb; ++b) d[b] = (long long)(h[off + 2 * b + 1] - h[off + 2 * b]);
                std::sort(d.begin(), d.end());
                printf("alternation %d, %-9s, %4d x %4d threads: first instruction -> first vector load in hand: median %lld ns, max %lld ns, min %lld ns\n",
                       alt, pre ? "preloaded" : "struct", nb, kern ? 256 : 1024, d[nb / 2] * 10, d[nb - 1] * 10, d[0] * 10);
            }
        }
    }
    return 0;
}
