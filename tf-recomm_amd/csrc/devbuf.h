// devbuf.h - owners of the device and pinned host memory behind the C-ABI's handles (api.hip, als_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfr {

// Move-only owner of capacity() elements of T: device memory, or pinned host memory when Host.
// reserve(n, s) grows to exactly n elements when n exceeds the capacity: it synchronises s (whatever may still read the
// old memory runs there), frees, then allocates; on failure the buffer is left empty (capacity 0).  The memory is freed
// on the current device, so an owner is released with its handle's device current.
template <typename T, bool Host = false>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    int64_t capacity() const { return cap_; }

    hipError_t reserve(int64_t n, hipStream_t s) {
        if (n <= cap_) return hipSuccess;
        if (p_) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
            reset();
        }
        void* p = nullptr;
        const hipError_t e = Host ? hipHostMalloc(&p, (size_t)n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, (size_t)n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }

    void reset() {
        if (p_) (void)(Host ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }

private:
    T* p_ = nullptr;
    int64_t cap_ = 0;
};

template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using HostBuf = Buf<T, true>;

}  // namespace tfr
