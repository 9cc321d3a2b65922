// mnv_devmem.h -- who owns device and pinned memory ("Ownership of device memory"): every hipMalloc / hipHostMalloc of the library
// sits behind one move-only owner, so no handle keeps a free list.  Host-only and header-only; plain C++ units include it too.
// The owners return the raw hipError_t: callers wrap it (check_hip / hip_check) with the text of their site.
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <utility>

namespace mnv {

enum class Mem { device, pinned };

// bytes the owners of this process hold right now (mnv_hook_live_bytes of the test-hook library reads them)
template <Mem K>
inline std::atomic<long long> &live_bytes() {
    static std::atomic<long long> n{0};
    return n;
}

template <typename T, Mem K = Mem::device>
class Buffer {
   public:
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept { swap(o); }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~Buffer() { reset(); }

    // frees what it holds, then allocates `count` elements (uninitialised); empty after a failure
    hipError_t alloc(size_t count) {
        reset();
        void *p = nullptr;
        const hipError_t e = K == Mem::device ? hipMalloc(&p, count * sizeof(T)) : hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) adopt(static_cast<T *>(p), count);
        return e;
    }
    void reset() {
        if (T *p = release()) (void)(K == Mem::device ? hipFree(p) : hipHostFree(p));
    }
    // takes over / gives up an allocation of the same kind that was made elsewhere
    void adopt(T *p, size_t count) {
        reset();
        p_ = p, n_ = p ? count : 0;
        live_bytes<K>().fetch_add((long long)bytes(), std::memory_order_relaxed);
    }
    T *release() {
        live_bytes<K>().fetch_sub((long long)bytes(), std::memory_order_relaxed);
        n_ = 0;
        return std::exchange(p_, nullptr);
    }
    void swap(Buffer &o) noexcept {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
    }
    T *get() const { return p_; }
    size_t count() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
    explicit operator bool() const { return p_ != nullptr; }

   private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
using PinnedBuffer = Buffer<T, Mem::pinned>;

// Grow-only array: after hipSuccess `b` holds at least `need` elements.  A new array has `slack` (>= need) elements: the caller's formula.
// `wait`: the stream may still use the old array, so it is drained before that goes.  keep > 0: the first `keep` elements move to the new
// array (stream-ordered copy, then a wait for it); otherwise the contents are lost and the old array goes before the new one is made.
template <typename T>
hipError_t grow(Buffer<T> &b, size_t need, size_t slack, hipStream_t stream, bool wait, size_t keep = 0) {
    if (need <= b.count()) return hipSuccess;
    hipError_t e;
    if (b && keep > 0) {
        Buffer<T> q;
        if ((e = q.alloc(slack)) != hipSuccess || (e = hipMemcpyAsync(q.get(), b.get(), keep * sizeof(T), hipMemcpyDeviceToDevice, stream)) != hipSuccess ||
            (e = hipStreamSynchronize(stream)) != hipSuccess)
            return e;
        b.swap(q);
        return hipSuccess;
    }
    if (b && wait && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    return b.alloc(slack);
}

// Device word(s) and their pinned mirror: both exist or neither does.
template <typename T>
struct Mirrored {
    Buffer<T> dev;
    PinnedBuffer<T> host;
    // *pinned_failed says which of the two allocations the error belongs to (for the caller's text)
    hipError_t alloc(size_t count, bool *pinned_failed = nullptr) {
        hipError_t e = dev.alloc(count);
        if (pinned_failed) *pinned_failed = false;
        if (e == hipSuccess && (e = host.alloc(count)) != hipSuccess) {
            dev.reset();
            if (pinned_failed) *pinned_failed = true;
        }
        return e;
    }
    explicit operator bool() const { return (bool)dev; }
};

// One hipEvent_t, destroyed with its owner (neither copied nor moved).
class Event {
   public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { reset(); }
    hipError_t create(unsigned flags) {
        reset();
        return hipEventCreateWithFlags(&e_, flags);
    }
    void reset() {
        if (e_) (void)hipEventDestroy(std::exchange(e_, nullptr));
    }
    hipEvent_t get() const { return e_; }

   private:
    hipEvent_t e_ = nullptr;
};

}  // namespace mnv
