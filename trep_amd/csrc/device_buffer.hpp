// device_buffer.hpp -- owners of the HIP resources of the host layer (trepamd.hip): device memory, pinned host memory, events.
// Host only.  Each owner is move-only (a move swaps, so the source frees what the target held) and releases what it holds in
// its destructor: a struct of them needs no list of what to free, and an early return leaks nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

namespace tg {

template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept { *this = std::move(o); }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
    ~DeviceBuffer() { if (p_) (void)hipFree(p_); }
    T *get() const { return p_; }
    size_t count() const { return n_; }      // elements asked for
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { DeviceBuffer dropped(std::move(*this)); }
    // A lazy buffer: allocated by the first call (one element at least, so get() is not null afterwards) and zero-filled on
    // request; later calls keep what is there.
    hipError_t ensure(size_t count, bool zero = false) {
        if (p_) return hipSuccess;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = count;
        return zero ? hipMemset(p_, 0, bytes) : hipSuccess;
    }
private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

// Pinned host memory (hipHostMalloc with the given flags), allocated by the first ensure() like a DeviceBuffer.
template <class T>
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer &&o) noexcept { *this = std::move(o); }
    PinnedBuffer &operator=(PinnedBuffer &&o) noexcept { std::swap(p_, o.p_); return *this; }
    ~PinnedBuffer() { if (p_) (void)hipHostFree(p_); }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { PinnedBuffer dropped(std::move(*this)); }
    hipError_t ensure(size_t count, unsigned int flags) {
        if (p_) return hipSuccess;
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p_), (count ? count : 1) * sizeof(T), flags);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
private:
    T *p_ = nullptr;
};

class Event {
public:
    Event() = default;
    Event(Event &&o) noexcept { *this = std::move(o); }
    Event &operator=(Event &&o) noexcept { std::swap(e_, o.e_); return *this; }
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    hipEvent_t get() const { return e_; }
    hipError_t create(unsigned int flags = hipEventDefault) {      // on an empty owner
        hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
private:
    hipEvent_t e_ = nullptr;
};

}  // namespace tg
