/*
 * dvo_buffers.h -- the two owning buffer types of the host layer: DevBuf<T> (hipMalloc / hipFree) and PinnedBuf<T>
 * (hipHostMalloc / hipHostFree).  Move-only; the destructor frees.  Host only; internal, not installed.
 *
 * Invariant: a pointer is never held without its size and a size never without its pointer -- after a failed alloc() the
 * buffer is empty and size() == 0.  The types know nothing about streams: whoever frees a buffer the device may still be
 * using waits for its stream first (regrow() in dvo_ctx.h does).
 */
#ifndef DVO_BUFFERS_H_
#define DVO_BUFFERS_H_

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace dvo_host {

template <class T>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    /* room for n elements (contents undefined); a live allocation is freed first, never held beside the new one */
    hipError_t alloc(size_t n) {
        reset();
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, sizeof(T) * n);
        if (e == hipSuccess && p) { p_ = static_cast<T *>(p); n_ = n; }
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
    size_t size() const { return n_; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
};

template <class T>
class PinnedBuf {
    T *p_ = nullptr;
    size_t n_ = 0;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t n) {
        reset();
        void *p = nullptr;
        const hipError_t e = hipHostMalloc(&p, sizeof(T) * n, hipHostMallocDefault);
        if (e == hipSuccess && p) { p_ = static_cast<T *>(p); n_ = n; }
        return e;
    }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr; n_ = 0;
    }
    size_t size() const { return n_; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
};

}  // namespace dvo_host
#endif
