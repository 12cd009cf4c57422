// srcnn_owned.hpp -- the two owner types of the host layer.  Every HIP resource the library keeps (srcnn_host.hpp binds
// these templates to events, streams, graphs, device and page-locked memory) is a member of one of them, so a struct
// releases what it holds by being destroyed or assigned from an empty one, and a creation that fails half way releases the
// half it got.  No HIP in here: tests/host/host_sanitize.cpp drives both under ASan / UBSan / TSan with malloc-backed traits.
//
// Neither destructor selects a device: whoever destroys a context-bound object binds its device first.  No owner may have
// static or thread storage duration (at process exit the HIP runtime may already be gone).
#pragma once
#include <cstddef>

namespace srcnn {

// One handle H (pointer-like: hipEvent_t, hipStream_t ...); Traits::destroy(h) runs exactly once per non-null handle.
template <class H, class Traits>
class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.release()) {}
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); h_ = o.release(); } return *this; }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != H{}; }
    void reset() { if (H h = release()) Traits::destroy(h); }
    H release() { H h = h_; h_ = H{}; return h; }      // hands the handle out; the caller destroys it
    // the out-parameter of a create call: hipEventCreate(e.put()).  The owner is empty afterwards unless the call fills it.
    H* put() { reset(); return &h_; }
private:
    H h_{};
};

// A block of `size()` elements that only ever grows.  Alloc has drain(), alloc(void** p, size_t bytes, args...) -> 0 or an
// error code, and free(void*).  Growing drains (work queued earlier may still use the old block), frees the old block and
// only then allocates: these are the multi-gigabyte scratch buffers, and a band sized to the workspace budget may not fit twice.
template <class T, class Alloc>
class GrowBuf {
public:
    GrowBuf() = default;
    GrowBuf(GrowBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    GrowBuf& operator=(GrowBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    ~GrowBuf() { reset(); }
    T* data() const { return p_; }
    size_t size() const { return n_; }
    void reset() { if (p_) Alloc::free(p_); p_ = nullptr; n_ = 0; }
    // at least `want` elements; `a...` goes to the allocator.  On failure the buffer is empty and the error is returned.
    template <class... A>
    int grow(size_t want, A&&... a)
    {
        if (want <= n_) return 0;
        if (p_) { Alloc::drain(); reset(); }
        void* q = nullptr;
        if (int rc = Alloc::alloc(&q, want * sizeof(T), a...)) return rc;
        p_ = static_cast<T*>(q);
        n_ = want;
        return 0;
    }
private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace srcnn
