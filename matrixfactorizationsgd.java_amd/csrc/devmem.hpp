// devmem.hpp -- the owners of what the device lends: every hipMalloc of the library lives in a DevBuf, which frees it (a
// pointer never leaves its DevBuf: ownership moves from one DevBuf to another);
// the DSGD ring's streams and events live in a Stream / an Event.
// Host-compilable (the C-ABI units, dsgd.cpp): the runtime API only.
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace mfsgd {

// Bytes held by the DevBufs of this process (mfsgd_debug_device_bytes): what a test compares before and after a
// call to see that nothing was kept -- free-memory readings of a shared GPU cannot tell.
inline std::atomic<int64_t> g_dev_live_bytes{0};

class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.forget(); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            bytes_ = o.bytes_;
            o.forget();
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    void* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T>
    T* as() const {
        return static_cast<T*>(p_);
    }

    // At least `bytes` bytes (16 for 0): a buffer that is already that large is kept, contents and all; a smaller one
    // is freed first.
    hipError_t alloc(size_t bytes) {
        if (p_ && bytes_ >= bytes) return hipSuccess;
        reset();
        if (bytes == 0) bytes = 16;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) {
            p_ = p;
            bytes_ = bytes;
            g_dev_live_bytes.fetch_add((int64_t)bytes, std::memory_order_relaxed);
        }
        return e;
    }
    void reset() {
        if (!p_) return;
        (void)hipFree(p_);
        g_dev_live_bytes.fetch_sub((int64_t)bytes_, std::memory_order_relaxed);
        forget();
    }

private:
    void forget() {
        p_ = nullptr;
        bytes_ = 0;
    }
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// A DevBuf of elements of one type, so that a buffer's element type and its size are written once: data() is typed, and
// alloc(n) and size() count elements, with DevBuf::alloc's semantics (a buffer that is large enough is kept, 0 elements
// become 16 bytes; size() is what is there, so at least the n asked for).  The memory and the live-bytes accounting
// are the DevBuf's, and one that another owner filled (the device packer's) is adopted whole.  Move-only, as its DevBuf.
template <class T>
class DevArray {
public:
    DevArray() = default;
    DevArray(DevBuf&& b) noexcept : buf_(std::move(b)) {}

    T* data() const { return buf_.template as<T>(); }
    size_t size() const { return buf_.bytes() / sizeof(T); }
    const DevBuf& buf() const { return buf_; }
    explicit operator bool() const { return (bool)buf_; }
    hipError_t alloc(size_t n) { return buf_.alloc(n * sizeof(T)); }
    void reset() { buf_.reset(); }

private:
    DevBuf buf_;
};

// The owner of a stream or an event: empty until create(flags), destroyed with its owner, handed to the runtime as
// the plain handle it converts to.
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class DevHandle {
public:
    DevHandle() = default;
    DevHandle(const DevHandle&) = delete;
    DevHandle& operator=(const DevHandle&) = delete;
    DevHandle(DevHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~DevHandle() { reset(); }

    hipError_t create(unsigned flags) {
        reset();
        return Create(&h_, flags);
    }
    operator H() const { return h_; }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }

private:
    H h_ = nullptr;
};
using Stream = DevHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using Event = DevHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

}  // namespace mfsgd
