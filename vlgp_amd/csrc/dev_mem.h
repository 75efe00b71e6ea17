// Who owns device memory: move-only owners of device blocks, pinned / mapped host blocks, events and
// streams, and the grow-only buffer built on them.  A pointer is EMPTY, OWNED (freed once, by whoever holds it last) or
// BORROWED (someone else's block: never freed here).  Every owner keeps the process-wide counters of live blocks and
// bytes up to date (vlgp_debug_live_memory).  The header names hipMalloc, hipFree, hipHostMalloc, hipHostFree,
// hipStreamSynchronize, hipEventDestroy, hipStreamDestroy and their types only, so a host program can supply stand-ins
// and compile it without HIP (tests/dev_mem_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

// live device blocks, device bytes, host blocks, host bytes
inline std::atomic<int64_t> g_live_memory[4];

struct DeviceSpace {
    enum { counter = 0 };
    static hipError_t get(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static hipError_t put(void* p) { return hipFree(p); }
};
struct HostSpace {  // flags: hipHostMallocDefault, hipHostMallocMapped, ...
    enum { counter = 2 };
    static hipError_t get(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static hipError_t put(void* p) { return hipHostFree(p); }
};

template <class T, class Space>
class MemPtr {
    T* p_ = nullptr;
    size_t bytes_ = 0;  // of an owned block; 0: empty or borrowed
    bool owned_ = false;
    void take(MemPtr& o) {
        p_ = o.p_; bytes_ = o.bytes_; owned_ = o.owned_;
        o.p_ = nullptr; o.bytes_ = 0; o.owned_ = false;
    }

public:
    MemPtr() = default;
    MemPtr(const MemPtr&) = delete;
    MemPtr& operator=(const MemPtr&) = delete;
    MemPtr(MemPtr&& o) noexcept { take(o); }
    MemPtr& operator=(MemPtr&& o) noexcept {
        if (this != &o) {
            reset();
            take(o);
        }
        return *this;
    }
    ~MemPtr() { reset(); }

    // n elements of its own, whatever it held before released first; empty after a failure
    hipError_t alloc(size_t n, unsigned flags = 0) {
        reset();
        void* q = nullptr;
        const hipError_t e = Space::get(&q, n * sizeof(T), flags);
        if (e != hipSuccess || !q) return e;
        p_ = static_cast<T*>(q); bytes_ = n * sizeof(T); owned_ = true;
        g_live_memory[Space::counter] += 1;
        g_live_memory[Space::counter + 1] += (int64_t)bytes_;
        return e;
    }
    void borrow(T* p) {
        reset();
        p_ = p;
    }
    void reset() {
        if (owned_) {
            (void)Space::put(const_cast<void*>(static_cast<const void*>(p_)));
            g_live_memory[Space::counter] -= 1;
            g_live_memory[Space::counter + 1] -= (int64_t)bytes_;
        }
        p_ = nullptr; bytes_ = 0; owned_ = false;
    }
    bool owned() const { return owned_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};
template <class T> using DevPtr = MemPtr<T, DeviceSpace>;
template <class T> using HostPtr = MemPtr<T, HostSpace>;

// A buffer that only grows.  ensure(n, capacity, stream): nothing when n <= len; otherwise the stream that uses the
// buffer is drained (when one is given), the old block goes and `capacity` elements are allocated.  Pointer empty and
// len 0 from before the allocation until it has succeeded.  The call site keeps its capacity rule and its stream.
template <class T, class Ptr = DevPtr<T>>
struct GrowBuf {
    Ptr p;
    int64_t len = 0;
    GrowBuf() = default;
    GrowBuf(GrowBuf&& o) noexcept : p(static_cast<Ptr&&>(o.p)), len(o.len) { o.len = 0; }
    GrowBuf& operator=(GrowBuf&& o) noexcept {
        if (this != &o) {
            p = static_cast<Ptr&&>(o.p);
            len = o.len;
            o.len = 0;
        }
        return *this;
    }
    hipError_t ensure(int64_t n, int64_t capacity, hipStream_t stream = nullptr, unsigned flags = 0) {
        if (n <= len) return hipSuccess;
        if (stream) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
        }
        len = 0;
        p.reset();
        const hipError_t e = p.alloc((size_t)capacity, flags);
        if (e == hipSuccess) len = capacity;
        return e;
    }
    T* get() const { return p.get(); }
    operator T*() const { return p.get(); }
};
template <class T> using HostGrowBuf = GrowBuf<T, HostPtr<T>>;

// An event or a stream: created by the site (put() hands out where the handle goes), destroyed here.
template <class H, hipError_t (*Destroy)(H)>
class DevHandle {
    H h_ = nullptr;

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
    H* put() {
        reset();
        return &h_;
    }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    operator H() const { return h_; }
};
using DevEvent = DevHandle<hipEvent_t, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamDestroy>;
