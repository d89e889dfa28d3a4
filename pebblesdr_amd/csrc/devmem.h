// devmem.h -- the two types that own memory in this library: DevBuf<T> (hipMalloc) and PinnedBuf<T> (hipHostMalloc).
// Move-only; allocating into a buffer that holds something frees that first; the destructor frees.  A raw T * beside one of
// these is a view of somebody else's memory.  Host-only header (no device code): it compiles with a plain C++17 compiler.
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace pg {

int fail(int code, const char *fmt, ...);  // common.h

// bytes this library holds in this process right now (pebblegpu_live_bytes)
inline std::atomic<uint64_t> g_live_device{0}, g_live_pinned{0};

struct DeviceMem {
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t put(void *p) { return hipFree(p); }
    static std::atomic<uint64_t> &live() { return g_live_device; }
    static const char *name() { return "hipMalloc"; }
};
struct PinnedMem {
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t put(void *p) { return hipHostFree(p); }
    static std::atomic<uint64_t> &live() { return g_live_pinned; }
    static const char *name() { return "hipHostMalloc"; }
};

struct PortableMem : PinnedMem {  // pinned for every device, not only the current one (the multibank's shared slots)
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocPortable); }
};

template <class T, class Mem>
class OwnedBuf {
    T *p_ = nullptr;
    size_t bytes_ = 0;  // (bytes, not elements: the destructor of a buffer of a type that is only declared needs no sizeof)

public:
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_; bytes_ = o.bytes_;
            o.p_ = nullptr; o.bytes_ = 0;
        }
        return *this;
    }
    ~OwnedBuf() { release(); }

    T *get() const { return p_; }
    size_t size() const { return bytes_ / sizeof(T); }  // elements
    operator T *() const { return p_; }
    T *operator->() const { return p_; }

    void release()
    {
        if (p_) {
            (void)Mem::put(p_);
            Mem::live() -= (uint64_t)bytes_;
        }
        p_ = nullptr;
        bytes_ = 0;
    }
    int alloc(size_t n)
    {
        release();
        void *q = nullptr;
        const hipError_t e = Mem::get(&q, n * sizeof(T));
        if (e != hipSuccess) return fail(-3, "%s of %zu bytes failed: %s", Mem::name(), n * sizeof(T), hipGetErrorString(e));
        if (!q) return 0;  // (a request of no bytes)
        p_ = static_cast<T *>(q);
        bytes_ = n * sizeof(T);
        Mem::live() += (uint64_t)bytes_;
        return 0;
    }
    int alloc_zero(size_t n)
    {
        if (int rc = alloc(n)) return rc;
        return filled(hipMemset(p_, 0, bytes_), "hipMemset");
    }
    // the synchronous copy the init paths use: the host array may go away when this returns
    int upload(const T *host, size_t n)
    {
        if (int rc = alloc(n)) return rc;
        return filled(hipMemcpy(p_, host, bytes_, hipMemcpyHostToDevice), "hipMemcpy");
    }
    // Grow-only, for a buffer that work queued on `s` may still be using: waits for the stream, frees, then allocates.  A request
    // the buffer already covers returns at once (no synchronisation); after a failure the buffer is empty.
    int grow(hipStream_t s, size_t n)
    {
        if (n * sizeof(T) <= bytes_) return 0;
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(-3, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
        return alloc(n);
    }

private:
    int filled(hipError_t e, const char *what)
    {
        if (e == hipSuccess) return 0;
        const size_t bytes = bytes_;
        release();
        return fail(-3, "%s of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
    }
};

template <class T> using DevBuf = OwnedBuf<T, DeviceMem>;
template <class T> using PinnedBuf = OwnedBuf<T, PinnedMem>;
template <class T> using PortableBuf = OwnedBuf<T, PortableMem>;

#define PG_TRY(expr)                   \
    do {                               \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

}  // namespace pg
