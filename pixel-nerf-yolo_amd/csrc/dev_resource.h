// Owning handles of the HIP resources the host side allocates: device buffers, pinned host blocks, events and streams.  Each is
// move-only and its destructor releases, so a struct that holds them needs no teardown code of its own.  They are members of
// heap-allocated handles only, never globals: a destructor that runs during static destruction would call into a HIP runtime
// that may already have shut down.  Whoever destroys a handle drains the device first (api_internal.h drain_device).
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <utility>

namespace pny {

int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

struct DeviceMem {
    static hipError_t alloc(void** p, size_t n) { return hipMalloc(p, n); }
    static hipError_t free(void* p) { return hipFree(p); }
    static constexpr const char* what = "hipMalloc(workspace)";
};
struct PinnedMem {   // device-visible host memory
    static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
    static constexpr const char* what = "hipHostMalloc(pinned block)";
};

// A block that only grows.  reserve() frees before it allocates.  hipFree waits for the device, and callers rely on that
// where a launch in flight may still read the old block; hipHostFree makes no such promise.
template <class Mem>
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~Buf() { release(); }
    int reserve(size_t need, const char* what = Mem::what) {   // what: names the site in the error text
        if (need <= bytes) return 0;
        release();
        hipError_t e = Mem::alloc(&p, need);
        if (e != hipSuccess) {
            p = nullptr;
            return hip_fail(e, what);
        }
        bytes = need;
        return 0;
    }
    void release() {
        if (p) (void)Mem::free(p);
        p = nullptr;
        bytes = 0;
    }
    float* f() const { return reinterpret_cast<float*>(p); }
};
using DevBuf = Buf<DeviceMem>;
using PinnedBuf = Buf<PinnedMem>;

// An event or a stream created on first use: ensure() creates it with the flags given unless it exists and returns a status
// like PNY_HIP does.  Converts to the raw handle, which is null while nothing was created.
template <class T, hipError_t (*Create)(T*, unsigned), hipError_t (*Destroy)(T)>
struct Lazy {
    T h = nullptr;
    Lazy() = default;
    Lazy(const Lazy&) = delete;
    Lazy& operator=(const Lazy&) = delete;
    Lazy(Lazy&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Lazy& operator=(Lazy&& o) noexcept {
        if (this != &o) {
            release();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~Lazy() { release(); }
    int ensure(unsigned flags, const char* what) {
        if (h) return 0;
        hipError_t e = Create(&h, flags);
        if (e == hipSuccess) return 0;
        h = nullptr;
        return hip_fail(e, what);
    }
    void release() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    operator T() const { return h; }
};
using Event = Lazy<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;   // flags 0 (hipEventDefault): a timing event
using Stream = Lazy<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// Small host -> device parameter tables that change from call to call (work lists of the weight-gradient GEMMs): staged
// through a pinned block; the block is rewritten only after the previous asynchronous copy out of it has executed.
struct PinnedStage {
    PinnedBuf host;
    Event ev;
    bool pending = false;
    int prepare(size_t bytes) {   // returns 0 and a writable block of >= bytes
        if (pending) {
            hipError_t e = hipEventSynchronize(ev);
            if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize(table stage)");
            pending = false;
        }
        if (bytes > host.bytes)
            if (int rc = host.reserve(bytes * 2, "hipHostMalloc(table stage)")) return rc;
        return ev.ensure(hipEventDisableTiming, "hipEventCreate(table stage)");
    }
    int upload(void* dst_dev, size_t bytes, hipStream_t st) {
        hipError_t e = hipMemcpyAsync(dst_dev, host.p, bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(table stage)");
        e = hipEventRecord(ev, st);
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord(table stage)");
        pending = true;
        return 0;
    }
};

}  // namespace pny
