// Owning handles of the HIP resources the host side allocates: device buffers, pinned host blocks, events and streams.  Each is
// move-only and its destructor releases, so a struct that holds them needs no teardown code of its own.  They are members of
// heap-allocated handles only, never globals: a destructor that runs during static destruction would call into a HIP runtime
// that may already have shut down (the one exception, StreamBlocks below, therefore never frees).  Whoever destroys a handle
// drains the device first (api_internal.h drain_device).
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

// The order of one scene's calls across streams.  A scene's state (latent, projected maps, workspace, cross-view slab) is
// written and read by the kernels of successive calls without any host synchronisation, which is only ordered if those calls
// share a stream.  When a call arrives on a DIFFERENT stream than the previous call on the same scene, the new stream is made
// to wait for everything the previous call enqueued (one event record + one stream wait, paid only on a stream switch).
// Move-only like the event it owns.
struct StreamOrder {
    hipStream_t last = nullptr;   // stream the last call on the scene was enqueued on
    bool has_last = false;
    Event ev;
    bool ev_valid = false;        // ev was recorded behind the last call's work (mark)

    // Every call that enqueues work of the scene on `st` enters first.
    int enter(hipStream_t st) {
        if (has_last && last != st) {
            if (int rc = ev.ensure(hipEventDisableTiming, "hipEventCreate(stream order)")) return rc;
            if (ev_valid) {   // recorded right behind the previous call's work (mark)
                if (int rc = wait(st)) return rc;
            } else if (hipEventRecord(ev, last) == hipSuccess) {
                if (int rc = wait(st)) return rc;
            } else {
                (void)hipGetLastError();  // the previous stream no longer exists: its work has drained
            }
        }
        ev_valid = false;   // the call that enters enqueues new work
        last = st;
        has_last = true;
        return 0;
    }
    // Records the order event NOW, behind the work just enqueued on the scene's stream: a later call on another stream then
    // waits for exactly this point and not for whatever else the first stream has been given in between (pny_scenes_encode:
    // the scenes of a super-batch are encoded on one stream and rendered on one stream each).
    int mark(hipStream_t st) {
        if (int rc = ev.ensure(hipEventDisableTiming, "hipEventCreate(stream order)")) return rc;
        hipError_t e = hipEventRecord(ev, st);
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord(s->order_ev, st)");
        ev_valid = true;
        return 0;
    }
    // Work that reads what the scene's calls read (pny_model_refresh: the packed weights) is about to be enqueued on `st` by
    // someone other than the scene: `st` waits for the scene's last call and becomes the scene's stream, so that the scene's
    // next call in turn waits for that work.
    int hand_over(hipStream_t st) {
        if (has_last && last != st) {
            if (int rc = ev.ensure(hipEventDisableTiming, "hipEventCreate(refresh order)")) return rc;
            if (hipEventRecord(ev, last) == hipSuccess) {
                if (int rc = wait(st)) return rc;
            } else {
                (void)hipGetLastError();
            }
            last = st;   // the scene's next call must in turn wait for the work on st
        } else if (!has_last) {
            last = st;
            has_last = true;
        }
        // an order event recorded BEFORE this hand-over (mark) no longer covers the scene's stream: a later call on another
        // stream has to wait for the work on st too, so enter must record a fresh event behind it
        ev_valid = false;
        return 0;
    }

private:
    int wait(hipStream_t st) {
        hipError_t e = hipStreamWaitEvent(st, ev, 0);
        return e == hipSuccess ? 0 : hip_fail(e, "hipStreamWaitEvent(st, s->order_ev, 0)");
    }
};

// One device block per (current device, stream): the ticket counter and the partial-sum table of a reduction kernel (loss.hip,
// metrics.hip).  Launches on one stream follow one another, so they can share a block; launches on different streams may
// overlap and get their own.  A block is made on the first request on a stream, only grows (it frees, then allocates: hipFree
// waits for the device), and its first zero_bytes bytes are zeroed ON that stream (no host wait) whenever it is made.
// A table of these is a global and is never freed (a few KB per stream the process ever used): the stated exception to the
// "never globals" rule at the top of this file.  The blocks are raw and the slots are never deleted on purpose, because a
// global's destructor would call hipFree after the HIP runtime may have shut down.
// Mutex: std::mutex in the library.  A parameter so that this header needs no more than it includes.
template <class Mutex>
struct StreamBlocks {
    const char* what_alloc;   // name the table's allocation and zero fill in the error text
    const char* what_zero;
    Mutex mu;
    struct Slot {
        int dev;
        hipStream_t st;
        void* p;
        size_t bytes;
        Slot* next;
    };
    Slot* slots = nullptr;
    StreamBlocks(const char* alloc_site, const char* zero_site) : what_alloc(alloc_site), what_zero(zero_site) {}

    // -> *out: the block of the current device and `st`, at least `need` bytes
    int get(hipStream_t st, size_t need, size_t zero_bytes, void** out) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return hip_fail(e, "hipGetDevice(&dev)");
        mu.lock();
        Slot* s = slot(dev, st);
        const int rc = grow(s, need, zero_bytes);
        if (!rc) *out = s->p;
        mu.unlock();
        return rc;
    }

private:
    Slot* slot(int dev, hipStream_t st) {
        for (Slot* s = slots; s; s = s->next)
            if (s->dev == dev && s->st == st) return s;
        return slots = new Slot{dev, st, nullptr, 0, slots};
    }
    int grow(Slot* s, size_t need, size_t zero_bytes) {
        if (need <= s->bytes) return 0;
        if (s->p) {
            hipError_t e = hipFree(s->p);
            if (e != hipSuccess) return hip_fail(e, "hipFree(w.p)");
        }
        s->p = nullptr, s->bytes = 0;
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, need);
        if (e != hipSuccess) return hip_fail(e, what_alloc);
        e = hipMemsetAsync(q, 0, zero_bytes, s->st);
        if (e != hipSuccess) {
            (void)hipFree(q);
            return hip_fail(e, what_zero);
        }
        s->p = q, s->bytes = need;
        return 0;
    }
};

}  // namespace pny
