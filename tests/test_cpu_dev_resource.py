"""
The owning handles of csrc/dev_resource.h (DevBuf, PinnedBuf, Event, Stream, PinnedStage), compiled by g++ into a program of its
own against counting fakes of the HIP entry points the header uses: no HIP library is linked and no GPU is needed.  The fakes
hand out real heap blocks and the program is built with -fsanitize=address,undefined, so a double free or a use after a move is
caught twice: by the fakes' own books and by the sanitizer.
"""
import os
import shutil
import subprocess

import pytest

from pixel_nerf_yolo_amd import lib as plib

CSRC = plib.CSRC
ROCM_INCLUDE = "/opt/rocm/include"

HOST_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "dev_resource.h"
using namespace pny;

// ------------------------------------------------------------------ the fakes: every call is logged, every handle is booked
static std::vector<std::string> g_log;
static std::set<void*> g_dev, g_pin, g_ev, g_st;
static std::vector<unsigned> g_flags;          // of every event / stream created, in order
static long g_made[4], g_gone[4];              // device, pinned, event, stream
static int g_fail_next = 0;                    // the next allocation / creation fails
static int g_fail_record = 0, g_fail_memset = 0;   // the next hipEventRecord / hipMemsetAsync fails
static int g_device = 0;                       // what hipGetDevice answers
struct StreamCall {                            // which stream a record, a wait or a zero fill names, and its event or block
    std::string op;
    hipStream_t st;
    void* what;
    size_t bytes;
    bool operator==(const StreamCall& o) const { return op == o.op && st == o.st && what == o.what && bytes == o.bytes; }
};
static std::vector<StreamCall> g_slog;
static std::string g_what;                     // the site the last hip_fail named
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)
static void gone(std::set<void*>& live, void* p, int kind, const char* name) {
    if (!live.erase(p)) { printf("FAILED: %s of a handle that is not live (double free)\n", name); exit(1); }
    ++g_gone[kind];
    g_log.push_back(name);
}
static hipError_t made(std::set<void*>& live, void** out, size_t n, int kind, const char* name) {
    g_log.push_back(name);
    if (g_fail_next) { g_fail_next = 0; return hipErrorOutOfMemory; }
    *out = malloc(n ? n : 1);
    live.insert(*out);
    ++g_made[kind];
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return made(g_dev, p, n, 0, "hipMalloc"); }
hipError_t hipFree(void* p) { gone(g_dev, p, 0, "hipFree"); free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned flags) { CHECK(flags == hipHostMallocDefault); return made(g_pin, p, n, 1, "hipHostMalloc"); }
hipError_t hipHostFree(void* p) { gone(g_pin, p, 1, "hipHostFree"); free(p); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    hipError_t r = made(g_ev, reinterpret_cast<void**>(e), 8, 2, "hipEventCreateWithFlags");
    if (r == hipSuccess) g_flags.push_back(flags);
    return r;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { gone(g_ev, e, 2, "hipEventDestroy"); free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    CHECK(g_ev.count(e));
    g_log.push_back("hipEventRecord");
    g_slog.push_back({"record", s, e, 0});
    if (g_fail_record) { g_fail_record = 0; return hipErrorInvalidHandle; }   // (the stream is gone)
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) {
    CHECK(g_ev.count(e) && flags == 0);
    g_log.push_back("hipStreamWaitEvent");
    g_slog.push_back({"wait", s, e, 0});
    return hipSuccess;
}
hipError_t hipGetLastError(void) { g_log.push_back("hipGetLastError"); return hipSuccess; }
hipError_t hipGetDevice(int* d) { g_log.push_back("hipGetDevice"); *d = g_device; return hipSuccess; }
hipError_t hipMemsetAsync(void* p, int value, size_t n, hipStream_t s) {
    CHECK(g_dev.count(p) && value == 0);
    g_log.push_back("hipMemsetAsync");
    g_slog.push_back({"zero", s, p, n});
    if (g_fail_memset) { g_fail_memset = 0; return hipErrorInvalidValue; }
    memset(p, 0, n);   // (past the block's end: the sanitizer reports it)
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) { CHECK(g_ev.count(e)); g_log.push_back("hipEventSynchronize"); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t e) { CHECK(g_ev.count(e)); g_log.push_back("hipEventQuery"); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    hipError_t r = made(g_st, reinterpret_cast<void**>(s), 8, 3, "hipStreamCreateWithFlags");
    if (r == hipSuccess) g_flags.push_back(flags);
    return r;
}
hipError_t hipStreamDestroy(hipStream_t s) { gone(g_st, s, 3, "hipStreamDestroy"); free(s); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t) {
    CHECK(kind == hipMemcpyHostToDevice && g_pin.count(const_cast<void*>(src)) && g_dev.count(dst));
    memcpy(dst, src, n);
    g_log.push_back("hipMemcpyAsync");
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "fake"; }
}
namespace pny {
int fail(int code, const std::string&) { return code; }
int hip_fail(hipError_t e, const char* what) { g_what = what; return 1000 + (int)e; }
}
static long count(const char* name) {
    long n = 0;
    for (const std::string& s : g_log) n += s == name;
    return n;
}
static bool balanced() {   // nothing live, and every handle made went exactly once
    for (int k = 0; k < 4; ++k) if (g_made[k] != g_gone[k]) return false;
    return g_dev.empty() && g_pin.empty() && g_ev.empty() && g_st.empty();
}
struct RingEntry {   // the shape of optim_api.hip's AdamGradTable
    PinnedBuf host;
    Event ev;
    bool pending = false;
};

static void scope_exit() {
    {
        DevBuf d;
        PinnedBuf p;
        Event e;
        Stream s;
        PinnedStage st;
        DevBuf unused;   // never reserved: nothing to free
        Event never;
        CHECK(d.reserve(100) == 0 && p.reserve(64) == 0 && e.ensure(hipEventDisableTiming, "e") == 0);
        CHECK(s.ensure(hipStreamNonBlocking, "s") == 0 && st.prepare(10) == 0);
        CHECK(d.p && d.bytes == 100 && d.f() == d.p && p.p && p.bytes == 64 && (hipEvent_t)e && (hipStream_t)s);
        CHECK(!unused.p && !(hipEvent_t)never);
        CHECK(g_made[0] == 1 && g_made[1] == 2 && g_made[2] == 2 && g_made[3] == 1 && g_gone[0] + g_gone[1] + g_gone[2] + g_gone[3] == 0);
    }
    CHECK(balanced());
    CHECK(count("hipFree") == 1 && count("hipHostFree") == 2 && count("hipEventDestroy") == 2 && count("hipStreamDestroy") == 1);
}

static void moves() {
    {
        DevBuf a;
        CHECK(a.reserve(32) == 0);
        void* block = a.p;
        DevBuf b(std::move(a));                    // move construction: the source is empty
        CHECK(!a.p && a.bytes == 0 && b.p == block && b.bytes == 32);
        DevBuf c;
        CHECK(c.reserve(16) == 0);
        c = std::move(b);                          // move assignment: the target's own block goes first
        CHECK(g_gone[0] == 1 && c.p == block && c.bytes == 32 && !b.p && b.bytes == 0);
        DevBuf& same = c;
        c = std::move(same);                       // onto itself: nothing happens
        CHECK(c.p == block && g_gone[0] == 1);
        Event e, f;
        CHECK(e.ensure(0, "e") == 0);
        hipEvent_t raw = e;
        f = std::move(e);
        CHECK(!(hipEvent_t)e && (hipEvent_t)f == raw);
        Stream s;
        CHECK(s.ensure(hipStreamNonBlocking, "s") == 0);
        Stream t(std::move(s));
        CHECK(!(hipStream_t)s && (hipStream_t)t);
        PinnedStage st;
        CHECK(st.prepare(8) == 0);
        PinnedStage st2(std::move(st));
        CHECK(!st.host.p && st2.host.p && st2.host.bytes == 16);
    }
    CHECK(balanced());
    {
        std::vector<Event> ev;                     // the timing events of a scene: grown one by one past every capacity
        std::vector<hipEvent_t> raw;
        const long ev_made = g_made[2], ev_gone = g_gone[2], pin_gone = g_gone[1];
        for (int i = 0; i < 37; ++i) {
            Event e;
            CHECK(e.ensure(0, "timing") == 0);
            raw.push_back(e);
            ev.push_back(std::move(e));
        }
        for (int i = 0; i < 37; ++i) CHECK((hipEvent_t)ev[i] == raw[i]);
        CHECK(g_made[2] == ev_made + 37 && g_gone[2] == ev_gone);   // relocation destroyed nothing
        std::vector<RingEntry> ring;               // the Adam ring: emplace_back relocates entries that own a block and an event
        for (int i = 0; i < 19; ++i) {
            ring.emplace_back();
            CHECK(ring.back().ev.ensure(hipEventDisableTiming, "ring") == 0 && ring.back().host.reserve(8 * (i + 1)) == 0);
            ring.back().pending = true;
        }
        for (int i = 0; i < 19; ++i) CHECK(ring[i].host.bytes == (size_t)8 * (i + 1) && ring[i].pending && g_ev.count((hipEvent_t)ring[i].ev));
        CHECK(g_gone[1] == pin_gone && g_gone[2] == ev_gone && g_made[2] == ev_made + 37 + 19);
        std::vector<DevBuf> allocs;                // EncoderWeights::allocs / zproj_allocs; clear() frees
        for (int i = 0; i < 9; ++i) {
            DevBuf b;
            CHECK(b.reserve(4) == 0);
            allocs.push_back(std::move(b));
        }
        CHECK(g_dev.size() == 9);
        allocs.clear();
        CHECK(g_dev.empty());
    }
    CHECK(balanced());
}

static void reserve() {
    DevBuf d;
    CHECK(d.reserve(0) == 0 && g_log.empty() && !d.p);
    CHECK(d.reserve(100) == 0 && g_log == std::vector<std::string>({"hipMalloc"}));
    void* first = d.p;
    CHECK(d.reserve(100) == 0 && d.reserve(1) == 0 && d.reserve(0) == 0 && g_log.size() == 1 && d.p == first);   // need <= bytes: no call
    CHECK(d.reserve(101) == 0 && d.bytes == 101);
    CHECK(g_log == std::vector<std::string>({"hipMalloc", "hipFree", "hipMalloc"}));   // grows: frees before it allocates
    g_fail_next = 1;
    CHECK(d.reserve(500) == 1000 + (int)hipErrorOutOfMemory);
    CHECK(!d.p && d.bytes == 0 && g_dev.empty());   // the old block is gone, nothing dangles
    CHECK(g_log == std::vector<std::string>({"hipMalloc", "hipFree", "hipMalloc", "hipFree", "hipMalloc"}));
    CHECK(d.reserve(8) == 0 && d.bytes == 8);        // and the buffer is usable again
    PinnedBuf p;
    g_fail_next = 1;
    CHECK(p.reserve(64) != 0 && !p.p && p.bytes == 0);
    CHECK(p.reserve(64) == 0 && p.reserve(32) == 0 && count("hipHostMalloc") == 2 && count("hipHostFree") == 0);
    CHECK(p.reserve(65) == 0 && count("hipHostMalloc") == 3 && count("hipHostFree") == 1 && p.bytes == 65);
}

static void stage() {
    DevBuf table;
    CHECK(table.reserve(1024) == 0);
    PinnedStage st;
    CHECK(st.prepare(100) == 0);
    CHECK(st.host.bytes == 200 && !st.pending && count("hipEventSynchronize") == 0);   // twice the request; nothing to wait for
    CHECK(g_flags == std::vector<unsigned>({hipEventDisableTiming}));
    void* block = st.host.p;
    CHECK(st.prepare(100) == 0 && st.prepare(200) == 0);                               // no upload in between: waits for nothing
    CHECK(count("hipEventSynchronize") == 0 && count("hipHostMalloc") == 1 && st.host.p == block && g_made[2] == 1);
    memcpy(st.host.p, "job table", 10);
    CHECK(st.upload(table.p, 10, nullptr) == 0 && st.pending);
    CHECK(!memcmp(table.p, "job table", 10) && count("hipMemcpyAsync") == 1 && count("hipEventRecord") == 1);
    CHECK(g_log[g_log.size() - 2] == "hipMemcpyAsync" && g_log.back() == "hipEventRecord");   // the event sits behind the copy
    CHECK(st.prepare(100) == 0 && !st.pending && count("hipEventSynchronize") == 1);   // a copy is pending: wait for it, once
    CHECK(st.prepare(100) == 0 && count("hipEventSynchronize") == 1);
    CHECK(st.upload(table.p, 10, nullptr) == 0);
    const size_t before = g_log.size();
    CHECK(st.prepare(201) == 0 && st.host.bytes == 402);                               // regrows to twice the request ...
    CHECK(g_log.size() == before + 3 && g_log[before] == "hipEventSynchronize" && g_log[before + 1] == "hipHostFree" &&
          g_log[before + 2] == "hipHostMalloc");                                       // ... only behind the pending copy
    CHECK(g_made[2] == 1);
    g_fail_next = 1;
    CHECK(st.prepare(1000) != 0 && !st.host.p && st.host.bytes == 0);
}

static void lazy() {
    Event e, t;
    Stream s;
    CHECK(!(hipEvent_t)e && !(hipStream_t)s && g_log.empty());                         // nothing until first use
    CHECK(e.ensure(hipEventDisableTiming, "e") == 0 && e.ensure(hipEventDisableTiming, "e") == 0 && e.ensure(0, "e") == 0);
    CHECK(t.ensure(hipEventDefault, "t") == 0 && t.ensure(hipEventDefault, "t") == 0);
    CHECK(s.ensure(hipStreamNonBlocking, "s") == 0 && s.ensure(hipStreamNonBlocking, "s") == 0);
    CHECK(g_made[2] == 2 && g_made[3] == 1 && g_log.size() == 3);                      // created once each
    CHECK(g_flags == std::vector<unsigned>({hipEventDisableTiming, hipEventDefault, hipStreamNonBlocking}));
    CHECK(hipEventDisableTiming != hipEventDefault && hipStreamNonBlocking != 0);
    Event bad;
    Stream bad_s;
    g_fail_next = 1;
    CHECK(bad.ensure(0, "bad") == 1000 + (int)hipErrorOutOfMemory && !(hipEvent_t)bad);
    g_fail_next = 1;
    CHECK(bad_s.ensure(hipStreamNonBlocking, "bad") != 0 && !(hipStream_t)bad_s);
    CHECK(bad.ensure(0, "bad") == 0 && (hipEvent_t)bad);                               // and the next use tries again
}

static void release_then_destructor() {
    {
        DevBuf d;
        PinnedBuf p;
        Event e;
        Stream s;
        CHECK(d.reserve(8) == 0 && p.reserve(8) == 0 && e.ensure(0, "e") == 0 && s.ensure(hipStreamNonBlocking, "s") == 0);
        d.release();
        p.release();
        e.release();
        s.release();
        CHECK(balanced() && !d.p && d.bytes == 0 && !p.p && !(hipEvent_t)e && !(hipStream_t)s);
        d.release();   // twice: nothing
        CHECK(d.reserve(8) == 0);   // usable again; the destructor frees this one
    }
    CHECK(balanced() && g_made[0] == 2 && g_made[1] == 1 && g_made[2] == 1 && g_made[3] == 1);
}

// ------------------------------------------------------------------ StreamOrder: the exact calls of a scene's stream order
static const hipStream_t A = (hipStream_t)0x10, B = (hipStream_t)0x20, C = (hipStream_t)0x30;   // never dereferenced
typedef std::vector<std::string> Log;
typedef std::vector<StreamCall> SLog;

static void order_enter() {
    StreamOrder o;
    CHECK(o.enter(A) == 0 && o.enter(A) == 0);                       // the first call and the same stream: nothing
    CHECK(g_log.empty() && g_slog.empty() && g_made[2] == 0 && o.has_last && o.last == A);
    CHECK(o.enter(B) == 0 && o.last == B && !o.ev_valid);            // a switch: one event, recorded on A, awaited on B
    CHECK(g_log == Log({"hipEventCreateWithFlags", "hipEventRecord", "hipStreamWaitEvent"}));
    CHECK(g_flags == std::vector<unsigned>({hipEventDisableTiming}) && g_made[2] == 1);
    hipEvent_t ev = o.ev;
    CHECK(g_slog == SLog({{"record", A, ev, 0}, {"wait", B, ev, 0}}));
    CHECK(o.enter(B) == 0 && g_log.size() == 3);
    CHECK(o.enter(A) == 0 && g_made[2] == 1);                        // the event is kept
    CHECK(g_slog == SLog({{"record", A, ev, 0}, {"wait", B, ev, 0}, {"record", B, ev, 0}, {"wait", A, ev, 0}}));
    StreamOrder moved(std::move(o));                                 // move-only: the event goes along, once
    CHECK(!(hipEvent_t)o.ev && (hipEvent_t)moved.ev == ev && moved.last == A && moved.has_last);
}

static void order_mark() {
    StreamOrder o;
    CHECK(o.enter(A) == 0 && o.mark(A) == 0 && o.ev_valid);          // the record happens at the mark ...
    hipEvent_t ev = o.ev;
    CHECK(g_log == Log({"hipEventCreateWithFlags", "hipEventRecord"}) && g_slog == SLog({{"record", A, ev, 0}}));
    CHECK(g_flags == std::vector<unsigned>({hipEventDisableTiming}));
    CHECK(o.enter(B) == 0 && !o.ev_valid);                           // ... and enter only waits
    CHECK(g_slog == SLog({{"record", A, ev, 0}, {"wait", B, ev, 0}}) && count("hipEventRecord") == 1);
    CHECK(o.enter(A) == 0);                                          // the mark is spent: records on B, waits on A
    CHECK(g_slog == SLog({{"record", A, ev, 0}, {"wait", B, ev, 0}, {"record", B, ev, 0}, {"wait", A, ev, 0}}));
    CHECK(g_made[2] == 1 && count("hipGetLastError") == 0);
}

static void order_mark_spent() {
    for (int entered_before = 0; entered_before < 2; ++entered_before) {
        g_slog.clear();
        StreamOrder o;
        if (entered_before) CHECK(o.enter(A) == 0);
        CHECK(o.mark(A) == 0 && o.enter(A) == 0 && !o.ev_valid);     // the same-stream call enqueues new work behind the mark
        hipEvent_t ev = o.ev;
        CHECK(g_slog == SLog({{"record", A, ev, 0}}));
        CHECK(o.enter(B) == 0);                                      // so the switch records again
        CHECK(g_slog == SLog({{"record", A, ev, 0}, {"record", A, ev, 0}, {"wait", B, ev, 0}}));
    }
}

static void order_record_fails() {
    StreamOrder o;
    CHECK(o.enter(A) == 0);
    g_fail_record = 1;                                               // A was destroyed: its work has drained
    CHECK(o.enter(B) == 0 && o.last == B && o.has_last && !o.ev_valid);
    CHECK(g_log == Log({"hipEventCreateWithFlags", "hipEventRecord", "hipGetLastError"}));   // no wait, the sticky error cleared once
    CHECK(g_slog == SLog({{"record", A, (hipEvent_t)o.ev, 0}}));
    g_fail_record = 1;
    CHECK(o.hand_over(A) == 0 && o.last == A && count("hipStreamWaitEvent") == 0 && count("hipGetLastError") == 2);
}

static void order_create_fails() {
    StreamOrder o;
    CHECK(o.enter(A) == 0);
    g_fail_next = 1;
    CHECK(o.enter(B) == 1000 + (int)hipErrorOutOfMemory && g_what == "hipEventCreate(stream order)");
    CHECK(o.last == A && o.has_last && !(hipEvent_t)o.ev && g_slog.empty());   // returned before any state changed
    g_fail_next = 1;
    CHECK(o.hand_over(B) == 1000 + (int)hipErrorOutOfMemory && g_what == "hipEventCreate(refresh order)");
    CHECK(o.last == A && o.has_last && g_slog.empty());
    g_fail_next = 1;
    CHECK(o.mark(A) == 1000 + (int)hipErrorOutOfMemory && g_what == "hipEventCreate(stream order)" && !o.ev_valid);
    CHECK(o.enter(B) == 0 && o.last == B && g_slog.size() == 2);     // and the next call tries again
}

static void order_hand_over() {
    {   // last A, argument B: records on A, waits on B, B adopted; the mark made before no longer shortens the next enter
        StreamOrder o;
        CHECK(o.enter(A) == 0 && o.mark(A) == 0);
        hipEvent_t ev = o.ev;
        CHECK(o.hand_over(B) == 0 && o.last == B && o.has_last && !o.ev_valid);
        CHECK(g_slog == SLog({{"record", A, ev, 0}, {"record", A, ev, 0}, {"wait", B, ev, 0}}));
        CHECK(o.enter(C) == 0);
        CHECK(g_slog == SLog({{"record", A, ev, 0}, {"record", A, ev, 0}, {"wait", B, ev, 0}, {"record", B, ev, 0}, {"wait", C, ev, 0}}));
        CHECK(g_made[2] == 1 && g_flags == std::vector<unsigned>({hipEventDisableTiming}));
    }
    g_slog.clear();
    {   // no last: no call, B adopted
        StreamOrder o;
        CHECK(o.mark(A) == 0);
        hipEvent_t ev = o.ev;
        const size_t calls = g_log.size();
        CHECK(o.hand_over(B) == 0 && g_log.size() == calls && o.last == B && o.has_last && !o.ev_valid);
        CHECK(o.enter(C) == 0);
        CHECK(g_slog == SLog({{"record", A, ev, 0}, {"record", B, ev, 0}, {"wait", C, ev, 0}}));
    }
    g_slog.clear();
    {   // last B: no call
        StreamOrder o;
        CHECK(o.enter(B) == 0 && o.mark(B) == 0);
        hipEvent_t ev = o.ev;
        const size_t calls = g_log.size();
        CHECK(o.hand_over(B) == 0 && g_log.size() == calls && o.last == B && !o.ev_valid);
        CHECK(o.enter(C) == 0);
        CHECK(g_slog == SLog({{"record", B, ev, 0}, {"record", B, ev, 0}, {"wait", C, ev, 0}}));
    }
    {   // a scene that was never used: nothing is created
        StreamOrder o;
        const long made = g_made[2];
        CHECK(o.hand_over(A) == 0 && o.hand_over(A) == 0 && g_made[2] == made && o.last == A);
    }
}

// ------------------------------------------------------------------ StreamBlocks: one block per (device, stream)
struct CountingMutex {
    int locks = 0, unlocks = 0;
    void lock() { CHECK(locks == unlocks); ++locks; }
    void unlock() { ++unlocks; CHECK(locks == unlocks); }
};
static StreamBlocks<CountingMutex> g_blocks{"alloc site", "zero site"};   // a global, as in the library: its slots stay reachable

static void blocks() {
    void *a = nullptr, *a2 = nullptr, *b = nullptr;
    CHECK(g_blocks.get(A, 100, 100, &a) == 0 && a && g_dev.count(a));
    CHECK(g_log == Log({"hipGetDevice", "hipMalloc", "hipMemsetAsync"}) && g_slog == SLog({{"zero", A, a, 100}}));
    CHECK(g_blocks.get(A, 100, 100, &a2) == 0 && a2 == a);             // the same (device, stream): the same block, no fill
    CHECK(g_log == Log({"hipGetDevice", "hipMalloc", "hipMemsetAsync", "hipGetDevice"}));
    CHECK(g_blocks.get(B, 100, 100, &b) == 0 && b != a && g_dev.size() == 2);   // a second stream: a second block, filled on B
    CHECK(g_slog == SLog({{"zero", A, a, 100}, {"zero", B, b, 100}}) && count("hipMalloc") == 2);
    size_t at = g_log.size();
    CHECK(g_blocks.get(A, 300, 16, &a2) == 0 && g_dev.count(a2) && !g_dev.count(a) && g_dev.size() == 2);   // grows: frees, then allocates
    CHECK(Log(g_log.begin() + at, g_log.end()) == Log({"hipGetDevice", "hipFree", "hipMalloc", "hipMemsetAsync"}));
    CHECK(g_slog.size() == 3 && g_slog.back() == StreamCall({"zero", A, a2, 16}));                   // only the head is zeroed
    a = a2;
    at = g_log.size();
    CHECK(g_blocks.get(A, 50, 16, &a2) == 0 && a2 == a && g_blocks.get(A, 300, 16, &a2) == 0 && a2 == a);   // grows only
    CHECK(g_log.size() == at + 2 && count("hipMalloc") == 3);
    g_device = 1;                                                    // the same stream handle on another device
    void* d1 = nullptr;
    CHECK(g_blocks.get(A, 100, 100, &d1) == 0 && d1 != a && d1 != b && g_dev.size() == 3);
    g_device = 0;
    CHECK(g_blocks.get(A, 100, 100, &a2) == 0 && a2 == a && g_dev.size() == 3);
    // a zero fill that fails: the new block is freed, the slot stays empty and the next request allocates afresh
    void* c = nullptr;
    at = g_log.size();
    g_fail_memset = 1;
    CHECK(g_blocks.get(C, 64, 64, &c) == 1000 + (int)hipErrorInvalidValue && g_what == "zero site" && !c && g_dev.size() == 3);
    CHECK(Log(g_log.begin() + at, g_log.end()) == Log({"hipGetDevice", "hipMalloc", "hipMemsetAsync", "hipFree"}));
    at = g_log.size();
    CHECK(g_blocks.get(C, 64, 64, &c) == 0 && c && g_dev.size() == 4);
    CHECK(Log(g_log.begin() + at, g_log.end()) == Log({"hipGetDevice", "hipMalloc", "hipMemsetAsync"}));
    g_fail_memset = 1;                                               // ... also when it was growing: the old block is gone too
    CHECK(g_blocks.get(C, 128, 64, &a2) != 0 && !g_dev.count(c) && g_dev.size() == 3);
    CHECK(g_blocks.get(C, 128, 64, &c) == 0 && g_dev.size() == 4);
    g_fail_next = 1;                                                 // an allocation that fails
    void* d = nullptr;
    CHECK(g_blocks.get((hipStream_t)0x40, 8, 8, &d) == 1000 + (int)hipErrorOutOfMemory && g_what == "alloc site" && !d);
    CHECK(g_blocks.get((hipStream_t)0x40, 8, 8, &d) == 0 && d && g_dev.size() == 5);
    CHECK(g_blocks.mu.locks == count("hipGetDevice") && g_blocks.mu.unlocks == g_blocks.mu.locks);
    // never freed, on purpose: the books are squared by hand
    CHECK(g_made[0] - g_gone[0] == 5);
    for (void* p : g_dev) { free(p); ++g_gone[0]; }
    g_dev.clear();
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string which = argv[1];
    if (which == "scope_exit") scope_exit();
    else if (which == "moves") moves();
    else if (which == "reserve") reserve();
    else if (which == "stage") stage();
    else if (which == "lazy") lazy();
    else if (which == "release_then_destructor") release_then_destructor();
    else if (which == "order_enter") order_enter();
    else if (which == "order_mark") order_mark();
    else if (which == "order_mark_spent") order_mark_spent();
    else if (which == "order_record_fails") order_record_fails();
    else if (which == "order_create_fails") order_create_fails();
    else if (which == "order_hand_over") order_hand_over();
    else if (which == "blocks") blocks();
    else return 3;
    CHECK(balanced());   // whatever the case left in scope is gone by now or was never made
    printf("ok\n");
    return 0;
}
"""

CASES = ["scope_exit", "moves", "reserve", "stage", "lazy", "release_then_destructor",
         "order_enter", "order_mark", "order_mark_spent", "order_record_fails", "order_create_fails", "order_hand_over", "blocks"]


@pytest.fixture(scope="module")
def handles(tmp_path_factory):
    """-> run(case): runs one case of the program; the program checks and says where it failed."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    tmp = tmp_path_factory.mktemp("dev_resource_host")
    src, exe = tmp / "host.cpp", tmp / "host"
    src.write_text(HOST_MAIN)
    # the sanitizer runtimes are linked statically: they sit inside the program, which runs in the environment as it is
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I", CSRC,
                         "-isystem", ROCM_INCLUDE, str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr

    def run(case):
        out = subprocess.run([str(exe), case], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.endswith("ok\n"), (out.returncode, out.stdout, out.stderr[-2000:])
    return run


def test_header_needs_only_the_hip_runtime_api():
    with open(os.path.join(CSRC, "dev_resource.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>", "<string>", "<utility>"]


@pytest.mark.parametrize("case", CASES)
def test_handles(handles, case):
    """scope_exit: every create is matched by exactly one destroy at scope exit.  moves: no double free after a move or after a
    std::vector of handles (the timing events, the Adam ring, the weight allocations) grew past its capacity, each resource freed
    exactly once.  reserve: DevBuf::reserve makes no call when need <= bytes, frees before it allocates when growing, and after
    a failed hipMalloc returns the error with p == nullptr and bytes == 0.  stage: PinnedStage::prepare waits on the event only
    while a copy is pending, regrows to twice the request, and a second prepare with no upload in between waits for nothing.
    lazy: Event / Stream ensure() creates once and passes the flags through.  release_then_destructor: frees once."""
    handles(case)
