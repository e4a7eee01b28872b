// C entry points of the NaN / Inf monitor (include/pnyolo.h pny_finite_*; kernels in finite.hip): argument checks, the
// registered table and its device copy, one launch per check.
#include <vector>

#include "api_internal.h"
#include "pny_finite.h"

using namespace pny;

// The registered table.  `host` is the truth; `table` holds the same entries on the device, brought up to date by
// pny_finite_add_tensor itself (on a stream of the handle's own, so that registration does not wait for the caller's queued
// work), so that a check is a launch and nothing else.
struct pny_finite {
    int device = 0;
    std::vector<FiniteEntry> host;
    long long chunks = 0;       // chunks of all entries
    DevBuf table;
    size_t cap = 0;             // entries the device table has room for
    Stream copy_stream;
};

static const long long FINITE_MAX_CHUNKS = INT32_MAX;

static long long chunks_of(long long count) { return (count + FINITE_CHUNK - 1) / FINITE_CHUNK; }

static int check_flags(const int32_t* flags_dev, const std::string& who) {
    if (!flags_dev || (reinterpret_cast<uintptr_t>(flags_dev) & 3)) return fail(PNY_ERR_ARG, who + "flags_dev is NULL or not 4-byte aligned");
    return 0;
}

static int check_tensor(const float* p, int64_t count, int group, const std::string& who) {
    if (count < 0 || group < 0) return fail(PNY_ERR_ARG, who + "negative count or group");
    if (count > 0 && !p) return fail(PNY_ERR_ARG, who + "NULL tensor with a count > 0");
    if (reinterpret_cast<uintptr_t>(p) & 3) return fail(PNY_ERR_ARG, who + "tensors must be 4-byte aligned");
    return 0;
}

extern "C" {

int pny_finite_create(pny_finite** out, int device) {
    if (!out) return fail(PNY_ERR_ARG, "pny_finite_create: null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PNY_ERR_NOGPU, "pny_finite_create: no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(PNY_ERR_ARG, "pny_finite_create: device ordinal out of range");
    pny_finite* f = new pny_finite();
    f->device = device;
    *out = f;
    return PNY_OK;
}

void pny_finite_destroy(pny_finite* f) {
    if (!f) return;
    drain_device(f->device);
    delete f;
}

int pny_finite_add_tensor(pny_finite* f, const float* dev, int64_t count, int group) {
    const std::string who = "pny_finite_add_tensor: ";
    if (!f) return fail(PNY_ERR_ARG, who + "null handle");
    int rc;
    if ((rc = check_tensor(dev, count, group, who))) return rc;
    if (f->host.size() >= (size_t)1 << 24 || f->chunks + chunks_of(count) > FINITE_MAX_CHUNKS)
        return fail(PNY_ERR_ARG, who + "table full");
    PNY_HIP(hipSetDevice(f->device));
    if ((rc = f->copy_stream.ensure(hipStreamNonBlocking, "hipStreamCreate(table copy)"))) return rc;
    const FiniteEntry e = {dev, (long long)count, group, (int)f->chunks};
    const size_t i = f->host.size();
    f->host.push_back(e);
    size_t first = i;
    if (i + 1 > f->cap) {   // grow (hipFree of the old table waits for the launches that read it), then copy every entry
        const size_t cap = f->cap ? 2 * f->cap : 64;
        if ((rc = f->table.reserve(cap * sizeof(FiniteEntry)))) {   // the old table is gone: the handle is empty again
            f->host.clear();
            f->chunks = 0;
            f->cap = 0;
            return rc;
        }
        f->cap = cap;
        first = 0;
    }
    hipError_t err = hipMemcpyAsync(reinterpret_cast<FiniteEntry*>(f->table.p) + first, f->host.data() + first,
                                    (i + 1 - first) * sizeof(FiniteEntry), hipMemcpyHostToDevice, f->copy_stream);
    if (err == hipSuccess) err = hipStreamSynchronize(f->copy_stream);
    if (err != hipSuccess) {
        f->host.pop_back();
        return hip_fail(err, "pny_finite_add_tensor: table copy");
    }
    f->chunks += chunks_of(count);
    return (int)i;
}

int pny_finite_check(pny_finite* f, int first, int n, int32_t* flags_dev, pny_stream stream) {
    const std::string who = "pny_finite_check: ";
    if (!f) return fail(PNY_ERR_ARG, who + "null handle");
    if (first < 0 || n < 0 || (size_t)first + (size_t)n > f->host.size()) return fail(PNY_ERR_ARG, who + "range outside the registered tensors");
    int rc;
    if ((rc = check_flags(flags_dev, who))) return rc;
    if (n == 0) return PNY_OK;
    const long long c0 = f->host[first].chunk0;
    const long long c1 = (size_t)(first + n) < f->host.size() ? f->host[first + n].chunk0 : f->chunks;
    if (c1 == c0) return PNY_OK;   // only empty tensors
    PNY_HIP(hipSetDevice(f->device));
    launch_finite_table(reinterpret_cast<const FiniteEntry*>(f->table.p), first, n, (int)c0, (int)(c1 - c0), flags_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_finite_check_tensors(const float* const* ptrs, const int64_t* counts, const int32_t* groups, int n, int32_t* flags_dev,
                             pny_stream stream) {
    const std::string who = "pny_finite_check_tensors: ";
    if (n < 0 || n > PNY_FINITE_MAX_IMMEDIATE) return fail(PNY_ERR_ARG, who + "n must be 0 .. 8 (register larger sets: pny_finite_add_tensor)");
    if (n > 0 && (!ptrs || !counts || !groups)) return fail(PNY_ERR_ARG, who + "null argument");
    int rc;
    if ((rc = check_flags(flags_dev, who))) return rc;
    FiniteImmediate t;
    long long chunks = 0;
    for (int i = 0; i < PNY_FINITE_MAX_IMMEDIATE; ++i) {
        if (i < n) {
            if ((rc = check_tensor(ptrs[i], counts[i], groups[i], who))) return rc;
            if (chunks + chunks_of(counts[i]) > FINITE_MAX_CHUNKS) return fail(PNY_ERR_ARG, who + "too many elements for one launch");
            t.e[i] = {ptrs[i], (long long)counts[i], groups[i], (int)chunks};
            chunks += chunks_of(counts[i]);
        } else {
            t.e[i] = {nullptr, 0, 0, (int)chunks};
        }
    }
    if (chunks == 0) return PNY_OK;   // nothing to scan
    launch_finite_immediate(t, n, (int)chunks, flags_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_finite_reset(int32_t* flags_dev, int n_groups, pny_stream stream) {
    const std::string who = "pny_finite_reset: ";
    if (n_groups < 0) return fail(PNY_ERR_ARG, who + "negative n_groups");
    int rc;
    if ((rc = check_flags(flags_dev, who))) return rc;
    if (n_groups == 0) return PNY_OK;
    launch_finite_reset(flags_dev, n_groups, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
