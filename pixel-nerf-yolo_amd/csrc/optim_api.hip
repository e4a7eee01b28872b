// C ABI of the optimizer (include/pnyolo.h pny_optim_*): the tables of optim.hip's Adam launch and the chained weight refresh.
// Host-side C++; the arithmetic is in optim.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "api_internal.h"

using namespace pny;

// The gradient pointers of one launch: host-pinned, read by the kernel itself (no copy command on the stream).  A table belongs
// to its launch until `ev` has passed; the next step takes another one of the ring, so nothing waits for the device.
struct AdamGradTable {
    PinnedBuf host;   // float* per tensor of the launch
    Event ev;
    bool pending = false;
    float** ptrs() const { return static_cast<float**>(host.p); }
};

struct pny_optim {
    int device = 0;
    std::vector<AdamTensor> tensors;
    std::vector<int> chunk_begin;   // first chunk of tensor i; [size] = number of chunks
    DevBuf tensors_dev, chunks_dev;
    bool tables_ready = false;
    std::vector<AdamGradTable> ring;
    size_t next = 0;
};

static const size_t ADAM_RING_MAX = 64;

// Tensor and chunk tables, once per set of tensors (the first step, and the first step after a tensor was added: the old
// tables may still be read by a launch in flight, which DevBuf::reserve's hipFree waits for).
static int build_tables(pny_optim* o) {
    std::vector<AdamChunk> chunks;
    o->chunk_begin.assign(o->tensors.size() + 1, 0);
    for (size_t i = 0; i < o->tensors.size(); ++i) {
        o->chunk_begin[i] = (int)chunks.size();
        for (long long off = 0; off < o->tensors[i].count; off += ADAM_CHUNK) {
            const long long left = o->tensors[i].count - off;
            chunks.push_back({(int)i, (int)(left < ADAM_CHUNK ? left : ADAM_CHUNK), off});
        }
    }
    o->chunk_begin[o->tensors.size()] = (int)chunks.size();
    int rc;
    o->tensors_dev.release();
    o->chunks_dev.release();
    if ((rc = o->tensors_dev.reserve(std::max<size_t>(o->tensors.size(), 1) * sizeof(AdamTensor)))) return rc;
    if ((rc = o->chunks_dev.reserve(std::max<size_t>(chunks.size(), 1) * sizeof(AdamChunk)))) return rc;
    PNY_HIP(hipMemcpy(o->tensors_dev.p, o->tensors.data(), o->tensors.size() * sizeof(AdamTensor), hipMemcpyHostToDevice));
    PNY_HIP(hipMemcpy(o->chunks_dev.p, chunks.data(), chunks.size() * sizeof(AdamChunk), hipMemcpyHostToDevice));
    o->tables_ready = true;
    return 0;
}

// A table no launch reads any more: the next one of the ring whose event has passed, else a new one; only with ADAM_RING_MAX
// launches outstanding (a host that far ahead of the device) does it wait for the oldest.
static int free_table(pny_optim* o, size_t need, AdamGradTable** out) {
    AdamGradTable* t = nullptr;
    for (size_t k = 0; k < o->ring.size() && !t; ++k) {
        AdamGradTable& c = o->ring[(o->next + k) % o->ring.size()];
        if (c.pending) {
            if (hipEventQuery(c.ev) != hipSuccess) {
                (void)hipGetLastError();
                continue;
            }
            c.pending = false;
        }
        t = &c;
        o->next = (o->next + k + 1) % o->ring.size();
    }
    if (!t && o->ring.size() < ADAM_RING_MAX) {
        o->ring.emplace_back();
        t = &o->ring.back();
        o->next = 0;
    }
    if (!t) {
        t = &o->ring[o->next];
        o->next = (o->next + 1) % o->ring.size();
        PNY_HIP(hipEventSynchronize(t->ev));
        t->pending = false;
    }
    if (int rc = t->ev.ensure(hipEventDisableTiming, "hipEventCreate(gradient table)")) return rc;
    if (int rc = t->host.reserve(need * sizeof(float*), "hipHostMalloc(gradient table)")) return rc;
    *out = t;
    return 0;
}

extern "C" {

int pny_optim_create(pny_optim** out, int device) {
    if (!out) return fail(PNY_ERR_ARG, "pny_optim_create: null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PNY_ERR_NOGPU, "pny_optim_create: no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(PNY_ERR_ARG, "pny_optim_create: device ordinal out of range");
    pny_optim* o = new pny_optim();
    o->device = device;
    *out = o;
    return PNY_OK;
}

void pny_optim_destroy(pny_optim* o) {
    if (!o) return;
    drain_device(o->device);
    delete o;
}

int pny_optim_add_tensor(pny_optim* o, float* param_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t count) {
    if (!o || count < 0 || (count > 0 && (!param_dev || !exp_avg_dev || !exp_avg_sq_dev)))
        return fail(PNY_ERR_ARG, "pny_optim_add_tensor: bad argument");
    if ((reinterpret_cast<uintptr_t>(param_dev) | reinterpret_cast<uintptr_t>(exp_avg_dev) | reinterpret_cast<uintptr_t>(exp_avg_sq_dev)) & 3)
        return fail(PNY_ERR_ARG, "pny_optim_add_tensor: pointers must be 4-byte aligned");
    if (o->tensors.size() >= (size_t)1 << 24) return fail(PNY_ERR_ARG, "pny_optim_add_tensor: too many tensors");
    o->tensors.push_back({param_dev, exp_avg_dev, exp_avg_sq_dev, (long long)count});
    o->tables_ready = false;
    return (int)o->tensors.size() - 1;
}

int pny_optim_adam_step(pny_optim* o, const pny_adam_hyper* h, float* const* grads_dev, int first, int n, pny_model* model,
                        pny_stream stream) {
    if (!o || !h || !grads_dev) return fail(PNY_ERR_ARG, "pny_optim_adam_step: null argument");
    if (first < 0 || n < 1 || (size_t)first + (size_t)n > o->tensors.size())
        return fail(PNY_ERR_ARG, "pny_optim_adam_step: tensor range outside the optimizer's tensors");
    if (h->step < 1) return fail(PNY_ERR_ARG, "pny_optim_adam_step: step must be >= 1");
    if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0) || !(h->eps >= 0.0) || !(h->lr >= 0.0) ||
        !(h->weight_decay >= 0.0))
        return fail(PNY_ERR_ARG, "pny_optim_adam_step: lr, eps, weight_decay must be >= 0 and the betas in [0, 1)");
    if (model && model->desc.device != o->device) return fail(PNY_ERR_ARG, "pny_optim_adam_step: the model lives on another device");
    for (int i = 0; i < n; ++i)
        if (reinterpret_cast<uintptr_t>(grads_dev[i]) & 3) return fail(PNY_ERR_ARG, "pny_optim_adam_step: gradient pointers must be 4-byte aligned");
    PNY_HIP(hipSetDevice(o->device));
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (!o->tables_ready && (rc = build_tables(o))) return rc;
    const int c0 = o->chunk_begin[first], c1 = o->chunk_begin[first + n];
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || (grads_dev[i] != nullptr && o->tensors[first + i].count > 0);
    if (any && c1 > c0) {
        AdamGradTable* t = nullptr;
        if ((rc = free_table(o, (size_t)n, &t))) return rc;
        for (int i = 0; i < n; ++i) t->ptrs()[i] = grads_dev[i];
        // torch.optim.Adam's scalars (_single_tensor_adam), in double; each reaches the kernel rounded to fp32 once
        const double bc1 = 1.0 - std::pow(h->beta1, (double)h->step), bc2 = 1.0 - std::pow(h->beta2, (double)h->step);
        AdamScalars sc;
        sc.step_size = (float)(h->lr / bc1);
        sc.one_minus_beta1 = (float)(1.0 - h->beta1);
        sc.beta2 = (float)h->beta2;
        sc.one_minus_beta2 = (float)(1.0 - h->beta2);
        sc.bc2_sqrt = (float)std::sqrt(bc2);
        sc.eps = (float)h->eps;
        sc.weight_decay = (float)h->weight_decay;
        launch_adam(reinterpret_cast<const AdamTensor*>(o->tensors_dev.p), reinterpret_cast<const AdamChunk*>(o->chunks_dev.p) + c0,
                    c1 - c0, t->ptrs(), first, sc, st);
        PNY_HIP(hipGetLastError());
        PNY_HIP(hipEventRecord(t->ev, st));
        t->pending = true;
    }
    // the packed operands of `model` rebuilt behind the update, on the same stream: a weight the step moved out of the f16
    // range is reported (PNY_RANGE_WEIGHT) by the step that moved it
    if (model) return pny_model_refresh(model, stream);
    return PNY_OK;
}

}  // extern "C"
