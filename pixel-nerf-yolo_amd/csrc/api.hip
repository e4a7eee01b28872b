// C ABI of libpnyolo.so (include/pnyolo.h): handles, weight packing, per-scene state and the
// launch sequences of a query / render call.  Host-side C++; all arithmetic of the hot path is
// in the kernels (mlp.hip, render_kernels.hip, encoder.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "api_internal.h"

namespace pny {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t e, const char* what) {
    g_err = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what;
    return PNY_ERR_HIP;
}
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace pny

using namespace pny;

// A scene's state (latent, projected maps, workspace, cross-view slab) is written and read by the kernels of
// successive calls without any host synchronisation, which is only ordered if those calls share a stream.  When a
// call arrives on a DIFFERENT stream than the previous call on the same scene, the new stream is made to wait for
// everything the previous call enqueued (one event record + one stream wait, paid only on a stream switch).
namespace pny {
int enter_stream(pny_scene* s, hipStream_t st) {
    if (s->has_last_stream && s->last_stream != st) {
        if (int rc = s->order_ev.ensure(hipEventDisableTiming, "hipEventCreate(stream order)")) return rc;
        if (s->order_ev_valid) {   // recorded right behind the previous call's work (mark_stream_point)
            PNY_HIP(hipStreamWaitEvent(st, s->order_ev, 0));
        } else if (hipEventRecord(s->order_ev, s->last_stream) == hipSuccess) {
            PNY_HIP(hipStreamWaitEvent(st, s->order_ev, 0));
        } else {
            (void)hipGetLastError();  // the previous stream no longer exists: its work has drained
        }
    }
    s->order_ev_valid = false;   // the call that enters enqueues new work
    s->last_stream = st;
    s->has_last_stream = true;
    return 0;
}
// Records the scene's order event NOW, behind the work just enqueued on its stream: a later call on another stream then waits
// for exactly this point and not for whatever else the first stream has been given in between (pny_scenes_encode: the scenes
// of a super-batch are encoded on one stream and rendered on one stream each).
int mark_stream_point(pny_scene* s, hipStream_t st) {
    if (int rc = s->order_ev.ensure(hipEventDisableTiming, "hipEventCreate(stream order)")) return rc;
    PNY_HIP(hipEventRecord(s->order_ev, st));
    s->order_ev_valid = true;
    return 0;
}
}  // namespace pny

// ---------------------------------------------------------------------------------- packed weights
// The operand layouts are pack.hip's: this file lays the images out in one allocation and lists, per image, the job that
// builds it from the state_dict tensor(s) it comes from (RepackEntry).  pny_model_finalize runs the jobs on uploaded copies
// of the tensors, pny_model_refresh on the live parameters.

// 16-byte elements a job of `kind` writes (PackJob::count); PACK_COPY / PACK_ADD2 count floats.  An image is 4 floats per element.
static int pack_count(int kind, int n_out, int k_in, int k_pad, int count) {
    if (kind == PACK_A || kind == PACK_NT || kind == PACK_H2) return (n_out / 32) * (k_pad / 8) * 64;
    if (kind == PACK_AT || kind == PACK_H2T) return (k_in / 32) * (k_pad / 8) * 64;   // the matrix is W^T: k_in rows, K = n_out padded
    if (kind == PACK_NTT) return (n_out / 32) * (k_in / 8) * 64;
    if (kind == PACK_H1) return (k_pad / 16) * (n_out / 32) * 64;
    if (kind == PACK_H2O) return (k_pad / 16) * (n_out > 32 ? 2 : 1) * 2 * 64;
    return count;
}

static const HostTensor* find(const pny_model* m, const std::string& name) {
    auto it = m->host.find(name);
    return it == m->host.end() ? nullptr : &it->second;
}

static int need(const pny_model* m, const std::string& name, std::vector<int64_t> shape, const HostTensor** out) {
    const HostTensor* t = find(m, name);
    if (!t) return fail(PNY_ERR_STATE, "missing weight tensor '" + name + "'");
    if (t->shape != shape) return fail(PNY_ERR_ARG, "weight tensor '" + name + "' has an unexpected shape");
    *out = t;
    return 0;
}

struct PackPlan {
    size_t floats = 0;                                  // size of the packed allocation so far
    std::vector<std::pair<const float**, size_t>> fix;  // pointer slot -> float offset in it
    size_t reserve(size_t n) {
        floats = (floats + 15) / 16 * 16;   // keep every sub-buffer 64-byte aligned
        const size_t off = floats;
        floats += n;
        return off;
    }
};

// Lays out the images of one MLP: validates the tensors, appends one RepackEntry per image to m->repack and records where
// each pointer of `w` / `wt` will point.  No bytes are produced here.
static int pack_mlp(pny_model* m, const std::string& pre, MlpWeights& w, MlpWeightsT& wt, PackPlan& plan) {
    const pny_model_desc& d = m->desc;
    const int d_in = pny::d_in(d), nvb = view_blocks(d);
    const HostTensor* t = nullptr;
    int rc;
    // one image of tensor `name` (`shape`: (n_out, k_in) of a matrix kind); PACK_COPY / PACK_ADD2 keep the tensor's own order
    auto add = [&](int kind, const std::string& name, const std::string& name2, std::vector<int64_t> shape, int k_pad,
                   const float** slot) -> int {
        const HostTensor* t2 = nullptr;
        if ((rc = need(m, name, shape, &t))) return rc;
        if (!name2.empty() && (rc = need(m, name2, shape, &t2))) return rc;
        const bool plain = kind == PACK_COPY || kind == PACK_ADD2;
        RepackEntry e{kind, name, name2, 0, nullptr, 0, 0, 0, 0};
        if (plain) {
            e.count = (int)t->data.size();
        } else {
            e.n_out = (int)shape[0];
            e.k_in = (int)shape[1];
            e.k_pad = k_pad;
        }
        if (kind == PACK_H2 || kind == PACK_H2T || kind == PACK_H2O)
            for (float v : t->data)
                if (!(std::fabs(v) <= 65504.0f)) m->f16_weights_ok = false;   // out of the f16 range (or NaN): AUTO stays on fp32
        e.dst_off = plan.reserve((plain ? 1 : 4) * (size_t)pack_count(kind, e.n_out, e.k_in, e.k_pad, e.count));
        plan.fix.push_back({slot, e.dst_off});
        m->repack.push_back(e);
        return 0;
    };
    // `x = x + lin_z[b](z)` (resnetfc.py:176-182) happens right after lin_in (b = 0) or right after
    // the previous block's fc_1 (b > 0): its bias is folded into that layer's bias here, so the kernel
    // has one bias vector per GEMM chain link and no separate bias pass.
    auto bias_plus = [&](const std::string& name, const std::string& extra, const float** slot) -> int {
        return add(extra.empty() ? PACK_COPY : PACK_ADD2, name, extra, {HID}, 0, slot);
    };
    auto zbias = [&](int b) { return b < nvb ? pre + "lin_z." + std::to_string(b) + ".bias" : std::string(); };
    auto block = [&](int b) { return pre + "blocks." + std::to_string(b); };
    if ((rc = add(PACK_A, pre + "lin_in.weight", "", {HID, d_in}, D_IN_PAD, &w.w_in))) return rc;
    if ((rc = bias_plus(pre + "lin_in.bias", zbias(0), &w.b_in))) return rc;
    for (int b = 0; b < nvb; ++b) {
        const std::string p = pre + "lin_z." + std::to_string(b);
        if ((rc = add(PACK_A, p + ".weight", "", {HID, d.d_latent}, d.d_latent, &w.w_z[b]))) return rc;
        w.b_z[b] = nullptr;  // folded
    }
    for (int b = 0; b < d.n_blocks; ++b) {
        if ((rc = add(PACK_A, block(b) + ".fc_0.weight", "", {HID, HID}, HID, &w.w_fc0[b]))) return rc;
        if ((rc = add(PACK_COPY, block(b) + ".fc_0.bias", "", {HID}, 0, &w.b_fc0[b]))) return rc;
        if ((rc = add(PACK_A, block(b) + ".fc_1.weight", "", {HID, HID}, HID, &w.w_fc1[b]))) return rc;
        if ((rc = bias_plus(block(b) + ".fc_1.bias", zbias(b + 1), &w.b_fc1[b]))) return rc;
    }
    if ((rc = add(PACK_COPY, pre + "lin_out.weight", "", {d.d_out, HID}, 0, &w.w_out))) return rc;
    if ((rc = add(PACK_COPY, pre + "lin_out.bias", "", {d.d_out}, 0, &w.b_out))) return rc;
    // split-f16 images for the f16x2 kernel (mlp_h2.hip)
    if ((rc = add(PACK_H2, pre + "lin_in.weight", "", {HID, d_in}, D_IN_PAD, &wt.h2.in))) return rc;
    for (int b = 0; b < d.n_blocks; ++b) {
        if ((rc = add(PACK_H2, block(b) + ".fc_0.weight", "", {HID, HID}, HID, &wt.h2.fc0[b]))) return rc;
        if ((rc = add(PACK_H2, block(b) + ".fc_1.weight", "", {HID, HID}, HID, &wt.h2.fc1[b]))) return rc;
    }
    // ... and lin_out, its d_out rows padded with zero rows to whole n-tiles (d_out <= 64: pny_model_create)
    if ((rc = add(PACK_H2O, pre + "lin_out.weight", "", {d.d_out, HID}, HID, &wt.h2.out))) return rc;
    // stacked transposed lin_z for the latent gradient (latent_grad.hip): W_cat[c][b * 512 + f] = lin_z[b].weight[f][c], one
    // n-tile-major image of K = nvb * 512 in which block b owns k-iterations [64 b, 64 b + 64) of every n-tile
    wt.wzT_cat = nullptr;
    if (nvb > 0) {
        const int Lc = d.d_latent, Kc = nvb * HID;
        const size_t off = plan.reserve((size_t)Lc * Kc);
        for (int b = 0; b < nvb; ++b) {
            const std::string name = pre + "lin_z." + std::to_string(b) + ".weight";
            if ((rc = need(m, name, {HID, Lc}, &t))) return rc;
            m->repack.push_back({PACK_NTT, name, "", off + (size_t)b * (HID / 8) * 64 * 4, nullptr, Lc, HID, Kc, 0});
        }
        plan.fix.push_back({&wt.wzT_cat, off});
    }
    // transposed images for the backward chain (dX^T = W^T dY^T, mlp_bwd.hip), fp32 and split-f16 (mlp_bwd_h2.hip): W^T is
    // (k_in x n_out), its rows (the GEMM's outputs) must be 512; its K (= n_out) is padded to a ring multiple
    if (d.d_out > D_IN_PAD) return fail(PNY_ERR_ARG, "d_out > 64");
    if ((rc = add(PACK_COPY, pre + "lin_in.weight", "", {HID, d_in}, 0, &wt.w_in_plain))) return rc;
    if ((rc = add(PACK_AT, pre + "lin_out.weight", "", {d.d_out, HID}, D_IN_PAD, &wt.wT_out))) return rc;
    for (int b = 0; b < d.n_blocks; ++b) {
        if ((rc = add(PACK_AT, block(b) + ".fc_0.weight", "", {HID, HID}, HID, &wt.wT_fc0[b]))) return rc;
        if ((rc = add(PACK_AT, block(b) + ".fc_1.weight", "", {HID, HID}, HID, &wt.wT_fc1[b]))) return rc;
    }
    if ((rc = add(PACK_H2T, pre + "lin_out.weight", "", {d.d_out, HID}, D_IN_PAD, &wt.h2.T_out))) return rc;
    for (int b = 0; b < d.n_blocks; ++b) {
        if ((rc = add(PACK_H2T, block(b) + ".fc_0.weight", "", {HID, HID}, HID, &wt.h2.T_fc0[b]))) return rc;
        if ((rc = add(PACK_H2T, block(b) + ".fc_1.weight", "", {HID, HID}, HID, &wt.h2.T_fc1[b]))) return rc;
    }
    return 0;
}

// m->repack -> the job table of one launch_repack; `src` holds the device address of every state_dict tensor by name
static int build_pack_jobs(const pny_model* m, const std::map<std::string, const float*>& src, std::vector<PackJob>& jobs,
                           long long& max_elems) {
    jobs.clear();
    max_elems = 0;
    for (const RepackEntry& e : m->repack) {
        auto it = src.find(e.name);
        if (it == src.end()) return fail(PNY_ERR_STATE, "pny_model_refresh: no device pointer bound for '" + e.name + "'");
        PackJob j;
        memset(&j, 0, sizeof(j));
        j.kind = e.kind;
        j.src = it->second;
        if (!e.name2.empty()) {
            auto it2 = src.find(e.name2);
            if (it2 == src.end()) return fail(PNY_ERR_STATE, "pny_model_refresh: no device pointer bound for '" + e.name2 + "'");
            j.src2 = it2->second;
        }
        j.dst = e.dst_abs ? e.dst_abs : m->packed.f() + e.dst_off;
        j.n_out = e.n_out;
        j.k_in = e.k_in;
        j.k_pad = e.k_pad;
        j.count = pack_count(e.kind, e.n_out, e.k_in, e.k_pad, e.count);
        max_elems = std::max(max_elems, (long long)j.count);
        jobs.push_back(j);
    }
    return 0;
}

// pny_model_finalize: every image of m->repack built by the device packer from copies of the state_dict tensors uploaded
// into `stage`.  Synchronous; `stage` and the job table live for this call only.
static int pack_from_host(pny_model* m) {
    DevBuf stage, table;
    std::map<std::string, size_t> at;   // tensor -> float offset in `stage` (several entries name the same tensor)
    size_t total = 0;
    for (const RepackEntry& e : m->repack)
        for (const std::string* name : {&e.name, &e.name2})
            if (!name->empty() && at.emplace(*name, total).second) total += m->host.at(*name).data.size();
    int rc;
    if ((rc = stage.reserve(total * sizeof(float)))) return rc;
    std::map<std::string, const float*> src;
    for (const auto& kv : at) {
        const std::vector<float>& v = m->host.at(kv.first).data;
        PNY_HIP(hipMemcpy(stage.f() + kv.second, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        src[kv.first] = stage.f() + kv.second;
    }
    std::vector<PackJob> jobs;
    long long max_elems;
    if ((rc = build_pack_jobs(m, src, jobs, max_elems))) return rc;
    if ((rc = table.reserve(jobs.size() * sizeof(PackJob)))) return rc;
    PNY_HIP(hipMemcpy(table.p, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
    // no range word: a weight outside the f16 range at finalize clears f16_weights_ok (pack_mlp) and reports nothing
    launch_repack(reinterpret_cast<const PackJob*>(table.p), (int)jobs.size(), max_elems, nullptr, nullptr);
    PNY_HIP(hipGetLastError());
    PNY_HIP(hipDeviceSynchronize());
    return 0;
}

// Single-plane f16 images for PNY_PRECISION_F16 (mlp_h1.hip): per 16-k step [n-tile][lane] x 8 halves, lane l holding
// f16(W[32 nt + (l & 31)][16 j + 8 (l >> 5) + 0..7]) -- by definition plane 0 of the split image (pack.hip PACK_H2), so they are
// copied out of the split images on the device (pack.hip PACK_H1) and are current whenever those are.  Built once a scene of
// the model is set to F16; from then on every pny_model_finalize rebuilds them and every pny_model_refresh repacks them right
// behind the split images on its stream.  A model that never runs F16 holds no such images and pays nothing for them.
static int build_h1_images(pny_model* m) {
    m->h1_ready = false;
    if (!m->finalized) return 0;   // pny_model_finalize builds them
    PNY_HIP(hipSetDevice(m->desc.device));
    const int nb = m->desc.n_blocks, nmlp = m->desc.has_fine ? 2 : 1;
    // halves: lin_in (K = 64) + 2 nb 512 x 512 layers; the transposed set (F16_TRAIN) is as large (lin_out^T: K = 64)
    const size_t per_mlp = ((size_t)D_IN_PAD + 2ull * nb * HID) * HID * (m->want_h1t ? 2 : 1);
    int rc;
    if ((rc = m->h1_packed.reserve(nmlp * per_mlp * sizeof(_Float16)))) return rc;
    std::vector<PackJob> jobs;
    _Float16* p = reinterpret_cast<_Float16*>(m->h1_packed.p);
    auto add = [&](const float* h2_image, int k_pad, const float** slot) {
        PackJob j;
        memset(&j, 0, sizeof(j));
        j.kind = PACK_H1;
        j.src = h2_image;
        j.dst = reinterpret_cast<float*>(p);
        j.n_out = HID;
        j.k_pad = k_pad;
        j.count = pack_count(PACK_H1, HID, 0, k_pad, 0);
        m->h1_max_elems = std::max(m->h1_max_elems, (long long)j.count);
        jobs.push_back(j);
        *slot = reinterpret_cast<const float*>(p);
        p += (size_t)k_pad * HID;
    };
    m->h1_max_elems = 0;
    for (int f = 0; f < nmlp; ++f) {
        const F16Images& h2 = f16_images(m, f != 0, false);
        F16Images& h1 = m->h1[f];
        h1 = F16Images{};
        h1.base = m->h1_packed.f();
        h1.bytes = m->h1_packed.bytes;
        add(h2.in, D_IN_PAD, &h1.in);
        for (int b = 0; b < nb; ++b) {
            add(h2.fc0[b], HID, &h1.fc0[b]);
            add(h2.fc1[b], HID, &h1.fc1[b]);
        }
    }
    for (int f = 0; f < nmlp && m->want_h1t; ++f) {   // the chain's W^T images: the same [16-k step][n-tile][plane][lane] layout, 512 rows
        const F16Images& h2 = f16_images(m, f != 0, false);
        F16Images& h1 = m->h1[f];
        add(h2.T_out, D_IN_PAD, &h1.T_out);
        for (int b = 0; b < nb; ++b) {
            add(h2.T_fc0[b], HID, &h1.T_fc0[b]);
            add(h2.T_fc1[b], HID, &h1.T_fc1[b]);
        }
    }
    if (nmlp == 1) m->h1[1] = m->h1[0];
    if ((rc = m->h1_jobs.reserve(jobs.size() * sizeof(PackJob)))) return rc;
    // once per model (and finalize): wait for every stream that may still rewrite the split images or read older images
    PNY_HIP(hipDeviceSynchronize());
    PNY_HIP(hipMemcpy(m->h1_jobs.p, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
    m->n_h1_jobs = (int)jobs.size();
    launch_repack(reinterpret_cast<const PackJob*>(m->h1_jobs.p), m->n_h1_jobs, m->h1_max_elems, nullptr, m->range_flag());
    PNY_HIP(hipGetLastError());
    PNY_HIP(hipDeviceSynchronize());
    m->h1_ready = true;
    return 0;
}

namespace pny {
int want_h1_images(pny_model* m, bool transposed) {
    const bool more = transposed && !m->want_h1t;   // (the transposed set joins an existing buffer: rebuild the whole)
    m->want_h1 = true;
    m->want_h1t = m->want_h1t || transposed;
    return (m->h1_ready && !more) ? 0 : build_h1_images(m);
}
}  // namespace pny

// ---------------------------------------------------------------------------------- C ABI
extern "C" {

int pny_version(void) { return PNY_ABI_VERSION; }
const char* pny_last_error(void) { return g_err.c_str(); }

int pny_model_create(pny_model** out, const pny_model_desc* desc) {
    if (!out || !desc) return fail(PNY_ERR_ARG, "pny_model_create: null argument");
    if (desc->d_hidden != HID) return fail(PNY_ERR_ARG, "pny_model_create: d_hidden must be 512");
    if (desc->n_blocks < 1 || desc->n_blocks > MAX_BLOCKS) return fail(PNY_ERR_ARG, "pny_model_create: n_blocks out of range [1,8]");
    if (desc->combine_layer < 0) return fail(PNY_ERR_ARG, "pny_model_create: combine_layer < 0");
    if (desc->d_latent < 128 || desc->d_latent % 128) return fail(PNY_ERR_ARG, "pny_model_create: d_latent must be a positive multiple of 128");
    if (desc->d_out < 1 || desc->d_out > 64) return fail(PNY_ERR_ARG, "pny_model_create: d_out out of range [1,64]");
    if (d_in(*desc) > D_IN_PAD || desc->num_freqs < 0) return fail(PNY_ERR_ARG, "pny_model_create: num_freqs too large (d_in must be <= 64)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PNY_ERR_NOGPU, "pny_model_create: no HIP device visible (this library has no CPU path)");
    if (desc->device < 0 || desc->device >= count) return fail(PNY_ERR_ARG, "pny_model_create: device ordinal out of range");
    PNY_HIP(hipSetDevice(desc->device));
    pny_model* m = new pny_model();
    m->desc = *desc;
    // f16-range guard word (pny_model_range_status): pinned, device-visible host memory; the kernels OR into it
    if (m->range_block.reserve(64)) {
        (void)hipGetLastError();
        delete m;
        return fail(PNY_ERR_HIP, "pny_model_create: hipHostMalloc(range flag) failed");
    }
    *m->range_flag() = 0;
    *out = m;
    return PNY_OK;
}

void pny_model_destroy(pny_model* m) {
    if (!m) return;
    drain_device(m->desc.device);
    trunk_release(m->trunk);
    delete m;
}

int pny_model_load_weights(pny_model* m, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    if (!m || !name || (!data_host && ndim > 0) || ndim < 0 || ndim > 4) return fail(PNY_ERR_ARG, "pny_model_load_weights: bad argument");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) return fail(PNY_ERR_ARG, "pny_model_load_weights: negative dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(data_host, data_host + n);
    m->host[name] = std::move(t);
    m->finalized = false;
    return PNY_OK;
}

int pny_model_finalize(pny_model* m) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_finalize: null model");
    PNY_HIP(hipSetDevice(m->desc.device));
    PackPlan plan;
    int rc;
    m->repack.clear();
    m->repack_ready = false;
    m->h1_ready = false;
    PNY_HIP(hipDeviceSynchronize());  // a re-finalize must not overwrite weights a running kernel reads
    m->f16_weights_ok = true;
    if ((rc = pack_mlp(m, "mlp_coarse.", m->coarse, m->coarse_t, plan))) return rc;
    if (m->desc.has_fine && (rc = pack_mlp(m, "mlp_fine.", m->fine, m->fine_t, plan))) return rc;
    if (plan.floats * sizeof(float) >= (1ull << 31)) return fail(PNY_ERR_ARG, "packed weights exceed the 2 GiB raw-buffer range");
    if ((rc = m->packed.reserve(plan.floats * sizeof(float)))) return rc;
    PNY_HIP(hipMemset(m->packed.p, 0, plan.floats * sizeof(float)));   // the alignment gaps between the images stay zero
    for (auto& f : plan.fix) *f.first = m->packed.f() + f.second;
    for (MlpWeightsT* wt : {&m->coarse_t, &m->fine_t}) {
        wt->h2.base = m->packed.f();
        wt->h2.bytes = m->packed.bytes;
    }
    if (!m->desc.has_fine) {
        m->fine = m->coarse;
        m->fine_t = m->coarse_t;
    }
    // encoder weights are optional (a scene may be fed through pny_scene_set_latent instead)
    // stacked lin_z maps for the projected-latent variant
    m->zproj_allocs.clear();
    m->has_zproj = false;
    {
        const int nvb = view_blocks(m->desc);
        if (nvb > 0) {
            for (int f = 0; f < (m->desc.has_fine ? 2 : 1); ++f) {
                const std::string pre = f ? "mlp_fine." : "mlp_coarse.";
                std::string err;
                if (!build_pixel_linear(nvb, HID, m->desc.d_latent, &m->zproj[f], &m->zproj_allocs, &err))
                    return fail(PNY_ERR_HIP, "latent projection weights: " + err);
                for (int b = 0; b < nvb; ++b)   // stacked along the output rows: block b owns n-tiles [16 b, 16 b + 16)
                    m->repack.push_back({PACK_NT, pre + "lin_z." + std::to_string(b) + ".weight", "", 0,
                                         m->zproj[f].w + (size_t)b * 16 * (m->desc.d_latent / 8) * 64 * 4, HID, m->desc.d_latent,
                                         m->desc.d_latent, 0});
            }
            if (!m->desc.has_fine) m->zproj[1] = m->zproj[0];
            m->has_zproj = true;
        }
    }
    if ((rc = pack_from_host(m))) return rc;
    ++m->generation;
    m->has_encoder = false;
    if (find(m, "encoder.model.conv1.weight")) {
        auto get = [&](const std::string& name, const float** data, std::vector<int64_t>* shape) -> bool {
            const HostTensor* t = find(m, name);
            if (!t) return false;
            *data = t->data.data();
            *shape = t->shape;
            return true;
        };
        std::string err;
        if (!m->enc.build(get, "encoder.model.", &err)) return fail(PNY_ERR_STATE, "encoder weights: " + err);
        m->has_encoder = true;
    }
    m->finalized = true;
    if (m->want_h1 && (rc = build_h1_images(m))) return rc;
    return PNY_OK;
}

int pny_model_bind_param(pny_model* m, const char* name, const float* param_dev) {
    if (!m || !name) return fail(PNY_ERR_ARG, "pny_model_bind_param: null argument");
    if (param_dev)
        m->params_dev[name] = param_dev;
    else
        m->params_dev.erase(name);
    m->repack_ready = false;
    if (strncmp(name, "encoder.model.", 14) == 0) trunk_params_rebound(m->trunk);
    return PNY_OK;
}

int pny_model_refresh(pny_model* m, pny_stream stream) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_refresh: null model");
    if (!m->finalized) return fail(PNY_ERR_STATE, "pny_model_refresh: call pny_model_finalize once first (it lays out the packed weights)");
    PNY_HIP(hipSetDevice(m->desc.device));
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (!m->repack_ready) {   // resolve names -> bound device pointers, upload the job table (once per binding)
        std::vector<PackJob> jobs;
        long long max_elems;
        if ((rc = build_pack_jobs(m, m->params_dev, jobs, max_elems))) return rc;
        const size_t bytes = jobs.size() * sizeof(PackJob);
        if ((rc = m->repack_jobs.reserve(bytes))) return rc;   // (a larger table: hipFree waits for the device)
        // The table is rewritten in place.  The repack launch of an earlier refresh may still be queued on another stream (or on
        // this one) and reads the table when it RUNS: the rewrite is a copy on `st`, ordered behind that launch by its event.  A
        // blocking hipMemcpy would order it behind nothing that runs on a non-blocking stream.
        if (m->repack_ev) PNY_HIP(hipStreamWaitEvent(st, m->repack_ev, 0));
        if ((rc = m->repack_stage.prepare(bytes))) return rc;
        memcpy(m->repack_stage.host.p, jobs.data(), bytes);
        if ((rc = m->repack_stage.upload(m->repack_jobs.p, bytes, st))) return rc;
        m->n_repack_jobs = (int)jobs.size();
        m->repack_max_elems = max_elems;
        m->repack_ready = true;
    }
    // order this stream behind the last call of every scene that may still read the packed weights on another stream
    for (pny_scene* s : m->scenes) {
        if (s->has_last_stream && s->last_stream != st) {
            if ((rc = s->order_ev.ensure(hipEventDisableTiming, "hipEventCreate(refresh order)"))) return rc;
            if (hipEventRecord(s->order_ev, s->last_stream) == hipSuccess)
                PNY_HIP(hipStreamWaitEvent(st, s->order_ev, 0));
            else
                (void)hipGetLastError();
            s->last_stream = st;   // the scene's next call must in turn wait for this refresh
        } else if (!s->has_last_stream) {
            s->last_stream = st;
            s->has_last_stream = true;
        }
        // an order event recorded BEFORE this refresh (mark_stream_point) no longer covers the scene's stream: a later call
        // on another stream has to wait for the repack too, so enter_stream must record a fresh event behind it
        s->order_ev_valid = false;
    }
    launch_repack(reinterpret_cast<const PackJob*>(m->repack_jobs.p), m->n_repack_jobs, m->repack_max_elems, st, m->range_flag());
    if ((rc = m->repack_ev.ensure(hipEventDisableTiming, "hipEventCreate(repack)"))) return rc;
    PNY_HIP(hipEventRecord(m->repack_ev, st));   // the last reader of the job table (see the rewrite above); no host wait
    if (m->h1_ready)  // single-plane images (F16 scenes): copied out of the split images just rewritten, same stream
        launch_repack(reinterpret_cast<const PackJob*>(m->h1_jobs.p), m->n_h1_jobs, m->h1_max_elems, st, m->range_flag());
    PNY_HIP(hipGetLastError());
    ++m->generation;   // projected maps of every scene are stale
    return PNY_OK;
}

int pny_model_use_fine(pny_model* m, int enable) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_use_fine: null model");
    m->use_fine = enable != 0;
    return PNY_OK;
}

int pny_scene_create(pny_scene** out, pny_model* m) {
    if (!out || !m) return fail(PNY_ERR_ARG, "pny_scene_create: null argument");
    pny_scene* s = new pny_scene();
    s->m = m;
    m->scenes.push_back(s);
    if (const char* e = getenv("PNYOLO_PROJECTION")) {  // process-wide default: off | on | auto
        if (!strcmp(e, "off")) s->zp_mode = PNY_PROJECTION_OFF;
        if (!strcmp(e, "on")) s->zp_mode = PNY_PROJECTION_ON;
    }
    if (const char* e = getenv("PNYOLO_MLP_PRECISION")) {  // process-wide default: f32 | f16x2 | f16 | auto
        if (!strcmp(e, "f32")) s->precision = PNY_PRECISION_F32;
        if (!strcmp(e, "f16x2")) s->precision = PNY_PRECISION_F16X2;
        if (!strcmp(e, "f16")) s->precision = PNY_PRECISION_F16;
        if (!strcmp(e, "f16_train")) s->precision = PNY_PRECISION_F16_TRAIN;
    }
    *out = s;
    if (s->precision == PNY_PRECISION_F16 || s->precision == PNY_PRECISION_F16_TRAIN)
        return want_h1_images(m, s->precision == PNY_PRECISION_F16_TRAIN);
    return PNY_OK;
}

void pny_scene_destroy(pny_scene* s) {
    if (!s) return;
    drain_device(s->m->desc.device);   // (a scene always has its model: pny_scene_create refuses a null one)
    auto& v = s->m->scenes;
    v.erase(std::remove(v.begin(), v.end(), s), v.end());
    delete s;
}

int pny_scene_set_cameras(pny_scene* s, const float* poses, int ns, const float* focal, int nf, const float* c, int nc,
                          int width, int height) {
    if (!s || !poses || !focal || !c) return fail(PNY_ERR_ARG, "pny_scene_set_cameras: null argument");
    if (ns < 1 || ns > MAX_VIEWS) return fail(PNY_ERR_ARG, "pny_scene_set_cameras: ns out of range [1,16]");
    if ((nf != 1 && nf != ns) || (nc != 1 && nc != ns)) return fail(PNY_ERR_ARG, "pny_scene_set_cameras: focal / c count must be 1 or ns");
    if (width < 1 || height < 1) return fail(PNY_ERR_ARG, "pny_scene_set_cameras: bad image size");
    for (int v = 0; v < ns; ++v) {
        const float* P = poses + 16 * v;
        Cam& cm = s->cams[v];
        if (!s->m->desc.yolo) {
            // reference models.py:116-118: rot = R^T, trans = -(R^T t) via bmm (fp32)
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) cm.w2c[4 * i + j] = P[4 * j + i];
                float acc = 0.f;
                for (int j = 0; j < 3; ++j) acc += P[4 * j + i] * P[4 * j + 3];
                cm.w2c[4 * i + 3] = -acc;
            }
        } else {
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) cm.w2c[4 * i + j] = P[4 * i + j];
        }
        const float* f = focal + 2 * (nf == 1 ? 0 : v);
        const float* cc = c + 2 * (nc == 1 ? 0 : v);
        cm.fx = f[0];
        cm.fy = s->m->desc.yolo ? f[1] : -f[1];  // models.py:136-137
        cm.cx = cc[0];
        cm.cy = cc[1];
    }
    s->cam_ns = ns;
    s->width = width;
    s->height = height;
    s->have_cams = true;
    s->occ_on = false;   // the grid was learnt on another sigma
    return PNY_OK;
}

int pny_scene_set_groups(pny_scene* s, int n_objs) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_set_groups: null scene");
    if (n_objs < 1 || n_objs > MAX_VIEWS) return fail(PNY_ERR_ARG, "pny_scene_set_groups: n_objs out of range [1,16]");
    s->n_objs = n_objs;   // (the view count is checked against it when a call needs both: check_ready)
    if (n_objs > 1) s->occ_on = false;   // one occupancy grid serves one object
    return PNY_OK;
}

// a new latent is in place: its shape, and the projected maps are stale
static void set_latent_shape(pny_scene* s, int ns, int L, int hl, int wl) {
    s->ns = ns;
    s->L = L;
    s->hl = hl;
    s->wl = wl;
    s->have_latent = true;
    s->zp_valid[0] = s->zp_valid[1] = false;
    s->occ_on = false;   // the grid was learnt on another sigma
}

// what pny_scene_encode and pny_scenes_encode ask of the model and the images; selects the device, returns the latent's size
static int encode_check(const std::string& who, const pny_model* m, int ns, int height, int width, int* hl, int* wl) {
    if (!m->finalized) return fail(PNY_ERR_STATE, who + ": call pny_model_finalize first");
    if (!m->has_encoder) return fail(PNY_ERR_STATE, who + ": no encoder.model.* weights were loaded");
    if (m->desc.d_latent != 512) return fail(PNY_ERR_ARG, who + ": ResNet-34 trunk yields 512 channels; model d_latent differs");
    if (ns < 1 || ns > MAX_VIEWS || height < 32 || width < 32) return fail(PNY_ERR_ARG, who + ": bad shape");
    PNY_HIP(hipSetDevice(m->desc.device));
    encoder_latent_size(height, width, hl, wl);
    if ((long long)*hl * *wl * 512 >= (1ll << 31)) return fail(PNY_ERR_ARG, who + ": latent too large for 32-bit tap offsets");
    return 0;
}

int pny_scene_set_latent(pny_scene* s, const float* latent_dev, int ns, int channels, int hl, int wl, pny_stream stream) {
    if (!s || !latent_dev) return fail(PNY_ERR_ARG, "pny_scene_set_latent: null argument");
    if (channels != s->m->desc.d_latent) return fail(PNY_ERR_ARG, "pny_scene_set_latent: channel count != model d_latent");
    if (ns < 1 || ns > MAX_VIEWS || hl < 1 || wl < 1) return fail(PNY_ERR_ARG, "pny_scene_set_latent: bad shape");
    if ((long long)hl * wl * channels >= (1ll << 31)) return fail(PNY_ERR_ARG, "pny_scene_set_latent: latent too large for 32-bit tap offsets");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    int rc;
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    if ((rc = s->latent.reserve((size_t)ns * channels * hl * wl * sizeof(float)))) return rc;
    launch_nchw_to_nhwc(latent_dev, s->latent.f(), ns, channels, hl * wl, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    set_latent_shape(s, ns, channels, hl, wl);
    return PNY_OK;
}

int pny_scene_set_latent_levels(pny_scene* s, const float* const* maps_dev, const int* channels, const int* h, const int* w, int n_levels,
                                int ns, pny_stream stream) {
    const char* who = "pny_scene_set_latent_levels";
    if (!s) return fail(PNY_ERR_ARG, std::string(who) + ": null argument");
    long long L = 0;
    int rc;
    if ((rc = latent_levels_check(who, maps_dev, channels, h, w, n_levels, ns, &L))) return rc;
    if (L != s->m->desc.d_latent) return fail(PNY_ERR_ARG, std::string(who) + ": channel count != model d_latent");
    if (ns > MAX_VIEWS) return fail(PNY_ERR_ARG, std::string(who) + ": bad shape");
    if ((long long)h[0] * w[0] * L >= (1ll << 31)) return fail(PNY_ERR_ARG, std::string(who) + ": latent too large for 32-bit tap offsets");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    if ((rc = s->latent.reserve((size_t)ns * L * h[0] * w[0] * sizeof(float)))) return rc;
    if ((rc = latent_levels_assemble(who, maps_dev, channels, h, w, n_levels, ns, s->latent.f(), (hipStream_t)stream))) return rc;
    set_latent_shape(s, ns, (int)L, h[0], w[0]);
    return PNY_OK;
}

int pny_scene_encode(pny_scene* s, const float* images_dev, int ns, int height, int width, pny_stream stream) {
    if (!s || !images_dev) return fail(PNY_ERR_ARG, "pny_scene_encode: null argument");
    int hl = 0, wl = 0, rc;
    if ((rc = encode_check("pny_scene_encode", s->m, ns, height, width, &hl, &wl))) return rc;
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    if ((rc = s->latent.reserve((size_t)ns * 512 * hl * wl * sizeof(float)))) return rc;
    const bool pool = s->m->desc.enc_use_first_pool != 0;
    if ((rc = s->enc_work.reserve(encoder_workspace_bytes(ns, height, width, pool)))) return rc;
    std::string err;
    if (!encoder_forward(s->m->enc, images_dev, ns, height, width, pool, s->enc_work.f(), s->latent.f(), (hipStream_t)stream, &err))
        return fail(PNY_ERR_HIP, "pny_scene_encode: " + err);
    set_latent_shape(s, ns, 512, hl, wl);
    return PNY_OK;
}

int pny_scenes_encode(pny_scene** scenes, int n_scenes, const float* images_dev, int ns, int height, int width, pny_stream stream) {
    if (!scenes || n_scenes < 1 || !images_dev) return fail(PNY_ERR_ARG, "pny_scenes_encode: null argument");
    for (int i = 0; i < n_scenes; ++i)
        if (!scenes[i] || scenes[i]->m != scenes[0]->m) return fail(PNY_ERR_ARG, "pny_scenes_encode: scenes must share one model");
    if (n_scenes == 1) return pny_scene_encode(scenes[0], images_dev, ns, height, width, stream);
    pny_model* m = scenes[0]->m;
    int hl = 0, wl = 0, rc;
    if ((rc = encode_check("pny_scenes_encode", m, ns, height, width, &hl, &wl))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t lat_bytes = (size_t)ns * 512 * hl * wl * sizeof(float);
    for (int i = 0; i < n_scenes; ++i) {
        if ((rc = enter_stream(scenes[i], st))) return rc;
        if ((rc = scenes[i]->latent.reserve(lat_bytes))) return rc;
    }
    // ONE pass of the trunk over every scene's images (n_scenes x ns): 41 launches instead of 41 per scene; the images are
    // independent in an eval-mode trunk, so scene i's latent is the i-th slice of the result
    const bool pool = m->desc.enc_use_first_pool != 0;
    const int n_img = n_scenes * ns;
    if ((rc = m->enc_batch_work.reserve(encoder_workspace_bytes(n_img, height, width, pool)))) return rc;
    if ((rc = m->enc_batch_lat.reserve(lat_bytes * (size_t)n_scenes))) return rc;
    std::string err;
    if (!encoder_forward(m->enc, images_dev, n_img, height, width, pool, m->enc_batch_work.f(), m->enc_batch_lat.f(), st, &err))
        return fail(PNY_ERR_HIP, "pny_scenes_encode: " + err);
    for (int i = 0; i < n_scenes; ++i) {
        pny_scene* s = scenes[i];
        PNY_HIP(hipMemcpyAsync(s->latent.p, reinterpret_cast<const char*>(m->enc_batch_lat.p) + lat_bytes * (size_t)i, lat_bytes,
                               hipMemcpyDeviceToDevice, st));
        set_latent_shape(s, ns, 512, hl, wl);
    }
    for (int i = 0; i < n_scenes; ++i)
        if ((rc = mark_stream_point(scenes[i], st))) return rc;
    return PNY_OK;
}

int pny_scene_latent_shape(pny_scene* s, int* ns, int* channels, int* hl, int* wl) {
    if (!s || !s->have_latent) return fail(PNY_ERR_STATE, "pny_scene_latent_shape: no latent");
    if (ns) *ns = s->ns;
    if (channels) *channels = s->L;
    if (hl) *hl = s->hl;
    if (wl) *wl = s->wl;
    return PNY_OK;
}

int pny_scene_get_latent(pny_scene* s, float* latent_dev, pny_stream stream) {
    if (!s || !latent_dev) return fail(PNY_ERR_ARG, "pny_scene_get_latent: null argument");
    if (!s->have_latent) return fail(PNY_ERR_STATE, "pny_scene_get_latent: no latent");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if (int rc = enter_stream(s, (hipStream_t)stream)) return rc;
    launch_nhwc_to_nchw(s->latent.f(), latent_dev, s->ns, s->L, s->hl * s->wl, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

// 3x3 / 4x4 inverses on the host in double precision (reference uses torch.inverse on fp32).
static bool invert4(const float* m, double* inv) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            a[i][j] = m[4 * i + j];
            a[i][4 + j] = (i == j) ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (std::fabs(a[piv][c]) < 1e-30) return false;
        if (piv != c)
            for (int j = 0; j < 8; ++j) std::swap(a[piv][j], a[c][j]);
        const double d = a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] /= d;
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const double f = a[r][c];
                for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j];
            }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv[4 * i + j] = a[i][4 + j];
    return true;
}

int pny_gen_rays_range(const float* poses_host, int b, int width, int height, const float focal[2], const float c[2],
                       float z_near, float z_far, int yolo_mode, int64_t first_ray, int64_t n_rays, float* out_dev,
                       pny_stream stream) {
    if (!poses_host || !focal || !c || (!out_dev && n_rays > 0)) return fail(PNY_ERR_ARG, "pny_gen_rays: null argument");
    if (b < 0 || width < 1 || height < 1) return fail(PNY_ERR_ARG, "pny_gen_rays: bad shape");
    const int64_t total = (int64_t)b * width * height;
    if (first_ray < 0 || n_rays < 0 || first_ray + n_rays > total) return fail(PNY_ERR_ARG, "pny_gen_rays: ray range outside the (b, h, w) grid");
    if (n_rays == 0) return PNY_OK;
    if (reinterpret_cast<uintptr_t>(out_dev) & 15) return fail(PNY_ERR_ARG, "pny_gen_rays: out_dev must be 16-byte aligned");
    std::vector<float> cam((size_t)b * 16);
    for (int i = 0; i < b; ++i) {
        const float* P = poses_host + 16 * i;
        float* o = cam.data() + 16 * i;
        if (!yolo_mode) {
            for (int r = 0; r < 3; ++r) {
                for (int q = 0; q < 3; ++q) o[3 * r + q] = P[4 * r + q];
                o[9 + r] = P[4 * r + 3];
            }
            o[12] = focal[0];
            o[13] = focal[1];
            o[14] = c[0];
            o[15] = c[1];
        } else {
            double inv[16];
            if (!invert4(P, inv)) return fail(PNY_ERR_ARG, "pny_gen_rays: singular extrinsic matrix");
            for (int r = 0; r < 3; ++r) {
                for (int q = 0; q < 3; ++q) o[3 * r + q] = (float)inv[4 * r + q];
                o[9 + r] = (float)inv[4 * r + 3];
            }
            if (focal[0] == 0.f || focal[1] == 0.f) return fail(PNY_ERR_ARG, "pny_gen_rays: zero focal length");
            o[12] = (float)(1.0 / focal[0]);
            o[13] = (float)(1.0 / focal[1]);
            o[14] = (float)(-(double)c[0] / focal[0]);
            o[15] = (float)(-(double)c[1] / focal[1]);
        }
    }
    // the per-image parameter blocks travel as kernel arguments: nothing is staged, allocated or synchronised here
    launch_gen_rays(cam.data(), b, width, height, z_near, z_far, yolo_mode, out_dev, (hipStream_t)stream, first_ray, n_rays);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_gen_rays(const float* poses_host, int b, int width, int height, const float focal[2], const float c[2],
                 float z_near, float z_far, int yolo_mode, float* out_dev, pny_stream stream) {
    if (b < 0 || width < 1 || height < 1) return fail(PNY_ERR_ARG, "pny_gen_rays: bad shape");
    return pny_gen_rays_range(poses_host, b, width, height, focal, c, z_near, z_far, yolo_mode, 0,
                              (int64_t)b * width * height, out_dev, stream);
}

int pny_sample_train_batch(const pny_train_batch_desc* d, const float* images_dev, const float* poses_dev,
                           const float* focal_dev, const float* c_dev, const float* bboxes_dev,
                           const pny_train_batch_draws* draws, float* rays_dev, float* rgb_gt_dev, int32_t* pix_dev,
                           pny_stream stream) {
    const char* who = "pny_sample_train_batch: ";
    if (!d || !images_dev || !poses_dev || !focal_dev || !rays_dev || !rgb_gt_dev)
        return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (d->n_objs < 1 || d->n_views < 1 || d->height < 1 || d->width < 1 || d->n_rays < 1)
        return fail(PNY_ERR_ARG, std::string(who) + "bad shape");
    if ((int64_t)d->n_objs * d->n_rays > INT32_MAX) return fail(PNY_ERR_ARG, std::string(who) + "more than 2^31 - 1 rays");
    // (also what keeps a seeded flat index inside one 32-bit Philox word's reach)
    if ((int64_t)d->n_views * d->height * d->width > (int64_t)UINT32_MAX)
        return fail(PNY_ERR_ARG, std::string(who) + "NV * H * W must be below 2^32");
    if ((d->focal_rows != 1 && d->focal_rows != d->n_objs) || (d->focal_cols != 1 && d->focal_cols != 2))
        return fail(PNY_ERR_ARG, std::string(who) + "focal must be (1 | SB, 1 | 2)");
    if (c_dev && d->c_rows != 1 && d->c_rows != d->n_objs) return fail(PNY_ERR_ARG, std::string(who) + "c must be (1 | SB, 2)");
    if (draws && (bboxes_dev ? (!draws->image_ids_dev || !draws->u_x_dev || !draws->u_y_dev) : !draws->pix_inds_dev))
        return fail(PNY_ERR_ARG, std::string(who) + (bboxes_dev ? "bbox mode replays image_ids_dev, u_x_dev and u_y_dev"
                                                                : "uniform mode replays pix_inds_dev"));
    if (reinterpret_cast<uintptr_t>(rays_dev) & 15) return fail(PNY_ERR_ARG, std::string(who) + "rays_dev must be 16-byte aligned");
    TrainBatchArgs a;
    a.sb = d->n_objs, a.nv = d->n_views, a.h = d->height, a.w = d->width, a.b = d->n_rays;
    a.znear = d->z_near, a.zfar = d->z_far;
    a.focal_rows = d->focal_rows, a.focal_cols = d->focal_cols, a.c_rows = c_dev ? d->c_rows : 1;
    a.seed = d->seed, a.draw_offset = draws ? 0 : d->draw_offset;
    a.images = images_dev, a.poses = poses_dev, a.focal = focal_dev, a.c = c_dev, a.bboxes = bboxes_dev;
    a.pix_inds = draws && !bboxes_dev ? draws->pix_inds_dev : nullptr;
    a.image_ids = draws && bboxes_dev ? draws->image_ids_dev : nullptr;
    a.u_x = draws && bboxes_dev ? draws->u_x_dev : nullptr;
    a.u_y = draws && bboxes_dev ? draws->u_y_dev : nullptr;
    a.rays = rays_dev, a.rgb = rgb_gt_dev, a.pix = pix_dev;
    launch_train_batch(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_train_batch(const pny_yolo_batch_desc* d, const float* poses_host, const int64_t* view_ids_host, const float focal[2],
                         const float c[2], const float* const* targets_dev, float* rays_dev, float* targets_out_dev,
                         int64_t* offsets_host, pny_stream stream) {
    const std::string who = "pny_yolo_train_batch: ";
    if (!d || !offsets_host) return fail(PNY_ERR_ARG, who + "null argument");
    const bool query = !rays_dev && !targets_out_dev;   // size query: offsets_host only
    if (!query && (!poses_host || !view_ids_host || !focal || !c || !targets_dev || !rays_dev || !targets_out_dev))
        return fail(PNY_ERR_ARG, who + "null argument");
    if (d->n_scales < 1 || d->n_scales > PNY_YOLO_BATCH_MAX_SCALES) return fail(PNY_ERR_ARG, who + "n_scales must be 1 .. 4");
    if (d->n_views < 1 || d->n_views > PNY_YOLO_BATCH_MAX_VIEWS)
        return fail(PNY_ERR_ARG, who + "n_views must be 1 .. 16 (one launch carries at most 16 selected cameras)");
    if (d->n_views_all < 1 || d->height < 1 || d->width < 1) return fail(PNY_ERR_ARG, who + "bad shape");
    if (d->n_anchors < 1 || d->n_anchors > 64) return fail(PNY_ERR_ARG, who + "bad shape: n_anchors must be 1 .. 64");
    if ((reinterpret_cast<uintptr_t>(rays_dev) & 15) || (reinterpret_cast<uintptr_t>(targets_out_dev) & 3))
        return fail(PNY_ERR_ARG, who + "rays_dev must be 16-byte aligned (targets_out_dev 4-byte)");
    YoloBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.n_scales = d->n_scales, a.row = d->n_anchors * 6;
    a.znear = d->z_near, a.zfar = d->z_far;
    a.rays = rays_dev, a.targets_out = targets_out_dev;
    if (!query && (focal[0] == 0.f || focal[1] == 0.f)) return fail(PNY_ERR_ARG, who + "zero focal length");
    for (int s = 0; s < d->n_scales; ++s) {
        const int cell = d->cell_sizes[s];
        if (cell < 1 || cell > d->height || cell > d->width)
            return fail(PNY_ERR_ARG, who + "every cell size must be 1 .. min(height, width)");
        a.hs[s] = d->height / cell, a.ws[s] = d->width / cell;
        a.off[s + 1] = a.off[s] + (long long)d->n_views * a.hs[s] * a.ws[s];
        if ((long long)d->n_views_all * a.hs[s] * a.ws[s] > INT32_MAX) return fail(PNY_ERR_ARG, who + "more than 2^31 - 1 cells in a grid");
        if (query) continue;
        if (!targets_dev[s] || (reinterpret_cast<uintptr_t>(targets_dev[s]) & 3)) return fail(PNY_ERR_ARG, who + "null or unaligned target grid");
        a.targets[s] = targets_dev[s];
        // the scale's intrinsics in fp32 (YoloTrainer.py:107-108), then Kinv's entries exactly as pny_gen_rays_range forms them
        const float fx = focal[0] / (float)cell, fy = focal[1] / (float)cell, cx = c[0] / (float)cell, cy = c[1] / (float)cell;
        a.kinv[s][0] = (float)(1.0 / fx);
        a.kinv[s][1] = (float)(1.0 / fy);
        a.kinv[s][2] = (float)(-(double)cx / fx);
        a.kinv[s][3] = (float)(-(double)cy / fy);
    }
    if (a.off[d->n_scales] * a.row > INT32_MAX) return fail(PNY_ERR_ARG, who + "more than 2^31 - 1 target values");
    if (query) {
        for (int s = 0; s <= d->n_scales; ++s) offsets_host[s] = a.off[s];
        return PNY_OK;
    }
    for (int i = 0; i < d->n_views; ++i) {
        const int64_t v = view_ids_host[i];
        if (v < 0 || v >= d->n_views_all) return fail(PNY_ERR_ARG, who + "view id outside [0, n_views_all)");
        double inv[16];
        if (!invert4(poses_host + 16 * v, inv)) return fail(PNY_ERR_ARG, who + "singular extrinsic matrix");
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) a.pose[i][3 * r + q] = (float)inv[4 * r + q];
            a.pose[i][9 + r] = (float)inv[4 * r + 3];
        }
        a.view_id[i] = (int)v;
    }
    for (int s = 0; s <= d->n_scales; ++s) offsets_host[s] = a.off[s];
    launch_yolo_train_batch(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------- MLP launch
namespace pny {
static unsigned range_bits(const pny_model* m) {
    return m->range_flag() ? __atomic_load_n(m->range_flag(), __ATOMIC_RELAXED) : 0u;
}
int check_ready(pny_scene* s, const char* who) {
    if (!s) return fail(PNY_ERR_ARG, std::string(who) + ": null scene");
    if (!s->m->finalized) return fail(PNY_ERR_STATE, std::string(who) + ": weights not finalized (pny_model_finalize)");
    // f16-range guard: scenes pinned to F32 neither cause nor suffer from it (weights beyond the f16 range are legal there)
    const unsigned bits = s->precision == PNY_PRECISION_F32 ? 0u : range_bits(s->m);
    if (bits) {
        if (bits & PNY_RANGE_WEIGHT) s->m->f16_weights_ok = false;   // AUTO scenes run F32 from here on
        return fail(PNY_ERR_RANGE, std::string(who) + ": an earlier f16 (F16X2 / F16) launch left the f16 range (" +
                                       std::string(bits & PNY_RANGE_ACTIVATION ? "activation " : "") +
                                       std::string(bits & PNY_RANGE_GRADIENT ? "gradient " : "") +
                                       std::string(bits & PNY_RANGE_WEIGHT ? "weight " : "") +
                                       "beyond +-65504 or not finite): its results are invalid.  Clear with pny_model_range_status(m, 0, 1), pin "
                                       "pny_scene_set_precision(s, PNY_PRECISION_F32) and repeat the call");
    }
    if (!s->have_latent) return fail(PNY_ERR_STATE, std::string(who) + ": scene has no latent (pny_scene_encode / pny_scene_set_latent)");
    if (!s->have_cams) return fail(PNY_ERR_STATE, std::string(who) + ": scene has no cameras (pny_scene_set_cameras)");
    if (s->cam_ns != s->ns) return fail(PNY_ERR_STATE, std::string(who) + ": camera count != latent view count");
    if (s->n_objs > 1 && s->ns % s->n_objs)
        return fail(PNY_ERR_STATE, std::string(who) + ": grouped scene: the view count is not a multiple of the object count");
    if (obj_views(s) > 1 && s->m->desc.combine_layer >= s->m->desc.n_blocks)
        return fail(PNY_ERR_ARG, std::string(who) + ": multi-view scene needs combine_layer < n_blocks");
    return 0;
}

int view_blocks(const pny_model_desc& d) { return d.combine_layer < d.n_blocks ? d.combine_layer : d.n_blocks; }
}  // namespace pny

namespace pny {
double mlp_flops_per_point(const pny_model_desc& d, int ns, MlpPass pass) {
    const int nvb = view_blocks(d);
    const double per_view = (pass == PASS_CHAIN ? 0.0 : (double)d_in(d) * HID) +
                            (pass == PASS_FORWARD ? (double)nvb * d.d_latent * HID : 0.0) + 2.0 * nvb * HID * HID;
    const double post = 2.0 * (d.n_blocks - nvb) * HID * HID + (double)HID * d.d_out;
    const double once = pass == PASS_FORWARD_VIEW_MEAN ? (double)(ns - 1) * HID * HID : 0.0;   // fc_1 GEMMs that do not run
    return 2.0 * (ns * per_view + post - once);
}
}  // namespace pny

// ---------------------------------------------------------------------------------- routing
// Which kernel an MLP launch runs and on which latent, decided here and nowhere else (run_mlp launches what it says,
// ensure_projection projects when and how it says).  The rules are those of include/pnyolo.h pny_scene_set_precision /
// pny_scene_set_projection:
//   * f16 kernels read the projected latent only, exist for the shapes mlp_h2_supports accepts, and are never taken by a scene
//     pinned to F32.  Weights beyond the f16 range (f16_weights_ok false) keep every scene but one pinned to F16X2 off them.
//   * Single-plane f16 wherever the split kernel would run: no-grad launches of F16 and F16_TRAIN scenes, stashing (training)
//     forwards of F16_TRAIN scenes only -- an F16 scene trains as AUTO, on the split kernel.
//   * A plain launch is projected when the scene's mode says so; AUTO projects every launch of a scene whose launches can run
//     f16 (f16_default below), else launches of at least 2 x hl x wl points.  A stashing forward ignores the mode: it forces
//     the projection when it can run f16 (which there also needs L % 128 == 0), and otherwise runs fp32 on the raw latent.
//   * f16_default differs from "can run f16" in one case, on purpose: an F16X2 scene of a model whose weights left the f16 range
//     runs the split kernel where it is projected, but AUTO projection keeps the 2 x hl x wl threshold and the projection
//     itself stays on the fp32 matrix path.
//   * Split f16 on 32-sample tiles (mlp_h2s.hip: 4-wave workgroups, two per CU, the same arithmetic per sample bit for bit)
//     only for no-grad split-f16 launches of at most 32 x CUs points.  Measured (profiles/r02zk_split_sweep.log): a launch
//     that gives every CU at most ONE 32-sample tile takes 0.40-0.43 ms against 0.47-0.51 ms on 64-sample tiles; as soon as
//     two workgroups share a CU the doubled weight stream per sample costs more than the overlap of their phases returns (full
//     C2 frame: 61.7 vs 39.9 ms per launch).  PNYOLO_H2_SPLIT=0|1 overrides.
//   * PNYOLO_GRID (diagnostic: fewer resident workgroups) caps plain launches only.  Both variables are read at every call.
enum MlpKernel { K_F32_8x64 = MLP_8x64, K_F32_16x64 = MLP_16x64, K_F32_8x32 = MLP_8x32, K_H2, K_H2S, K_H1 };
struct MlpRoute {
    MlpKernel kernel;
    Prec prec;        // its arithmetic
    bool stash;       // STASH instantiation: writes the backward's operands into the model-level reservation
    bool projected;   // reads the projected latent maps
    int tile;         // samples per workgroup tile
    int grid_cap;     // resident workgroups
};

static bool f16_default(const pny_scene* s) {
    const pny_model* m = s->m;
    return s->precision != PNY_PRECISION_F32 && m->f16_weights_ok && mlp_h2_supports(m->desc.n_blocks, m->desc.combine_layer);
}

// whether a launch of n_points reads projected maps (force: whatever the scene's mode says)
static bool wants_projection(const pny_scene* s, long long n_points, bool force) {
    if (!s->m->has_zproj) return false;
    // 32-bit tap offsets, in BYTES in the f16 kernels' wave-owned gather (mlp_h2.hip h2wave_issue: one buffer resource per
    // view's map): a view's map stays under 4 GiB, larger ones stay direct
    if ((long long)s->hl * s->wl * view_blocks(s->m->desc) * HID >= (1ll << 30)) return false;
    if (force) return true;
    if (s->zp_mode == PNY_PROJECTION_OFF) return false;
    return s->zp_mode != PNY_PROJECTION_AUTO || f16_default(s) || n_points >= 2ll * s->hl * s->wl;
}

// stash: a stashing forward was asked for AND the reservation has room for it (otherwise the plain forward runs)
static MlpRoute route_mlp(const pny_scene* s, long long n_points, bool stash) {
    const pny_model_desc& d = s->m->desc;
    const int prec = s->precision;
    const bool can_f16 = prec != PNY_PRECISION_F32 && (s->m->f16_weights_ok || prec == PNY_PRECISION_F16X2) &&
                         mlp_h2_supports(d.n_blocks, d.combine_layer) && (!stash || s->L % 128 == 0);
    MlpRoute r;
    r.stash = stash;
    r.projected = stash ? can_f16 && wants_projection(s, n_points, true) : wants_projection(s, n_points, false);
    const bool f16 = r.projected && can_f16;
    const bool h1 = f16 && (prec == PNY_PRECISION_F16_TRAIN || (prec == PNY_PRECISION_F16 && !stash));
    bool h2s = f16 && !h1 && !stash && n_points <= 32ll * mlp_max_grid(MLP_8x64);
    if (f16 && !h1 && !stash)
        if (const char* e = getenv("PNYOLO_H2_SPLIT")) h2s = atoi(e) != 0;
    const int shape = (f16 || stash) ? MLP_8x64 : mlp_pick_variant(n_points);   // (the STASH instantiations are 8x64)
    r.kernel = h1 ? K_H1 : h2s ? K_H2S : f16 ? K_H2 : MlpKernel(shape);
    r.prec = h1 ? PREC_H1 : f16 ? PREC_H2 : PREC_F32;
    r.tile = h2s ? 32 : mlp_tile_samples(shape);
    r.grid_cap = h2s ? 2 * mlp_max_grid(MLP_8x64) : mlp_max_grid(shape);
    if (!stash)
        if (const char* e = getenv("PNYOLO_GRID")) {
            const int g = atoi(e);
            if (g > 0 && g < r.grid_cap) r.grid_cap = g;
        }
    return r;
}

// Projected latent: zp[v][y][x][b*512 + n] = sum_k lin_z[b].weight[n][k] * latent[v][y][x][k], computed
// once per (scene latent, weights) on the caller's stream and cached.  AUTO (wants_projection): with the f16x2 kernel
// available every launch is projected -- a lone 64-sample tile on it (0.5 ms) beats the 32-sample fp32 shape on the
// unprojected latent (1.0 ms) even with the one-off projection of the scene (0.3 ms per MLP at C2), and a ray's result then
// never depends on the size of the batch it is rendered in.  Without it (F32 scenes, more than 6 blocks): when the launch
// has at least twice as many points as the latent has pixels per view (the projection costs one lin_z per PIXEL instead of
// one per (sample, view); tiny training-size batches on large maps stay direct).
namespace pny {
// The projection itself, for the cache below and for the read-out (pny_scene_projection): MLP `which`'s stacked lin_z applied
// to every pixel of the scene's latent, into out (ns hl wl, view blocks x 512).  Scenes whose projected launches run the f16x2
// kernel project on the split-f16 matrix path too.  route: see run_pixel_linear.
static int project_latent(const pny_scene* s, int which, float* out, hipStream_t st, int* route) {
    const pny_model* m = s->m;
    if (!m->desc.has_fine) which = 0;
    const long long npix = (long long)s->ns * s->hl * s->wl;
    if (!run_pixel_linear(m->zproj[which], s->latent.f(), npix, out, st, f16_default(s), route))
        return fail(PNY_ERR_HIP, "latent projection launch failed");
    return 0;
}

int ensure_projection(pny_scene* s, int which, long long n_points, hipStream_t st, const float** zp, bool force) {
    *zp = nullptr;
    const pny_model* m = s->m;
    if (!wants_projection(s, n_points, force)) return 0;
    const int nvb = view_blocks(m->desc);
    if (s->zp_generation != m->generation) {
        s->zp_valid[0] = s->zp_valid[1] = false;
        s->zp_generation = m->generation;
    }
    if (!m->desc.has_fine) which = 0;
    if (!s->zp_valid[which]) {
        const long long npix = (long long)s->ns * s->hl * s->wl;
        int rc;
        if ((rc = s->zp[which].reserve((size_t)npix * nvb * HID * sizeof(float)))) return rc;
        if ((rc = project_latent(s, which, s->zp[which].f(), st, nullptr))) return rc;
        s->zp_valid[which] = true;
    }
    *zp = s->zp[which].f();
    return 0;
}
}  // namespace pny

namespace pny {
int fill_mlp_args(pny_scene* s, int mode, const float* xyz, const float* dirs, const float* rays, const float* z, int K,
                  long long n_points, int coarse, float* out, MlpArgs* pa) {
    const pny_model_desc& d = s->m->desc;
    MlpArgs& a = *pa;
    memset(&a, 0, sizeof(a));
    const bool fine_w = mlp_index(s->m, coarse) == 1;
    a.w = fine_w ? s->m->fine : s->m->coarse;
    a.n_blocks = d.n_blocks;
    use_images(a, f16_images(s->m, fine_w, false));   // (in the packed blob, like `w`)
    a.range_flag = s->m->range_flag();
    a.latent = s->latent.f();
    a.zp = nullptr;
    a.zp_stride = view_blocks(d) * HID;
    a.tap_stride = s->L;
    memcpy(a.cams, s->cams, sizeof(Cam) * (size_t)s->ns);
    a.xyz = xyz;
    a.dirs = dirs;
    a.rays = rays;
    a.z = z;
    a.out = out;
    a.n_points = n_points;
    a.K = K;
    a.mode = mode;
    a.NS = obj_views(s);
    a.obj_pts = 0;
    if (s->n_objs > 1) {   // grouped scene: equal consecutive shares, whole tiles per object (pny_scene_set_groups)
        if (n_points % s->n_objs || (n_points / s->n_objs) % 64)
            return fail(PNY_ERR_ARG, "grouped scene: every object's share of the samples must be the same multiple of 64");
        a.obj_pts = n_points / s->n_objs;
    }
    a.L = s->L;
    a.Hl = s->hl;
    a.Wl = s->wl;
    a.combine_layer = d.combine_layer;
    a.d_out = d.d_out;
    a.yolo = d.yolo;
    a.num_freqs = d.num_freqs;
    a.freq_factor = d.freq_factor;
    // latent_scaling / image_size in fp32 (reference encoder.py:97,170-172)
    const float lsx = (float)s->wl / ((float)s->wl - 1.0f) * 2.0f;
    const float lsy = (float)s->hl / ((float)s->hl - 1.0f) * 2.0f;
    a.sx = lsx / (float)s->width;
    a.sy = lsy / (float)s->height;
    const long long tiles = (n_points + 63) / 64;
    if (tiles > 0x7fffffffll) return fail(PNY_ERR_ARG, "too many points for one launch");
    a.n_tiles = (int)tiles;
    a.idx32 = (tiles * 64) < 0xffffffffll;
    if (mode == 1 && (reinterpret_cast<uintptr_t>(rays) & 15)) return fail(PNY_ERR_ARG, "rays must be 16-byte aligned");
    int rc;
    if ((rc = s->scratch.reserve(mlp_scratch_floats() * sizeof(float)))) return rc;
    a.scratch = s->scratch.f();
    return 0;
}
}  // namespace pny

// One MLP evaluation of a query / render call.  stash_pass (pny_scene_stash_next_render; 0 coarse, 1 fine pass of the
// render): the training forward -- the STASH instantiation of the routed kernel (64-sample tiles) writes every GEMM operand
// into the tiles this pass takes from the model-level reservation, and the backward of the same reservation epoch then
// starts at the dX chain (the f16 instantiations read the projected latent for the forward and gather the raw latent once more
// per view for lin_z's weight gradient; the same stash layout and contents).  Without room in the reservation the plain
// forward runs and the backward recomputes.
static int run_mlp(pny_scene* s, int mode, const float* xyz, const float* dirs, const float* rays, const float* z,
                   int K, long long n_points, int coarse, float* out, hipStream_t st, int stash_pass = -1) {
    if (n_points == 0) return 0;
    pny_model* m = s->m;
    const pny_model_desc& d = m->desc;
    MlpArgs a;
    int rc;
    if ((rc = fill_mlp_args(s, mode, xyz, dirs, rays, z, K, n_points, coarse, out, &a))) return rc;
    const int which = mlp_index(m, coarse);
    bool room = false;
    if (stash_pass >= 0) {
        s->stashed[stash_pass].valid = false;
        room = m->stash.book.has_room(which, obj_views(s), a.n_tiles);
    }
    const MlpRoute r = route_mlp(s, n_points, room);
    if (r.stash) {
        const StashedPass& sp = s->stashed[stash_pass] = m->stash.book.take_pass(which, a.n_tiles, n_points);
        a.lay = stash_layout(d, obj_views(s), s->L);
        a.stash_x = m->stash.x_record(a.lay, which, sp.tile0);
    }
    if (r.projected) {
        if ((rc = ensure_projection(s, which, n_points, st, &a.zp, r.stash))) return rc;
        a.tap_stride = a.zp_stride;
    }
    if (r.kernel == K_H1) {   // (F16_TRAIN scenes: the same no-grad kernel as F16's, so their no-grad results are F16's bit for bit)
        if ((rc = want_h1_images(m, s->precision == PNY_PRECISION_F16_TRAIN))) return rc;
        use_images(a, f16_images(m, which == 1, true));
    }
    const long long tiles = (n_points + r.tile - 1) / r.tile;
    if (tiles > 0x7fffffffll) return fail(PNY_ERR_ARG, "too many points for one launch");
    a.n_tiles = (int)tiles;
    a.idx32 = (tiles * r.tile) < 0xffffffffll;
    const int grid = (int)std::min<long long>(r.grid_cap, tiles);
    if ((rc = stamp_event(s->timing, s->ev, s->ev_used, st))) return rc;
    switch (r.kernel) {
    case K_H1: (r.stash ? launch_mlp_h1_stash : launch_mlp_h1)(a, grid, st); break;
    case K_H2: (r.stash ? launch_mlp_h2_stash : launch_mlp_h2)(a, grid, st); break;
    case K_H2S: launch_mlp_h2s(a, grid, st); break;
    default:
        if (r.stash)
            launch_mlp_stash(a, grid, st);
        else
            launch_mlp(a, r.kernel, grid, st);
    }
    PNY_HIP(hipGetLastError());
    if ((rc = stamp_event(s->timing, s->ev, s->ev_used, st))) return rc;
    s->last_prec = r.prec;
    s->last_projected = r.projected;
    // executed FLOPs: the non-stashing split-f16 kernels run the last per-view fc_1 once, on the mean over views (mlp_h2.hip)
    const bool view_mean = !r.stash && (r.kernel == K_H2 || r.kernel == K_H2S);
    s->last_flops += mlp_flops_per_point(d, obj_views(s), view_mean ? PASS_FORWARD_VIEW_MEAN : r.projected ? PASS_FORWARD_PROJECTED : PASS_FORWARD) *
                     (double)n_points;
    s->last_flops_ref += mlp_flops_per_point(d, obj_views(s), PASS_FORWARD) * (double)n_points;
    s->last_launches += 1;
    return 0;
}

static void begin_call(pny_scene* s) {
    s->ev_used = 0;
    s->last_flops = 0.0;
    s->last_flops_ref = 0.0;
    s->last_launches = 0;
}

// One MLP pass of a pny_render with an occupancy grid attached (pny_occupancy.h): classify the n x K depth samples, read the
// kept count M (the pass's ONE host wait), gather the kept samples' points into M compact rows, evaluate the MLP on them as a
// point list (pny_query's launch) and expand into `samp` (n, K, 4), a rejected sample getting (0, 0, 0, 0).  M == 0 launches
// no MLP kernel.
static int culled_mlp(pny_scene* s, const float* rays, const float* z, int64_t n, int K, int coarse, float* samp, hipStream_t st,
                      int pass) {
    const int64_t S = n * K;
    if (n > OCC_MAX_SAMPLES / K) return fail(PNY_ERR_ARG, "pny_render: more than 2^30 samples in a pass with an occupancy grid attached");
    if (reinterpret_cast<uintptr_t>(samp) % 16)
        return fail(PNY_ERR_ARG, "pny_render: per-sample buffers must be 16-byte aligned with an occupancy grid attached");
    int rc;
    const OccLayout l = occ_layout(S);
    const size_t o_sums = mc_align((size_t)S * sizeof(int32_t)), o_kept = o_sums + l.bytes;
    if ((rc = s->occ_work.reserve(o_kept + 256, "hipMalloc(occupancy workspace)"))) return rc;
    if ((rc = s->occ_count.reserve(sizeof(int64_t), "hipHostMalloc(occupancy count)"))) return rc;
    char* W = reinterpret_cast<char*>(s->occ_work.p);
    int32_t* slot = reinterpret_cast<int32_t*>(W);
    int64_t* kept_dev = reinterpret_cast<int64_t*>(W + o_kept);
    occupancy_classify(s->occ, rays, z, S, K, slot, kept_dev, W + o_sums, st);
    PNY_HIP(hipGetLastError());
    PNY_HIP(hipMemcpyAsync(s->occ_count.p, kept_dev, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PNY_HIP(hipStreamSynchronize(st));
    const int64_t M = *static_cast<const int64_t*>(s->occ_count.p);
    if (M < 0 || M > S) return fail(PNY_ERR_HIP, "pny_render: the occupancy classification returned an impossible count");
    s->cull_kept[pass] = M, s->cull_total[pass] = S;
    float* outc = nullptr;
    if (M > 0) {
        const size_t m3 = ((size_t)M * 3 + 63) & ~(size_t)63;
        if ((rc = s->occ_rows.reserve((2 * m3 + (size_t)M * 4) * sizeof(float), "hipMalloc(occupancy rows)"))) return rc;
        float* xyz = s->occ_rows.f();
        float* dirs = xyz + m3;
        outc = dirs + m3;
        launch_occupancy_gather(slot, rays, z, S, K, M, xyz, dirs, st);
        PNY_HIP(hipGetLastError());
        if ((rc = run_mlp(s, 0, xyz, dirs, nullptr, nullptr, 1, M, coarse, outc, st))) return rc;
    }
    launch_occupancy_expand(slot, outc, S, M, samp, st);
    PNY_HIP(hipGetLastError());
    return 0;
}

extern "C" {

int pny_query(pny_scene* s, const float* xyz_dev, const float* viewdirs_dev, int64_t n, int coarse, float* out_dev,
              pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_query"))) return rc;
    if (n < 0 || (n > 0 && (!xyz_dev || !viewdirs_dev || !out_dev))) return fail(PNY_ERR_ARG, "pny_query: bad argument");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    begin_call(s);
    return run_mlp(s, 0, xyz_dev, viewdirs_dev, nullptr, nullptr, 1, n, coarse, out_dev, (hipStream_t)stream);
}

int pny_sample_coarse(const float* rays_dev, int64_t n, int n_coarse, int lindisp, const float* u_dev, uint64_t seed,
                      float* z_dev, pny_stream stream) {
    if (n < 0 || n_coarse < 1 || (n > 0 && (!rays_dev || !z_dev))) return fail(PNY_ERR_ARG, "pny_sample_coarse: bad argument");
    launch_sample_coarse(rays_dev, n, n_coarse, lindisp, u_dev, seed, z_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_composite(const float* rays_dev, const float* z_dev, const float* sample_dev, int64_t n, int k, int white_bkgd,
                  float* weights_dev, float* rgb_dev, float* depth_dev, pny_stream stream) {
    if (n < 0 || k < 1 || (n > 0 && (!rays_dev || !z_dev || !sample_dev))) return fail(PNY_ERR_ARG, "pny_composite: bad argument");
    launch_composite(rays_dev, z_dev, sample_dev, n, k, white_bkgd, weights_dev, rgb_dev, depth_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_sample_fine(const float* rays_dev, const float* z_coarse_dev, const float* weights_dev, const float* depth_dev,
                    int64_t n, int n_coarse, int n_fine, int n_fine_depth, float depth_std, int lindisp,
                    const float* u_dev, const float* u2_dev, const float* g_dev, uint64_t seed, float* z_out_dev,
                    pny_stream stream) {
    if (n < 0 || n_coarse < 1 || n_fine < 0 || n_fine_depth < 0 || n_fine_depth > n_fine)
        return fail(PNY_ERR_ARG, "pny_sample_fine: bad sample counts");
    if (n > 0 && (!rays_dev || !z_coarse_dev || !weights_dev || !z_out_dev || (n_fine_depth > 0 && !depth_dev)))
        return fail(PNY_ERR_ARG, "pny_sample_fine: null argument");
    if ((size_t)(4 * n_coarse + 1 + 2 * n_fine) * 4 * sizeof(float) > 160 * 1024)
        return fail(PNY_ERR_ARG, "pny_sample_fine: n_coarse + n_fine too large for the LDS-resident sort");
    launch_sample_fine(rays_dev, z_coarse_dev, weights_dev, depth_dev, n, n_coarse, n_fine, n_fine_depth, depth_std,
                       lindisp, u_dev, u2_dev, g_dev, seed, z_out_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_aggregate(const float* raw_dev, int64_t n, int k, int n_anchors, float* out_dev, pny_stream stream) {
    if (n < 0 || k < 1 || n_anchors < 1 || (n > 0 && (!raw_dev || !out_dev))) return fail(PNY_ERR_ARG, "pny_yolo_aggregate: bad argument");
    launch_yolo_aggregate(raw_dev, n, k, n_anchors, out_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_render(pny_scene* s, const float* rays_dev, int64_t n, const pny_render_opts* o, const pny_render_out* out,
               pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_render"))) return rc;
    if (!o || !out || n < 0 || (n > 0 && !rays_dev)) return fail(PNY_ERR_ARG, "pny_render: bad argument");
    if (s->m->desc.yolo || s->m->desc.d_out != 4) return fail(PNY_ERR_ARG, "pny_render: model is in YOLO mode (use pny_yolo_render)");
    if (o->n_coarse < 1 || o->n_fine < 0 || o->n_fine_depth < 0 || o->n_fine_depth > o->n_fine)
        return fail(PNY_ERR_ARG, "pny_render: bad sample counts");
    const int kimp = o->n_fine - o->n_fine_depth;
    const bool any_u = o->u_coarse_dev || o->u_fine_dev || o->u_fine2_dev || o->g_depth_dev;
    if (any_u) {
        if (!o->u_coarse_dev || (kimp > 0 && (!o->u_fine_dev || !o->u_fine2_dev)) || (o->n_fine_depth > 0 && !o->g_depth_dev))
            return fail(PNY_ERR_ARG, "pny_render: explicit random draws must be given for every stage or for none");
    }
    // an occupancy grid (pny_scene_set_occupancy) is for no-grad renders: a culled pass writes no stash
    const bool cull = s->occ_on;
    if (cull && s->stash_next) {
        s->stash_next = false;
        return fail(PNY_ERR_STATE, "pny_render: the scene has an occupancy grid attached and was told to stash for a backward "
                                   "(pny_scene_stash_next_render); clear the grid with pny_scene_set_occupancy(s, NULL, ...) to train");
    }
    s->cull_kept[0] = s->cull_kept[1] = s->cull_total[0] = s->cull_total[1] = 0;
    if (n == 0) return PNY_OK;
    PNY_HIP(hipSetDevice(s->m->desc.device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = enter_stream(s, st))) return rc;
    begin_call(s);
    const int kc = o->n_coarse, kt = o->n_coarse + o->n_fine;
    // workspace carve (floats): z_c, samp_c, w_c, rgb_c(3)+depth_c, z_f, samp_f
    size_t off = 0;
    auto carve = [&](size_t nfl) {
        size_t r = off;
        off += (nfl + 63) & ~(size_t)63;
        return r;
    };
    const size_t o_zc = carve((size_t)n * kc), o_sc = carve((size_t)n * kc * 4), o_wc = carve((size_t)n * kc);
    const size_t o_dc = carve((size_t)n), o_rc = carve((size_t)n * 3);
    const size_t o_zf = carve((size_t)n * kt), o_sf = carve((size_t)n * kt * 4);
    if ((rc = s->work.reserve(off * sizeof(float)))) return rc;
    float* W = s->work.f();
    float* zc = out->z_coarse ? out->z_coarse : W + o_zc;
    float* sc = out->sample_coarse ? out->sample_coarse : W + o_sc;
    float* wc = out->weights_coarse ? out->weights_coarse : W + o_wc;
    float* dc = out->depth_coarse ? out->depth_coarse : W + o_dc;
    float* rgbc = out->rgb_coarse ? out->rgb_coarse : W + o_rc;

    const bool stash = s->stash_next;
    s->stash_next = false;
    s->stashed[0].valid = s->stashed[1].valid = false;
    launch_sample_coarse(rays_dev, n, kc, o->lindisp, o->u_coarse_dev, o->seed, zc, st);
    if (cull) {
        if ((rc = culled_mlp(s, rays_dev, zc, n, kc, 1, sc, st, 0))) return rc;
    } else if ((rc = run_mlp(s, 1, nullptr, nullptr, rays_dev, zc, kc, (long long)n * kc, 1, sc, st, stash ? 0 : -1))) {
        return rc;
    }
    launch_composite(rays_dev, zc, sc, n, kc, o->white_bkgd, wc, rgbc, dc, st, o->sigma_noise_coarse_dev);
    if (o->n_fine > 0) {
        float* zf = out->z_fine ? out->z_fine : W + o_zf;
        float* sf = out->sample_fine ? out->sample_fine : W + o_sf;
        if ((size_t)(4 * kc + 1 + 2 * o->n_fine) * 4 * sizeof(float) > 160 * 1024)
            return fail(PNY_ERR_ARG, "pny_render: n_coarse + n_fine too large for the LDS-resident sort");
        launch_sample_fine(rays_dev, zc, wc, dc, n, kc, o->n_fine, o->n_fine_depth, o->depth_std, o->lindisp,
                           o->u_fine_dev, o->u_fine2_dev, o->g_depth_dev, o->seed, zf, st);
        if (cull) {
            if ((rc = culled_mlp(s, rays_dev, zf, n, kt, 0, sf, st, 1))) return rc;
        } else if ((rc = run_mlp(s, 1, nullptr, nullptr, rays_dev, zf, kt, (long long)n * kt, 0, sf, st, stash ? 1 : -1))) {
            return rc;
        }
        launch_composite(rays_dev, zf, sf, n, kt, o->white_bkgd, out->weights_fine, out->rgb_fine, out->depth_fine, st,
                         o->sigma_noise_fine_dev);
    }
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_render(pny_scene* s, const float* rays_dev, int64_t n, int n_coarse, const float* u_coarse_dev,
                    uint64_t seed, float* out_dev, float* raw_dev, pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_yolo_render"))) return rc;
    const pny_model_desc& d = s->m->desc;
    if (!d.yolo || d.d_out % 7) return fail(PNY_ERR_ARG, "pny_yolo_render: model is not in YOLO mode");
    if (n < 0 || n_coarse < 1 || (n > 0 && (!rays_dev || !out_dev))) return fail(PNY_ERR_ARG, "pny_yolo_render: bad argument");
    if (n == 0) return PNY_OK;
    PNY_HIP(hipSetDevice(d.device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = enter_stream(s, st))) return rc;
    begin_call(s);
    const size_t nz = ((size_t)n * n_coarse + 63) & ~(size_t)63;
    if ((rc = s->work.reserve((nz + (size_t)n * n_coarse * d.d_out) * sizeof(float)))) return rc;
    float* z = s->work.f();
    float* raw = raw_dev ? raw_dev : s->work.f() + nz;
    launch_sample_coarse(rays_dev, n, n_coarse, 0, u_coarse_dev, seed, z, st);
    if ((rc = run_mlp(s, 1, nullptr, nullptr, rays_dev, z, n_coarse, (long long)n * n_coarse, 1, raw, st))) return rc;
    launch_yolo_aggregate(raw, n, n_coarse, d.d_out / 7, out_dev, st);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_scene_enable_timing(pny_scene* s, int enable) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_enable_timing: null scene");
    s->timing = enable != 0;
    return PNY_OK;
}

int pny_scene_set_projection(pny_scene* s, int mode) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_set_projection: null scene");
    if (mode != PNY_PROJECTION_OFF && mode != PNY_PROJECTION_ON && mode != PNY_PROJECTION_AUTO)
        return fail(PNY_ERR_ARG, "pny_scene_set_projection: mode must be PNY_PROJECTION_{OFF,ON,AUTO}");
    s->zp_mode = mode;
    return PNY_OK;
}

int pny_scene_set_precision(pny_scene* s, int mode) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_set_precision: null scene");
    if (mode != PNY_PRECISION_F32 && mode != PNY_PRECISION_F16X2 && mode != PNY_PRECISION_AUTO && mode != PNY_PRECISION_F16 &&
        mode != PNY_PRECISION_F16_TRAIN)
        return fail(PNY_ERR_ARG, "pny_scene_set_precision: mode must be PNY_PRECISION_{F32,F16X2,AUTO,F16,F16_TRAIN}");
    // (F16_TRAIN, F16, F16X2 and AUTO project alike: only a switch to or from F32 re-projects)
    if ((mode == PNY_PRECISION_F32) != (s->precision == PNY_PRECISION_F32)) s->zp_valid[0] = s->zp_valid[1] = false;   // re-project in the new arithmetic
    s->precision = mode;
    if (mode == PNY_PRECISION_F16 || mode == PNY_PRECISION_F16_TRAIN) return want_h1_images(s->m, mode == PNY_PRECISION_F16_TRAIN);
    return PNY_OK;
}

int pny_model_range_status(pny_model* m, unsigned* bits, int clear) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_range_status: null model");
    const unsigned b = range_bits(m);
    if (bits) *bits = b;
    if (b & PNY_RANGE_WEIGHT) m->f16_weights_ok = false;   // until the next finalize re-checks on the host
    if (clear && m->range_flag()) __atomic_store_n(m->range_flag(), 0u, __ATOMIC_RELAXED);
    return PNY_OK;
}

int pny_scene_last_precision(pny_scene* s, int* f16x2) {
    if (!s || !f16x2) return fail(PNY_ERR_ARG, "pny_scene_last_precision: null argument");
    *f16x2 = s->last_prec;
    return PNY_OK;
}

int pny_scene_last_backward_precision(pny_scene* s, int* code) {
    if (!s || !code) return fail(PNY_ERR_ARG, "pny_scene_last_backward_precision: null argument");
    *code = s->last_bwd_prec;
    return PNY_OK;
}

int pny_scene_project(pny_scene* s, pny_stream stream) {
    int rc;
    if ((rc = check_ready(s, "pny_scene_project"))) return rc;
    if (!s->m->has_zproj) return PNY_OK;  // no per-view blocks: nothing to project
    if (s->zp_mode == PNY_PROJECTION_OFF) return fail(PNY_ERR_STATE, "pny_scene_project: projection is switched off for this scene");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    const int keep = s->zp_mode;
    s->zp_mode = PNY_PROJECTION_ON;
    const float* zp = nullptr;
    rc = ensure_projection(s, 0, 0, (hipStream_t)stream, &zp);
    if (!rc && s->m->desc.has_fine && s->m->use_fine) rc = ensure_projection(s, 1, 0, (hipStream_t)stream, &zp);
    s->zp_mode = keep;
    if (rc) return rc;
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_scene_projection(pny_scene* s, int fine, float* out_dev, int64_t out_floats, int* route, pny_stream stream) {
    if (!s || !out_dev) return fail(PNY_ERR_ARG, "pny_scene_projection: null argument");
    const pny_model* m = s->m;
    if (!m->finalized) return fail(PNY_ERR_STATE, "pny_scene_projection: weights not finalized (pny_model_finalize)");
    if (!m->has_zproj) return fail(PNY_ERR_ARG, "pny_scene_projection: the model has no per-view blocks, nothing is projected");
    if (!s->have_latent) return fail(PNY_ERR_STATE, "pny_scene_projection: scene has no latent (pny_scene_encode / pny_scene_set_latent)");
    const long long need = (long long)s->ns * s->hl * s->wl * view_blocks(m->desc) * HID;
    if (out_floats < need)
        return fail(PNY_ERR_ARG, "pny_scene_projection: out_dev holds " + std::to_string((long long)out_floats) + " floats, the maps need " +
                                     std::to_string(need));
    PNY_HIP(hipSetDevice(m->desc.device));
    int rc;
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    int launched = 0;
    if ((rc = project_latent(s, fine ? 1 : 0, out_dev, (hipStream_t)stream, &launched))) return rc;
    if (route) *route = launched;
    return PNY_OK;
}

int pny_scene_last_mlp_stats(pny_scene* s, double* flops, double* flops_reference, double* kernel_ms, int* launches,
                             int* projected) {
    if (!s) return fail(PNY_ERR_ARG, "pny_scene_last_mlp_stats: null scene");
    if (flops) *flops = s->last_flops;
    if (flops_reference) *flops_reference = s->last_flops_ref;
    if (projected) *projected = s->last_projected ? 1 : 0;
    if (launches) *launches = s->last_launches;
    if (kernel_ms) {
        double tot = 0.0;
        for (int i = 0; i + 1 < s->ev_used; i += 2) {
            PNY_HIP(hipEventSynchronize(s->ev[i + 1]));
            float ms = 0.f;
            PNY_HIP(hipEventElapsedTime(&ms, s->ev[i], s->ev[i + 1]));
            tot += ms;
        }
        *kernel_ms = s->timing ? tot : -1.0;
    }
    return PNY_OK;
}

}  // extern "C"
