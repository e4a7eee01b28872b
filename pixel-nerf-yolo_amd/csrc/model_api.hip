// C entry points of the model handle (include/pnyolo.h): the packed-weight layout, create / finalize / refresh and the
// f16-range status.  Host-side C++; the operand formats and the kernel that builds them are pack.hip's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "api_internal.h"

using namespace pny;

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
    for (pny_scene* s : m->scenes)
        if ((rc = s->order.hand_over(st))) return rc;
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

int pny_model_range_status(pny_model* m, unsigned* bits, int clear) {
    if (!m) return fail(PNY_ERR_ARG, "pny_model_range_status: null model");
    const unsigned b = range_bits(m);
    if (bits) *bits = b;
    if (b & PNY_RANGE_WEIGHT) m->f16_weights_ok = false;   // until the next finalize re-checks on the host
    if (clear && m->range_flag()) __atomic_store_n(m->range_flag(), 0u, __ATOMIC_RELAXED);
    return PNY_OK;
}

}  // extern "C"
