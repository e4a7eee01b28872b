// C entry points of the scene handle (include/pnyolo.h): cameras, the latent and the encoders that produce it, the scene's
// settings and what it reports of its last call.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "api_internal.h"

using namespace pny;

extern "C" {

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
    if (n_objs > 1) s->term_on = false;  // ... and termination one object's rays
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
        if ((rc = scenes[i]->order.mark(st))) return rc;
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
