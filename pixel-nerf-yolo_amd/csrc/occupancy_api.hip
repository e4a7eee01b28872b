// C entry points of the occupancy grid and of early ray termination (include/pnyolo.h, "occupancy grid" and "early ray
// termination" sections; kernels in occupancy.hip and termination.hip; the culled passes of pny_render in render_api.hip): argument checks, then the launches.  The model-free entries allocate nothing and wait for nothing;
// pny_scene_set_occupancy copies the bits into a buffer the scene owns.
#include <math.h>

#include <string>

#include "api_internal.h"

using namespace pny;

namespace {

// dims = {X, Y, Z}: each at least 2 and 3 X Y Z below 2^31
int check_dims(const char* who, const int32_t* dims) {
    for (int k = 0; k < 3; ++k)
        if (dims[k] < 2) return fail(PNY_ERR_ARG, std::string(who) + "every dimension must be at least 2");
    if ((int64_t)dims[0] * dims[1] * dims[2] > MC_MAX_POINTS) return fail(PNY_ERR_ARG, std::string(who) + "3 X Y Z must be below 2^31");
    return 0;
}

int check_box(const char* who, const double* c1, const double* c2) {
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(c1[k]) || !isfinite(c2[k])) return fail(PNY_ERR_ARG, std::string(who) + "bounds must be finite");
        if (!(c2[k] > c1[k])) return fail(PNY_ERR_ARG, std::string(who) + "c2 must be above c1 on every axis");
    }
    return 0;
}

}  // namespace

namespace pny {
void occupancy_classify(const OccGrid& g, const float* rays, const float* z, int64_t n_samples, int k, int32_t* slot, int64_t* kept,
                        void* workspace, hipStream_t st) {
    const OccLayout l = occ_layout(n_samples);
    char* ws = reinterpret_cast<char*>(workspace);
    OccClassifyArgs a;
    a.g = g, a.rays = rays, a.z = z, a.n_samples = (uint32_t)n_samples, a.K = (uint32_t)k, a.slot = slot;
    a.sums1 = reinterpret_cast<uint32_t*>(ws + l.sums1);
    launch_occupancy_classify(a, l, reinterpret_cast<uint32_t*>(ws + l.sums2), kept, st);
}

void occupancy_classify_segment(const OccGrid& g, const float* rays, const float* z, int64_t n, int k, int k_begin, int k_end,
                                const uint8_t* alive, int32_t* slot, int64_t* kept, void* workspace, hipStream_t st) {
    const int64_t n_samples = n * (k_end - k_begin);
    const OccLayout l = occ_layout(n_samples);
    char* ws = reinterpret_cast<char*>(workspace);
    OccSegmentArgs a;
    a.g = g, a.rays = rays, a.z = z, a.alive = alive, a.n_samples = (uint32_t)n_samples;
    a.K = (uint32_t)k, a.k_begin = (uint32_t)k_begin, a.Ks = (uint32_t)(k_end - k_begin), a.slot = slot;
    a.sums1 = reinterpret_cast<uint32_t*>(ws + l.sums1);
    launch_occupancy_classify_segment(a, l, reinterpret_cast<uint32_t*>(ws + l.sums2), kept, st);
}
}  // namespace pny

extern "C" {

int pny_occupancy_words(const int32_t dims[3], int64_t* words) {
    const char* who = "pny_occupancy_words: ";
    if (!dims || !words) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (int rc = check_dims(who, dims)) return rc;
    *words = occ_words(occ_cells(dims[0], dims[1], dims[2]));
    return PNY_OK;
}

int pny_occupancy_build(const float* sigma_dev, const float* sigma2_dev, const int32_t dims[3], float thresh, int dilate,
                        uint32_t* bits_dev, int64_t* occupied_dev, pny_stream stream) {
    const char* who = "pny_occupancy_build: ";
    if (!sigma_dev || !dims || !bits_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (int rc = check_dims(who, dims)) return rc;
    if (thresh != thresh) return fail(PNY_ERR_ARG, std::string(who) + "thresh must not be a NaN");
    if (dilate < 0 || dilate > OCC_MAX_DILATE) return fail(PNY_ERR_ARG, std::string(who) + "dilate out of range [0,4]");
    OccBuildArgs a;
    a.sigma = sigma_dev, a.sigma2 = sigma2_dev, a.d.x = dims[0], a.d.y = dims[1], a.d.z = dims[2], a.thresh = thresh, a.dilate = dilate;
    a.bits = bits_dev, a.occupied = reinterpret_cast<unsigned long long*>(occupied_dev);
    a.n_words = (uint32_t)occ_words(occ_cells(dims[0], dims[1], dims[2]));
    if (occupied_dev) PNY_HIP(hipMemsetAsync(occupied_dev, 0, sizeof(int64_t), (hipStream_t)stream));
    launch_occupancy_build(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_occupancy_classify_workspace_bytes(int64_t n_samples, int64_t* bytes) {
    const char* who = "pny_occupancy_classify_workspace_bytes: ";
    if (!bytes) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n_samples < 0 || n_samples > OCC_MAX_SAMPLES) return fail(PNY_ERR_ARG, std::string(who) + "need 0 <= n k <= 2^30 samples");
    *bytes = (int64_t)occ_layout(n_samples).bytes;
    return PNY_OK;
}

int pny_occupancy_classify(const uint32_t* bits_dev, const int32_t dims[3], const double c1[3], const double c2[3], int outside_empty,
                           const float* rays_dev, const float* z_dev, int64_t n, int k, int32_t* slot_dev, int64_t* kept_dev,
                           void* workspace_dev, int64_t workspace_bytes, pny_stream stream) {
    const char* who = "pny_occupancy_classify: ";
    if (!bits_dev || !dims || !c1 || !c2 || !kept_dev || !workspace_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n < 0 || k < 1) return fail(PNY_ERR_ARG, std::string(who) + "need n >= 0 and k >= 1");
    if (n > 0 && (!rays_dev || !z_dev || !slot_dev)) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    int rc;
    if ((rc = check_dims(who, dims)) || (rc = check_box(who, c1, c2))) return rc;
    if (n > OCC_MAX_SAMPLES / k) return fail(PNY_ERR_ARG, std::string(who) + "need n k <= 2^30 samples");
    if (reinterpret_cast<uintptr_t>(rays_dev) % 16) return fail(PNY_ERR_ARG, std::string(who) + "rays_dev must be 16-byte aligned");
    if (workspace_bytes < (int64_t)occ_layout(n * k).bytes || reinterpret_cast<uintptr_t>(workspace_dev) % 256)
        return fail(PNY_ERR_ARG, std::string(who) + "workspace too small (pny_occupancy_classify_workspace_bytes) or not 256-byte aligned");
    if (n == 0) {
        PNY_HIP(hipMemsetAsync(kept_dev, 0, sizeof(int64_t), (hipStream_t)stream));
        return PNY_OK;
    }
    OccGrid g;
    g.bits = bits_dev, g.outside_empty = outside_empty != 0;
    occ_grid_axes(g, dims, c1, c2);
    occupancy_classify(g, rays_dev, z_dev, n * k, k, slot_dev, kept_dev, workspace_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_scene_set_occupancy(pny_scene* s, const uint32_t* bits_dev, const int32_t dims[3], const double c1[3], const double c2[3],
                            int outside_empty, pny_stream stream) {
    const char* who = "pny_scene_set_occupancy: ";
    if (!s) return fail(PNY_ERR_ARG, std::string(who) + "null scene");
    if (!bits_dev) {
        s->occ_on = false;
        return PNY_OK;
    }
    if (!dims || !c1 || !c2) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    int rc;
    if ((rc = check_dims(who, dims)) || (rc = check_box(who, c1, c2))) return rc;
    if (s->m->desc.yolo || s->m->desc.d_out != 4)
        return fail(PNY_ERR_ARG, std::string(who) + "the model is in YOLO mode: its aggregation weighs by objectness, not by sigma");
    if (s->n_objs > 1) return fail(PNY_ERR_ARG, std::string(who) + "the scene is grouped (pny_scene_set_groups): one grid serves one object");
    PNY_HIP(hipSetDevice(s->m->desc.device));
    if ((rc = enter_stream(s, (hipStream_t)stream))) return rc;
    const size_t bytes = (size_t)occ_words(occ_cells(dims[0], dims[1], dims[2])) * sizeof(uint32_t);
    s->occ_on = false;
    if ((rc = s->occ_bits.reserve(bytes, "hipMalloc(occupancy bits)"))) return rc;
    PNY_HIP(hipMemcpyAsync(s->occ_bits.p, bits_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    s->occ.bits = reinterpret_cast<const uint32_t*>(s->occ_bits.p);
    s->occ.outside_empty = outside_empty != 0;
    occ_grid_axes(s->occ, dims, c1, c2);
    s->occ_on = true;
    return PNY_OK;
}

int pny_scene_last_cull(pny_scene* s, int64_t kept[2], int64_t total[2]) {
    if (!s || !kept || !total) return fail(PNY_ERR_ARG, "pny_scene_last_cull: null argument");
    for (int p = 0; p < 2; ++p) kept[p] = s->cull_kept[p], total[p] = s->cull_total[p];
    return PNY_OK;
}

// ---------------------------------------------------------------------------------- early ray termination (pny_termination.h)
int pny_occupancy_classify_segment(const uint32_t* bits_dev, const int32_t dims[3], const double c1[3], const double c2[3],
                                   int outside_empty, const float* rays_dev, const float* z_dev, int64_t n, int k, int k_begin, int k_end,
                                   const uint8_t* alive_dev, int32_t* slot_dev, int64_t* kept_dev, void* workspace_dev,
                                   int64_t workspace_bytes, pny_stream stream) {
    const char* who = "pny_occupancy_classify_segment: ";
    if (!kept_dev || !workspace_dev || (bits_dev && (!dims || !c1 || !c2))) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n < 0 || k < 1) return fail(PNY_ERR_ARG, std::string(who) + "need n >= 0 and k >= 1");
    if (k_begin < 0 || k_begin >= k_end || k_end > k) return fail(PNY_ERR_ARG, std::string(who) + "need 0 <= k_begin < k_end <= k");
    if (n > 0 && (!rays_dev || !z_dev || !slot_dev)) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    int rc;
    if (bits_dev && ((rc = check_dims(who, dims)) || (rc = check_box(who, c1, c2)))) return rc;
    if (n > OCC_MAX_SAMPLES / k) return fail(PNY_ERR_ARG, std::string(who) + "need n k <= 2^30 samples");
    if (reinterpret_cast<uintptr_t>(rays_dev) % 16) return fail(PNY_ERR_ARG, std::string(who) + "rays_dev must be 16-byte aligned");
    if (workspace_bytes < (int64_t)occ_layout(n * (k_end - k_begin)).bytes || reinterpret_cast<uintptr_t>(workspace_dev) % 256)
        return fail(PNY_ERR_ARG, std::string(who) + "workspace too small (pny_occupancy_classify_workspace_bytes) or not 256-byte aligned");
    if (n == 0) {
        PNY_HIP(hipMemsetAsync(kept_dev, 0, sizeof(int64_t), (hipStream_t)stream));
        return PNY_OK;
    }
    OccGrid g{};
    g.bits = bits_dev, g.outside_empty = outside_empty != 0;
    if (bits_dev) occ_grid_axes(g, dims, c1, c2);
    occupancy_classify_segment(g, rays_dev, z_dev, n, k, k_begin, k_end, alive_dev, slot_dev, kept_dev, workspace_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_termination_update(const float* rays_dev, const float* z_dev, const float* sample_dev, int64_t n, int k, int k_begin, int k_end,
                           float t_min, float* T_dev, uint8_t* alive_dev, int64_t* alive_count_dev, pny_stream stream) {
    const char* who = "pny_termination_update: ";
    if (n < 0 || k < 1) return fail(PNY_ERR_ARG, std::string(who) + "need n >= 0 and k >= 1");
    if (k_begin < 0 || k_begin >= k_end || k_end > k) return fail(PNY_ERR_ARG, std::string(who) + "need 0 <= k_begin < k_end <= k");
    if (t_min != t_min) return fail(PNY_ERR_ARG, std::string(who) + "t_min must not be a NaN");
    if (!(t_min >= 0.0f && t_min < 1.0f)) return fail(PNY_ERR_ARG, std::string(who) + "t_min out of range [0,1)");
    if (n > 0 && (!rays_dev || !z_dev || !sample_dev || !T_dev || !alive_dev)) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n > OCC_MAX_SAMPLES / k) return fail(PNY_ERR_ARG, std::string(who) + "need n k <= 2^30 samples");
    if (reinterpret_cast<uintptr_t>(sample_dev) % 16) return fail(PNY_ERR_ARG, std::string(who) + "sample_dev must be 16-byte aligned");
    if (alive_count_dev) PNY_HIP(hipMemsetAsync(alive_count_dev, 0, sizeof(int64_t), (hipStream_t)stream));
    if (n == 0) return PNY_OK;
    TermUpdateArgs a;
    a.rays = rays_dev, a.z = z_dev, a.samp = sample_dev, a.n = n, a.K = k, a.k_begin = k_begin, a.k_end = k_end, a.t_min = t_min;
    a.T = T_dev, a.alive = alive_dev, a.alive_count = reinterpret_cast<unsigned long long*>(alive_count_dev);
    launch_termination_update(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_scene_set_termination(pny_scene* s, float t_min, int segments) {
    const char* who = "pny_scene_set_termination: ";
    if (!s) return fail(PNY_ERR_ARG, std::string(who) + "null scene");
    if (t_min != t_min) return fail(PNY_ERR_ARG, std::string(who) + "t_min must not be a NaN");
    if (!(t_min >= 0.0f && t_min < 1.0f)) return fail(PNY_ERR_ARG, std::string(who) + "t_min out of range [0,1)");
    if (t_min == 0.0f) {
        s->term_on = false;
        return PNY_OK;
    }
    if (segments < 1 || segments > TERM_MAX_SEGMENTS) return fail(PNY_ERR_ARG, std::string(who) + "segments out of range [1,16]");
    if (s->m->desc.yolo || s->m->desc.d_out != 4)
        return fail(PNY_ERR_ARG, std::string(who) + "the model is in YOLO mode: its aggregation weighs by objectness, not by sigma");
    if (s->n_objs > 1)
        return fail(PNY_ERR_ARG, std::string(who) + "the scene is grouped (pny_scene_set_groups): termination serves one object's rays");
    s->term_t_min = t_min, s->term_segments = segments;
    s->term_on = true;
    return PNY_OK;
}

int pny_scene_last_segments(pny_scene* s, int pass, int64_t* alive_rays, int64_t* kept, int cap, int* n_issued) {
    const char* who = "pny_scene_last_segments: ";
    if (!s || !n_issued || (cap > 0 && (!alive_rays || !kept))) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (pass < 0 || pass > 1 || cap < 0) return fail(PNY_ERR_ARG, std::string(who) + "need pass 0 or 1 and cap >= 0");
    *n_issued = s->seg_issued[pass];
    for (int j = 0; j < cap && j < s->seg_issued[pass]; ++j) alive_rays[j] = s->seg_alive[pass][j], kept[j] = s->seg_kept[pass][j];
    return PNY_OK;
}

}  // extern "C"
