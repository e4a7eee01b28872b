// C entry points of the occupancy grid (include/pnyolo.h, "occupancy grid" section; kernels in occupancy.hip; the culled passes of
// pny_render in render_api.hip): argument checks, then the launches.  The model-free entries allocate nothing and wait for nothing;
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

}  // extern "C"
