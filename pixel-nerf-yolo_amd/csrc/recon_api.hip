// C entry points of the mesh extraction (include/pnyolo.h, "mesh extraction" section; kernels in recon.hip): argument checks,
// then the launches.  No allocation, no copy, no synchronisation: the caller owns the workspace and reads the two counts.
#include <math.h>

#include <string>

#include "api_internal.h"
#include "pny_recon.h"

namespace pny {
void launch_grid_points(const GridArgs& a, hipStream_t st);
void launch_mc_count(const McArgs& a, const McLayout& l, McCount* sums2, int32_t* counts, hipStream_t st);
void launch_mc_vertices(const McArgs& a, hipStream_t st);
void launch_mc_triangles(const McArgs& a, hipStream_t st);
}  // namespace pny

using namespace pny;

namespace {

// dims = {X, Y, Z}: each at least 2 and 3 X Y Z below 2^31
int check_dims(const char* who, const int32_t* dims) {
    for (int k = 0; k < 3; ++k)
        if (dims[k] < 2) return fail(PNY_ERR_ARG, std::string(who) + "every dimension must be at least 2");
    if ((int64_t)dims[0] * dims[1] * dims[2] > MC_MAX_POINTS) return fail(PNY_ERR_ARG, std::string(who) + "3 X Y Z must be below 2^31");
    return 0;
}

McArgs mc_args(const float* sigma, const int32_t* dims, float iso, void* workspace, const McLayout& l) {
    char* ws = reinterpret_cast<char*>(workspace);
    McArgs a;
    a.sigma = sigma, a.d.x = dims[0], a.d.y = dims[1], a.d.z = dims[2], a.iso = iso;
    a.voff = reinterpret_cast<uint32_t*>(ws + l.voff), a.toff = reinterpret_cast<uint32_t*>(ws + l.toff);
    a.sums1 = reinterpret_cast<McCount*>(ws + l.sums1);
    a.n_points = (uint32_t)l.n_points;
    a.n_vertices = a.n_triangles = 0, a.vertices = nullptr, a.triangles = nullptr;
    return a;
}

}  // namespace

extern "C" {

int pny_grid_points(const double* c1_host, const double* c2_host, const int32_t* reso_host, int64_t i0, int64_t i1, float* xyz_dev,
                    float* dirs_dev, pny_stream stream) {
    const char* who = "pny_grid_points: ";
    if (!c1_host || !c2_host || !reso_host || !xyz_dev || !dirs_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    for (int k = 0; k < 3; ++k) {
        if (reso_host[k] < 2) return fail(PNY_ERR_ARG, std::string(who) + "every reso must be at least 2");
        if (!isfinite(c1_host[k]) || !isfinite(c2_host[k])) return fail(PNY_ERR_ARG, std::string(who) + "bounds must be finite");
        if (!(c2_host[k] > c1_host[k])) return fail(PNY_ERR_ARG, std::string(who) + "c2 must be above c1 on every axis");
    }
    const int64_t n = (int64_t)reso_host[0] * reso_host[1] * reso_host[2];
    if (n > MC_MAX_POINTS) return fail(PNY_ERR_ARG, std::string(who) + "3 X Y Z must be below 2^31");
    if (i0 < 0 || i1 > n || i0 >= i1) return fail(PNY_ERR_ARG, std::string(who) + "need 0 <= i0 < i1 <= X Y Z");
    GridArgs a;
    a.xyz = xyz_dev, a.dirs = dirs_dev, a.sx = reso_host[0], a.sy = reso_host[1], a.sz = reso_host[2], a.i0 = i0, a.i1 = i1;
    for (int k = 0; k < 3; ++k) {
        a.lo[k] = c1_host[k], a.hi[k] = c2_host[k];
        a.step[k] = (c2_host[k] - c1_host[k]) / (double)(reso_host[k] - 1);      // np.linspace: delta / div
    }
    launch_grid_points(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_mc_workspace_bytes(const int32_t* dims_host, int64_t* bytes) {
    const char* who = "pny_mc_workspace_bytes: ";
    if (!dims_host || !bytes) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    int rc;
    if ((rc = check_dims(who, dims_host))) return rc;
    *bytes = (int64_t)mc_layout(dims_host[0], dims_host[1], dims_host[2]).bytes;
    return PNY_OK;
}

int pny_mc_count(const float* sigma_dev, const int32_t* dims_host, float iso, void* workspace_dev, int32_t* counts_dev,
                 pny_stream stream) {
    const char* who = "pny_mc_count: ";
    if (!sigma_dev || !dims_host || !workspace_dev || !counts_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    int rc;
    if ((rc = check_dims(who, dims_host))) return rc;
    if (!isfinite(iso)) return fail(PNY_ERR_ARG, std::string(who) + "iso must be finite");
    const McLayout l = mc_layout(dims_host[0], dims_host[1], dims_host[2]);
    const McArgs a = mc_args(sigma_dev, dims_host, iso, workspace_dev, l);
    launch_mc_count(a, l, reinterpret_cast<McCount*>(reinterpret_cast<char*>(workspace_dev) + l.sums2), counts_dev, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_mc_emit(const float* sigma_dev, const int32_t* dims_host, float iso, const void* workspace_dev, int64_t n_vertices,
                int64_t n_triangles, float* vertices_dev, int32_t* triangles_dev, pny_stream stream) {
    const char* who = "pny_mc_emit: ";
    if (!sigma_dev || !dims_host || !workspace_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    int rc;
    if ((rc = check_dims(who, dims_host))) return rc;
    if (!isfinite(iso)) return fail(PNY_ERR_ARG, std::string(who) + "iso must be finite");
    if (n_vertices < 0 || n_triangles < 0) return fail(PNY_ERR_ARG, std::string(who) + "negative count");
    if ((n_vertices > 0 && !vertices_dev) || (n_triangles > 0 && !triangles_dev))
        return fail(PNY_ERR_ARG, std::string(who) + "null argument (an output with a positive count)");
    const McLayout l = mc_layout(dims_host[0], dims_host[1], dims_host[2]);
    if (n_vertices > 3 * l.n_points || n_triangles > (int64_t)5 * l.n_points)
        return fail(PNY_ERR_ARG, std::string(who) + "more vertices or triangles than the volume can have");
    McArgs a = mc_args(sigma_dev, dims_host, iso, const_cast<void*>(workspace_dev), l);
    a.n_vertices = n_vertices, a.n_triangles = n_triangles, a.vertices = vertices_dev, a.triangles = triangles_dev;
    if (n_vertices > 0) {
        launch_mc_vertices(a, (hipStream_t)stream);
        PNY_HIP(hipGetLastError());
    }
    if (n_triangles > 0) {
        launch_mc_triangles(a, (hipStream_t)stream);
        PNY_HIP(hipGetLastError());
    }
    return PNY_OK;
}

}  // extern "C"
