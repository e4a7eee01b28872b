// C entry point of the view metrics (include/pnyolo.h, "view metrics" section; kernel in metrics.hip): argument checks, the
// per-stream reduction workspace, one launch.
#include <mutex>
#include <string>

#include "api_internal.h"
#include "pny_metrics.h"

namespace pny {
void launch_view_metrics(const ViewMetricsArgs& a, hipStream_t st);
}

using namespace pny;

namespace {

// The ticket counter (its own 256 bytes, the part that is zeroed) and the table of one row per workgroup, one per (device,
// stream) (dev_resource.h StreamBlocks), as the losses keep theirs (loss_api.hip).  The table holds METRICS_WS_ROWS rows from
// the first call on a stream on; a launch of more workgroups (more than 65 536 tiles: 2 000 views of 128 x 128) replaces it by
// a larger one, and only that replacement waits for the device (hipFree).
constexpr size_t METRICS_WS_ROWS = 65536;
StreamBlocks<std::mutex> g_ws{"hipMalloc(&q, bytes)", "hipMemsetAsync(metrics workspace)"};

int metrics_workspace(hipStream_t st, size_t rows, unsigned** ticket, double** partials) {
    const size_t want = rows > METRICS_WS_ROWS ? rows : METRICS_WS_ROWS;
    void* p = nullptr;
    if (int rc = g_ws.get(st, 256 + want * METRICS_SUMS * sizeof(double), 256, &p)) return rc;
    *ticket = reinterpret_cast<unsigned*>(p);
    *partials = reinterpret_cast<double*>(reinterpret_cast<char*>(p) + 256);
    return 0;
}

}  // namespace

extern "C" {

int pny_view_metrics(const pny_view_metrics_desc* desc, const float* rgb_dev, const float* gt_dev, double* metrics_dev,
                     uint8_t* rgb8_dev, pny_stream stream) {
    const char* who = "pny_view_metrics: ";
    if (!desc || !rgb_dev || !gt_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (!metrics_dev && !rgb8_dev) return fail(PNY_ERR_ARG, std::string(who) + "both outputs are null");
    if (desc->win_size != METRICS_WIN) return fail(PNY_ERR_ARG, std::string(who) + "win_size must be 7 in this build");
    if (desc->n_views <= 0 || desc->height <= 0 || desc->width <= 0)
        return fail(PNY_ERR_ARG, std::string(who) + "n_views, height and width must be positive");
    const bool flat = desc->gt_layout == PNY_GT_FLAT;
    if (desc->gt_layout != PNY_GT_NHWC_01 && desc->gt_layout != PNY_GT_NCHW_PM1 && !flat)
        return fail(PNY_ERR_ARG, std::string(who) + "unknown gt_layout");
    if (flat && rgb8_dev) return fail(PNY_ERR_ARG, std::string(who) + "PNY_GT_FLAT has no 8-bit output");
    if (!flat && (desc->height < METRICS_WIN || desc->width < METRICS_WIN))
        return fail(PNY_ERR_ARG, std::string(who) + "height and width must be at least win_size");
    const int64_t elems = (int64_t)desc->n_views * desc->height * desc->width * (flat ? 1 : 3);
    if (elems >= ((int64_t)1 << 31)) return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
    ViewMetricsArgs a;
    a.rgb = rgb_dev, a.gt = gt_dev, a.metrics = metrics_dev, a.rgb8 = rgb8_dev;
    a.nv = desc->n_views, a.layout = desc->gt_layout;
    a.h = flat ? 1 : desc->height, a.w = flat ? desc->height * desc->width : desc->width;
    a.tiles_y = flat ? 1 : metrics_tiles(a.h, METRICS_TILE_H);
    a.tiles_x = flat ? (a.w + METRICS_FLAT_CHUNK - 1) / METRICS_FLAT_CHUNK : metrics_tiles(a.w, METRICS_TILE_W);
    a.ticket = nullptr, a.partials = nullptr;
    int rc;
    if (metrics_dev && (rc = metrics_workspace((hipStream_t)stream, (size_t)a.nv * a.tiles_y * a.tiles_x, &a.ticket, &a.partials)))
        return rc;
    launch_view_metrics(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
