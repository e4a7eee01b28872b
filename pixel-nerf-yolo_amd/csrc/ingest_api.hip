// C entry points of the device ingest (include/pnyolo.h, "ingest" section; kernels in ingest.hip): argument checks, then one
// launch (two for pny_ingest_views with white_mask).  No workspace, no allocation, no synchronisation.
#include <math.h>

#include <string>

#include "api_internal.h"
#include "pny_ingest.h"

namespace pny {
void launch_ingest(const IngestArgs& a, int n_views, hipStream_t st);
void launch_ingest_box(const IngestBoxArgs& a, int n_views, hipStream_t st);
void launch_targets(const TargetsArgs& a, int n_views, hipStream_t st);
}  // namespace pny

using namespace pny;

static_assert(INGEST_RESIZE_NONE == PNY_RESIZE_NONE && INGEST_RESIZE_BILINEAR_U8 == PNY_RESIZE_BILINEAR_U8 &&
                  INGEST_RESIZE_AREA == PNY_RESIZE_AREA, "pny_ingest.h and pnyolo.h disagree on the resize modes");
static_assert(TARGETS_MAX_SCALES == PNY_YOLO_BATCH_MAX_SCALES, "pny_ingest.h and pnyolo.h disagree on the scales");
static_assert(TARGETS_MAX_ANCHORS == PNY_YOLO_TARGETS_MAX_ANCHORS, "pny_ingest.h and pnyolo.h disagree on the anchors");

extern "C" {

int pny_ingest_views(const pny_ingest_desc* desc, const uint8_t* images_dev, float* out_dev, float* mask_dev, float* bbox_dev,
                     pny_stream stream) {
    const char* who = "pny_ingest_views: ";
    if (!desc || !images_dev || !out_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (desc->n_views <= 0 || desc->height <= 0 || desc->width <= 0 || desc->out_height <= 0 || desc->out_width <= 0)
        return fail(PNY_ERR_ARG, std::string(who) + "n_views, height, width, out_height and out_width must be positive");
    if (desc->channels != 3 && desc->channels != 4) return fail(PNY_ERR_ARG, std::string(who) + "channels must be 3 or 4");
    if (desc->resize != PNY_RESIZE_NONE && desc->resize != PNY_RESIZE_BILINEAR_U8 && desc->resize != PNY_RESIZE_AREA)
        return fail(PNY_ERR_ARG, std::string(who) + "unknown resize");
    if (desc->resize == PNY_RESIZE_NONE && (desc->out_height != desc->height || desc->out_width != desc->width))
        return fail(PNY_ERR_ARG, std::string(who) + "PNY_RESIZE_NONE needs out_height == height and out_width == width");
    const int64_t lim = (int64_t)1 << 31;
    const int64_t in_px = (int64_t)desc->height * desc->width, out_px = (int64_t)desc->out_height * desc->out_width;
    if (in_px >= lim || out_px >= lim || in_px * desc->channels >= lim || in_px * desc->channels * desc->n_views >= lim ||
        out_px * 3 * desc->n_views >= lim)
        return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
    if (desc->white_mask != 0 && desc->white_mask != 1) return fail(PNY_ERR_ARG, std::string(who) + "white_mask must be 0 or 1");
    if (!desc->white_mask && (mask_dev || bbox_dev))
        return fail(PNY_ERR_ARG, std::string(who) + "mask_dev and bbox_dev need white_mask");
    if (desc->white_mask && (!mask_dev || !bbox_dev))
        return fail(PNY_ERR_ARG, std::string(who) + "white_mask needs mask_dev and bbox_dev");
    if (desc->white_mask && desc->resize == PNY_RESIZE_BILINEAR_U8)
        return fail(PNY_ERR_ARG, std::string(who) + "white_mask with PNY_RESIZE_BILINEAR_U8 (no dataset resizes a mask that way)");
    IngestArgs a;
    a.in = images_dev, a.out = out_dev, a.mask = mask_dev;
    a.h = desc->height, a.w = desc->width, a.c = desc->channels, a.oh = desc->out_height, a.ow = desc->out_width;
    a.resize = desc->resize;
    a.tiles_x = (a.ow + INGEST_TILE_X - 1) / INGEST_TILE_X, a.tiles_y = (a.oh + INGEST_TILE_Y - 1) / INGEST_TILE_Y;
    a.scale_y = (float)a.h / (float)a.oh, a.scale_x = (float)a.w / (float)a.ow;
    if ((int64_t)a.tiles_x * a.tiles_y * desc->n_views >= lim) return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
    launch_ingest(a, desc->n_views, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    if (desc->white_mask) {
        IngestBoxArgs b;
        b.in = images_dev, b.bbox = bbox_dev, b.h = a.h, b.w = a.w, b.c = a.c;
        b.scaled = desc->resize != PNY_RESIZE_NONE;
        b.scale = (float)((double)desc->out_height / (double)desc->height);      // data.py:129-133, a double rounded once
        launch_ingest_box(b, desc->n_views, (hipStream_t)stream);
        PNY_HIP(hipGetLastError());
    }
    return PNY_OK;
}

int pny_yolo_build_targets(const pny_yolo_targets_desc* desc, const double* boxes_dev, const int32_t* n_boxes_dev,
                           const float* anchors_host, float* const* targets_dev, pny_stream stream) {
    const char* who = "pny_yolo_build_targets: ";
    if (!desc || !boxes_dev || !n_boxes_dev || !anchors_host || !targets_dev)
        return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (desc->n_views <= 0 || desc->max_boxes <= 0 || desc->height <= 0 || desc->width <= 0)
        return fail(PNY_ERR_ARG, std::string(who) + "n_views, max_boxes, height and width must be positive");
    if (desc->n_scales < 1 || desc->n_scales > PNY_YOLO_BATCH_MAX_SCALES)
        return fail(PNY_ERR_ARG, std::string(who) + "n_scales must be 1 .. 4");
    if (desc->n_anchors < 1 || desc->n_anchors > PNY_YOLO_TARGETS_MAX_ANCHORS ||
        desc->n_scales * desc->n_anchors > PNY_YOLO_TARGETS_MAX_ANCHORS)
        return fail(PNY_ERR_ARG, std::string(who) + "n_anchors must be 1 .. 64 and n_scales * n_anchors at most 64");
    if (!(desc->ignore_iou_thresh >= 0.0f) || isinf(desc->ignore_iou_thresh))
        return fail(PNY_ERR_ARG, std::string(who) + "ignore_iou_thresh must be finite and not negative");
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)desc->n_views * desc->max_boxes * 5 >= lim) return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
    TargetsArgs a;
    for (int s = 0; s < TARGETS_MAX_SCALES; ++s) a.g.hs[s] = a.g.ws[s] = 0, a.grid[s] = nullptr;
    for (int s = 0; s < desc->n_scales; ++s) {
        const int cell = desc->cell_sizes[s];
        if (cell < 1 || cell > desc->height || cell > desc->width)
            return fail(PNY_ERR_ARG, std::string(who) + "a cell size below 1 or above the image");
        if (!targets_dev[s]) return fail(PNY_ERR_ARG, std::string(who) + "null argument (a target grid)");
        a.g.hs[s] = desc->height / cell, a.g.ws[s] = desc->width / cell;
        if ((int64_t)a.g.hs[s] * a.g.ws[s] * desc->n_anchors * 6 * desc->n_views >= lim)
            return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
        a.grid[s] = targets_dev[s];
    }
    a.g.n_scales = desc->n_scales, a.g.n_anchors = desc->n_anchors, a.g.thresh = desc->ignore_iou_thresh;
    const int na = desc->n_scales * desc->n_anchors;
    for (int i = 0; i < 2 * TARGETS_MAX_ANCHORS; ++i) a.g.anchors[i] = i < 2 * na ? anchors_host[i] : 1.0f;
    a.boxes = boxes_dev, a.n_boxes = n_boxes_dev, a.max_boxes = desc->max_boxes;
    launch_targets(a, desc->n_views, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
