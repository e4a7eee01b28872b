// C entry points of the training losses (include/pnyolo.h, "training losses" section; kernels in loss.hip): argument checks,
// the per-stream reduction workspace, one launch.
#include <mutex>
#include <string>

#include "api_internal.h"
#include "pny_loss.h"

using namespace pny;

namespace {

// The ticket counter and the partial-sum table of a launch, one per (device, stream) (dev_resource.h StreamBlocks): a fixed
// LOSS_WS_BYTES, all of it zeroed.
StreamBlocks<std::mutex> g_ws{"hipMalloc(&q, LOSS_WS_BYTES)", "hipMemsetAsync(loss workspace)"};

int loss_workspace(hipStream_t st, unsigned** ticket, double** partials) {
    void* p = nullptr;
    if (int rc = g_ws.get(st, LOSS_WS_BYTES, LOSS_WS_BYTES, &p)) return rc;
    *ticket = reinterpret_cast<unsigned*>(p);
    *partials = reinterpret_cast<double*>(reinterpret_cast<char*>(p) + 256);
    return 0;
}

}  // namespace

extern "C" {

int pny_rgb_loss(const pny_rgb_loss_desc* desc, const float* coarse_dev, const float* fine_dev, const float* gt_dev, int64_t n,
                 float* terms_dev, float* d_coarse_dev, float* d_fine_dev, pny_stream stream) {
    const char* who = "pny_rgb_loss: ";
    if (!desc || !coarse_dev || !gt_dev || !terms_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n <= 0) return fail(PNY_ERR_ARG, std::string(who) + "n must be positive");
    if (d_fine_dev && !fine_dev) return fail(PNY_ERR_ARG, std::string(who) + "d_fine_dev without fine_dev");
    RgbLossArgs a;
    a.coarse = coarse_dev, a.fine = fine_dev, a.gt = gt_dev, a.n = n;
    a.l1_coarse = desc->use_l1_coarse != 0, a.l1_fine = desc->use_l1_fine != 0;
    a.lambda_coarse = desc->lambda_coarse, a.lambda_fine = desc->lambda_fine;
    a.terms = terms_dev, a.d_coarse = d_coarse_dev, a.d_fine = d_fine_dev;
    int rc;
    if ((rc = loss_workspace((hipStream_t)stream, &a.ticket, &a.partials))) return rc;
    launch_rgb_loss(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_loss(const pny_yolo_loss_desc* desc, const float* pred_dev, const float* target_dev, const float* anchors_dev,
                  int64_t cells, float* terms_dev, int32_t* counts_dev, float* d_pred_dev, pny_stream stream) {
    const char* who = "pny_yolo_loss: ";
    if (!desc || !pred_dev || !target_dev || !anchors_dev || !terms_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (cells <= 0) return fail(PNY_ERR_ARG, std::string(who) + "cells must be positive");
    if (desc->num_anchors < 1) return fail(PNY_ERR_ARG, std::string(who) + "num_anchors must be at least 1");
    if (desc->num_classes < 1) return fail(PNY_ERR_ARG, std::string(who) + "num_classes must be at least 1");
    if (cells > (int64_t)INT32_MAX / desc->num_anchors)   // (the counts are int32)
        return fail(PNY_ERR_ARG, std::string(who) + "more than 2^31 - 1 (cell, anchor) pairs");
    YoloLossArgs a;
    a.pred = pred_dev, a.target = target_dev, a.anchors = anchors_dev;
    a.items = cells * desc->num_anchors, a.A = desc->num_anchors, a.C = desc->num_classes;
    a.w_box = desc->box_loss, a.w_obj = desc->object_loss, a.w_noobj = desc->no_object_loss, a.w_cls = desc->class_loss;
    a.terms = terms_dev, a.counts = counts_dev, a.d_pred = d_pred_dev;
    int rc;
    if ((rc = loss_workspace((hipStream_t)stream, &a.ticket, &a.partials))) return rc;
    launch_yolo_loss(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

// M and N of a mini-batch description, or PNY_ERR_ARG with a message that starts with `who`.
static int batches_geometry(const char* who, const pny_yolo_batches_desc* b, int64_t* n_rows) {
    if (!b) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (b->n_scales < 1 || b->n_scales > LOSS_MAX_SCALES) return fail(PNY_ERR_ARG, std::string(who) + "n_scales must be 1 .. 4");
    if (b->batch_rows <= 0) return fail(PNY_ERR_ARG, std::string(who) + "batch_rows must be positive");
    int64_t m = 0, n = 0;
    for (int s = 0; s < b->n_scales; ++s) {
        if (b->rows[s] <= 0) return fail(PNY_ERR_ARG, std::string(who) + "rows[" + std::to_string(s) + "] must be positive");
        if (b->rows[s] > (int64_t)INT32_MAX) return fail(PNY_ERR_ARG, std::string(who) + "more than 2^31 - 1 (row, anchor) pairs");
        m += b->rows[s] / b->batch_rows + (b->rows[s] % b->batch_rows != 0);
        n += b->rows[s];
        if (m > LOSS_MAX_SEGMENTS)
            return fail(PNY_ERR_ARG, std::string(who) + "more than " + std::to_string(LOSS_MAX_SEGMENTS) + " mini-batches");
    }
    if (n_rows) *n_rows = n;
    return (int)m;
}

int pny_yolo_loss_batches_count(const pny_yolo_batches_desc* batches) {
    return batches_geometry("pny_yolo_loss_batches_count: ", batches, nullptr);
}

int pny_yolo_loss_batches(const pny_yolo_loss_desc* desc, const pny_yolo_batches_desc* batches, const float* pred_dev,
                          const float* target_dev, const float* anchors_dev, float* terms_seg_dev, int32_t* counts_seg_dev,
                          float* step_dev, float* d_pred_dev, pny_stream stream) {
    const char* who = "pny_yolo_loss_batches: ";
    if (!desc || !batches || !pred_dev || !target_dev || !anchors_dev || !terms_seg_dev || !step_dev)
        return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    int64_t n_rows = 0;
    const int m = batches_geometry(who, batches, &n_rows);
    if (m < 0) return m;
    if (desc->num_anchors < 1) return fail(PNY_ERR_ARG, std::string(who) + "num_anchors must be at least 1");
    if (desc->num_classes < 1) return fail(PNY_ERR_ARG, std::string(who) + "num_classes must be at least 1");
    if (n_rows > (int64_t)INT32_MAX / desc->num_anchors)   // (the counts are int32)
        return fail(PNY_ERR_ARG, std::string(who) + "more than 2^31 - 1 (row, anchor) pairs");
    YoloBatchesArgs a;
    a.pred = pred_dev, a.target = target_dev, a.anchors = anchors_dev;
    a.n_scales = batches->n_scales, a.batch_rows = batches->batch_rows, a.segments = m;
    for (int s = 0; s < LOSS_MAX_SCALES; ++s) a.rows[s] = s < batches->n_scales ? batches->rows[s] : 0;
    a.A = desc->num_anchors, a.C = desc->num_classes;
    a.w_box = desc->box_loss, a.w_obj = desc->object_loss, a.w_noobj = desc->no_object_loss, a.w_cls = desc->class_loss;
    a.terms_seg = terms_seg_dev, a.counts_seg = counts_seg_dev, a.step = step_dev, a.d_pred = d_pred_dev;
    int rc;
    double* unused = nullptr;   // (the partial-sum table: the mini-batches' terms are their own table)
    if ((rc = loss_workspace((hipStream_t)stream, &a.ticket, &unused))) return rc;
    launch_yolo_loss_batches(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
