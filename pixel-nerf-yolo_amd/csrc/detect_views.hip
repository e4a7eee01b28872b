// The detection scores of all views of a YOLO metric pass in one launch (include/pnyolo.h pny_detect_views): what
// YoloTrainer.metric_step (reference train/trainlib/YoloTrainer.py:338-354) does per destination view with Python lists --
// convert_cells_to_bboxes per scale, calculate_tp_fp_fn, three running sums -- for V views at once, one workgroup per view,
// nothing decoded to global memory, no allocation, no host read.  The per-image kernels of detect.hip stay the reference's
// per-view interface; the decode and the IoU are one copy of device code (pny_detect.h), the list semantics are nms_kernel's
// and match_kernel's restated on LDS-resident candidates, so the counts are the per-view path's.  Steps 1 - 3 and the parking of
// the kept targets are pny_detect_views_core.h suppress_view, which the threshold sweep (detect_sweep.hip) runs too.
//
// Per list (targets, then predictions) of a view:
//   1. stream the view's cells (scale by scale, (y, x, anchor) within a scale) or rows 256 at a time: decode, filter, block scan,
//      compact the survivors into LDS in input order; running maximum of ALL scores and the count above the threshold;
//   2. rank sort by descending confidence, the candidate slot (= input order) breaking ties;
//   3. greedy suppression with the reference's remove-while-iterating semantics (detect.hip nms_kernel);
//   4. targets: park x, y, w, h of the survivors in LDS; predictions: match the two lists (detect.hip match_kernel);
//   5. the view's record, and integer atomic adds into the totals.
#include "dev_resource.h"
#include "pny_detect.h"
#include "pny_detect_views_core.h"

namespace pny {

namespace {

__global__ __launch_bounds__(DETECT_THREADS) void detect_views_kernel(const DetectViewsArgs a) {
    extern __shared__ int lds_detect[];
    const Lds l = carve(lds_detect, a.cap);
    const int tid = threadIdx.x, v = blockIdx.x;
    if (tid < 4) l.cnt[tid] = 0;
    const ViewLists r = suppress_view(a, l, v, a.nms_thr, a.nms_iou);
    const int status = r.status, nt = r.n_kept[0], np = r.n_kept[1];
    // reference util.py:779-802 on the two suppressed lists, as detect.hip match_kernel
    if (!status) {
        if (nt == 0) {
            if (tid == 0) l.cnt[1] = np;
        } else if (np == 0) {
            if (tid == 0) l.cnt[2] = nt;
        } else {
            for (int p = tid; p < np; p += DETECT_THREADS) {
                const float* pb = l.cand + (size_t)l.kept[p] * 6 + 2;
                float best = -INFINITY;
                for (int t = 0; t < nt; ++t) best = fmaxf(best, iou_xywh(pb, l.tkept + (size_t)t * 4));
                atomicAdd(&l.cnt[best > a.match_iou ? 0 : 1], 1);
            }
            for (int t = tid; t < nt; t += DETECT_THREADS) {
                const float* tb = l.tkept + (size_t)t * 4;
                float best = -INFINITY;
                for (int p = 0; p < np; ++p) best = fmaxf(best, iou_xywh(tb, l.cand + (size_t)l.kept[p] * 6 + 2));
                if (best < a.match_iou) atomicAdd(&l.cnt[2], 1);
            }
        }
    }
    __syncthreads();
    int32_t* rec = a.per_view + (size_t)v * PNY_DETECT_RECORD;
    if (tid < 3) {
        rec[tid] = l.cnt[tid];
        if (!status) atomicAdd(a.totals + tid, (unsigned long long)l.cnt[tid]);
    } else if (tid == 3) {
        rec[3] = nt;
        rec[4] = np;
        rec[5] = r.above[0];
        rec[6] = r.above[1];
        rec[7] = status;
        a.highest_conf[(size_t)v * 2] = r.highest[0];
        a.highest_conf[(size_t)v * 2 + 1] = r.highest[1];
        if (status) atomicAdd(a.totals + 3, 1ull);
    }
}

}  // namespace

void launch_detect_views(const DetectViewsArgs& a, size_t lds_bytes, hipStream_t st) {
    hipLaunchKernelGGL(detect_views_kernel, dim3(a.n_views), dim3(DETECT_THREADS), lds_bytes, st, a);
}

hipError_t detect_views_lds_limit(size_t lds_bytes) {
    static LdsLimit limit;
    return limit.raise(lds_bytes, detect_views_kernel);
}

// The checks and the argument block that pny_detect_views and pny_detect_sweep share (declared in pny_detect.h): first the form
// and the view count, then -- behind the caller's own checks -- the geometry or the rows, the input pointers and the LDS map.
int detect_check_form(const std::string& who, const pny_detect_views_desc* desc) {
    if (desc->form != PNY_DETECT_CELLS && desc->form != PNY_DETECT_BOXES)
        return fail(PNY_ERR_ARG, who + "form must be PNY_DETECT_CELLS or PNY_DETECT_BOXES, got " + std::to_string(desc->form));
    if (desc->n_views < 1) return fail(PNY_ERR_ARG, who + "n_views must be at least 1, got " + std::to_string(desc->n_views));
    return PNY_OK;
}

int detect_fill_inputs(const std::string& who, const pny_detect_views_desc* desc, const float* const* preds_dev,
                       const float* const* targets_dev, const float* anchors_host, const float* pred_rows_dev,
                       const int32_t* pred_offsets_dev, const float* target_rows_dev, const int32_t* target_offsets_dev,
                       DetectViewsArgs* args) {
    DetectViewsArgs& a = *args;
    a.form = desc->form, a.n_views = desc->n_views;
    int64_t longest = 0;
    if (desc->form == PNY_DETECT_CELLS) {
        if (desc->n_scales < 1 || desc->n_scales > PNY_YOLO_BATCH_MAX_SCALES)
            return fail(PNY_ERR_ARG, who + "n_scales must be 1 .. 4, got " + std::to_string(desc->n_scales));
        if (desc->n_anchors < 1 || desc->n_anchors > 4)
            return fail(PNY_ERR_ARG, who + "n_anchors must be 1 .. 4, got " + std::to_string(desc->n_anchors));
        if (desc->height < 1 || desc->width < 1) return fail(PNY_ERR_ARG, who + "height and width must be positive");
        if (!preds_dev || !targets_dev || !anchors_host)
            return fail(PNY_ERR_ARG, who + "preds_dev, targets_dev and anchors_host are required in the cells form");
        a.n_scales = desc->n_scales, a.n_anchors = desc->n_anchors;
        for (int s = 0; s < desc->n_scales; ++s) {
            const int cell = desc->cell_sizes[s];
            if (cell < 1 || cell > desc->height || cell > desc->width)
                return fail(PNY_ERR_ARG, who + "cell_sizes[" + std::to_string(s) + "] = " + std::to_string(cell) +
                                             " must be 1 .. min(height, width)");
            if (!preds_dev[s] || !targets_dev[s])
                return fail(PNY_ERR_ARG, who + "preds_dev[" + std::to_string(s) + "] or targets_dev[" + std::to_string(s) + "] is NULL");
            a.hs[s] = desc->height / cell, a.ws[s] = desc->width / cell;
            // 1/w as the reference forms it: Python double 1/w rounded to fp32 (pny_cells_to_bboxes)
            a.inv_w[s] = (float)(1.0 / (double)a.ws[s]), a.inv_h[s] = (float)(1.0 / (double)a.hs[s]);
            for (int k = 0; k < desc->n_anchors; ++k) {
                a.anchors[s][k][0] = anchors_host[(s * desc->n_anchors + k) * 2];
                a.anchors[s][k][1] = anchors_host[(s * desc->n_anchors + k) * 2 + 1];
            }
            a.list[DETECT_PREDS].cells[s] = preds_dev[s], a.list[DETECT_TARGETS].cells[s] = targets_dev[s];
            longest += (int64_t)a.hs[s] * a.ws[s] * desc->n_anchors;
        }
        if (longest >= ((int64_t)1 << 31) - DETECT_THREADS)
            return fail(PNY_ERR_ARG, who + "a view of 2^31 or more cells");
    } else {
        if (desc->n_pred_rows < 0 || desc->n_target_rows < 0)
            return fail(PNY_ERR_ARG, who + "n_pred_rows and n_target_rows must not be negative");
        if (!pred_offsets_dev || !target_offsets_dev) return fail(PNY_ERR_ARG, who + "pred_offsets_dev or target_offsets_dev is NULL");
        if ((desc->n_pred_rows > 0 && !pred_rows_dev) || (desc->n_target_rows > 0 && !target_rows_dev))
            return fail(PNY_ERR_ARG, who + "pred_rows_dev or target_rows_dev is NULL");
        a.list[DETECT_PREDS].rows = pred_rows_dev, a.list[DETECT_PREDS].offsets = pred_offsets_dev;
        a.list[DETECT_PREDS].n_rows = desc->n_pred_rows;
        a.list[DETECT_TARGETS].rows = target_rows_dev, a.list[DETECT_TARGETS].offsets = target_offsets_dev;
        a.list[DETECT_TARGETS].n_rows = desc->n_target_rows;
        longest = desc->n_pred_rows > desc->n_target_rows ? desc->n_pred_rows : desc->n_target_rows;
    }
    // no list can hold more candidates than boxes: a short pass takes a short LDS map
    a.cap = (int)(longest < 1 ? 1 : longest < DETECT_MAXC ? longest : DETECT_MAXC);
    return PNY_OK;
}

}  // namespace pny

using namespace pny;

extern "C" {

int pny_detect_views(const pny_detect_views_desc* desc, const float* const* preds_dev, const float* const* targets_dev,
                     const float* anchors_host, const float* pred_rows_dev, const int32_t* pred_offsets_dev,
                     const float* target_rows_dev, const int32_t* target_offsets_dev, int32_t* per_view_dev,
                     float* highest_conf_dev, int64_t* totals_dev, float* kept_targets_dev, float* kept_preds_dev,
                     pny_stream stream) {
    const std::string who = "pny_detect_views: ";
    if (!desc) return fail(PNY_ERR_ARG, who + "desc is NULL");
    if (!per_view_dev) return fail(PNY_ERR_ARG, who + "per_view_dev is NULL");
    if (!highest_conf_dev) return fail(PNY_ERR_ARG, who + "highest_conf_dev is NULL");
    if (!totals_dev) return fail(PNY_ERR_ARG, who + "totals_dev is NULL");
    if (const int rc = detect_check_form(who, desc)) return rc;
    if (desc->max_kept < 0 || ((kept_targets_dev || kept_preds_dev) && desc->max_kept < 1))
        return fail(PNY_ERR_ARG, who + "max_kept must be at least 1 with a kept-box output (and never negative), got " +
                                     std::to_string(desc->max_kept));
    if (!std::isfinite(desc->nms_iou) || !std::isfinite(desc->nms_threshold) || !std::isfinite(desc->match_iou))
        return fail(PNY_ERR_ARG, who + "nms_iou, nms_threshold and match_iou must be finite");
    DetectViewsArgs a = {};
    a.max_kept = desc->max_kept;
    a.nms_iou = (float)desc->nms_iou, a.match_iou = (float)desc->match_iou, a.nms_thr = desc->nms_threshold;
    a.per_view = per_view_dev, a.highest_conf = highest_conf_dev;
    a.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    a.list[DETECT_TARGETS].kept = kept_targets_dev, a.list[DETECT_PREDS].kept = kept_preds_dev;
    const int rc = detect_fill_inputs(who, desc, preds_dev, targets_dev, anchors_host, pred_rows_dev, pred_offsets_dev, target_rows_dev,
                                      target_offsets_dev, &a);
    if (rc != PNY_OK) return rc;
    const size_t lds = detect_lds_bytes(a.cap);
    const hipError_t e = detect_views_lds_limit(lds);
    if (e != hipSuccess) {  // refuse here, not through the launch that would fail next
        (void)hipGetLastError();
        set_error(who + std::to_string(lds) + " bytes of dynamic LDS and the device refused that limit (" + hipGetErrorString(e) + ")");
        return PNY_ERR_HIP;
    }
    launch_detect_views(a, lds, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
