// Device arithmetic shared by the YOLO detection tail's kernels: the per-image ones of detect.hip (pny_cells_to_bboxes,
// pny_nms, pny_tp_fp_fn) and the batched scorer of detect_views.hip (pny_detect_views).  One copy of the box decode and of the
// IoU, so that the batched counts equal the per-view path's by construction.  Also the batched kernel's argument block and its
// LDS map, and the argument block of the threshold sweep (detect_sweep.hip, pny_detect_sweep), which runs the batched kernel's
// device code (pny_detect_views_core.h) at a grid of settings.
#pragma once
#include <string>

#include "pny_common.h"

namespace pny {

// iou(box1, box2) of reference util.py:576-611 (is_pred=True), [x, y, w, h] boxes, fp32 op for op.
__device__ __forceinline__ float iou_xywh(const float* a, const float* b) {
    const float a_x1 = a[0] - a[2] / 2.0f, a_y1 = a[1] - a[3] / 2.0f;
    const float a_x2 = a[0] + a[2] / 2.0f, a_y2 = a[1] + a[3] / 2.0f;
    const float b_x1 = b[0] - b[2] / 2.0f, b_y1 = b[1] - b[3] / 2.0f;
    const float b_x2 = b[0] + b[2] / 2.0f, b_y2 = b[1] + b[3] / 2.0f;
    const float x1 = fmaxf(a_x1, b_x1), y1 = fmaxf(a_y1, b_y1);
    const float x2 = fminf(a_x2, b_x2), y2 = fminf(a_y2, b_y2);
    const float inter = fmaxf(x2 - x1, 0.0f) * fmaxf(y2 - y1, 0.0f);
    const float area_a = fabsf((a_x2 - a_x1) * (a_y2 - a_y1));
    const float area_b = fabsf((b_x2 - b_x1) * (b_y2 - b_y1));
    const float uni = area_a + area_b - inter;
    return inter / (uni + 1e-6f);
}

// One cell of util.convert_cells_to_bboxes (reference util.py:633-689): c = the cell's 7 (predictions) or 6 (targets) floats,
// (x, y) its grid position, (aw, ah) its anchor, inv_w = 1 / grid width, inv_h = 1 / grid height -> o = [class, score, x, y, w, h].
__device__ __forceinline__ void cell_to_bbox(const float* c, int is_pred, int x, int y, float aw, float ah, float inv_w,
                                             float inv_h, float* o) {
    const int C = is_pred ? 7 : 6;
    float bx = c[1], by = c[2], bw = c[3], bh = c[4], cls;
    if (is_pred) {
        bx = 1.0f / (1.0f + expf(-bx));
        by = 1.0f / (1.0f + expf(-by));
        bw = expf(bw) * aw;
        bh = expf(bh) * ah;
        // torch.argmax over the class logits (first maximum wins)
        int best = 0;
        float bv = c[5];
        for (int k = 1; k < C - 5; ++k)
            if (c[5 + k] > bv) {
                bv = c[5 + k];
                best = k;
            }
        cls = (float)best;
    } else {
        cls = c[5];
    }
    o[0] = cls;
    o[1] = c[0];
    o[2] = inv_w * (bx + (float)x);
    o[3] = inv_h * (by + (float)y);
    o[4] = inv_w * bw;
    o[5] = inv_h * bh;
}

// The reference's confidence and size filters of nms() (util.py:693-700): Python floats, so doubles.
__device__ __forceinline__ bool conf_above(float score, double conf_thr) { return (double)score > conf_thr; }
__device__ __forceinline__ bool size_ok(float w, float h) {
    const double bw = (double)w, bh = (double)h;
    return 10e-4 < bw && bw < 10e4 && 10e-4 < bh && bh < 10e4;
}

// ------------------------------------------------------------------ pny_detect_views (detect_views.hip)
constexpr int DETECT_THREADS = 256;
constexpr int DETECT_WAVES = DETECT_THREADS / 64;
constexpr int DETECT_MAXC = PNY_DETECT_MAX_CANDIDATES;
enum { DETECT_TARGETS = 0, DETECT_PREDS = 1 };

// One of the two lists of every view, in either input form.
struct DetectList {
    const float* cells[PNY_YOLO_BATCH_MAX_SCALES];   // cells form: scale s is (V * hs * ws, A, 7 | 6), rows ordered (view, y, x)
    const float* rows;                               // boxes form: (n_rows, 6)
    const int32_t* offsets;                          // boxes form: V + 1 row offsets; view v owns rows [offsets[v], offsets[v + 1])
    int n_rows;
    float* kept;                                     // optional (V, max_kept, 6)
};

struct DetectViewsArgs {
    DetectList list[2];                              // DETECT_TARGETS, DETECT_PREDS
    int form, n_views, n_scales, n_anchors, max_kept;
    int cap;                                         // candidate slots of this launch's LDS map, <= DETECT_MAXC
    int hs[PNY_YOLO_BATCH_MAX_SCALES], ws[PNY_YOLO_BATCH_MAX_SCALES];
    float inv_w[PNY_YOLO_BATCH_MAX_SCALES], inv_h[PNY_YOLO_BATCH_MAX_SCALES];
    float anchors[PNY_YOLO_BATCH_MAX_SCALES][4][2];
    float nms_iou, match_iou;                        // rounded to fp32 once on the host, as the reference's tensors hold them
    double nms_thr;
    int32_t* per_view;                               // (V, PNY_DETECT_RECORD)
    float* highest_conf;                             // (V, 2): targets, predictions
    unsigned long long* totals;                      // 4 words: tp, fp, fn, failed views
};

// LDS map for `cap` candidate slots (53 bytes each: 108 544 at cap = 2048, plus 52 of scan words).  A candidate's slot is its
// rank in input order, which is all the stable sort needs of its original position:
//   cand   [cap][6] float   the list at hand: filtered boxes in input order
//   tkept  [cap][4] float   x, y, w, h of the kept targets, held while the predictions are processed
//   listA, listB [cap] int  candidate slots: sorted order, then the two buffers of the suppression rounds
//   kept   [cap]    int     candidate slots of the survivors, in the reference's output order
//   scan   [DETECT_WAVES + 1] int,  redf [DETECT_WAVES] float,  cnt [4] int
//   flag   [cap]    byte
constexpr size_t detect_lds_bytes(int cap) {
    return (size_t)cap * (6 + 4 + 1 + 1 + 1) * 4 + (size_t)(DETECT_WAVES + 1 + DETECT_WAVES + 4) * 4 + (size_t)cap;
}
static_assert(detect_lds_bytes(DETECT_MAXC) <= 160 * 1024, "PNY_DETECT_MAX_CANDIDATES must fit gfx950's 160 KB of LDS");

void launch_detect_views(const DetectViewsArgs& a, size_t lds_bytes, hipStream_t st);

// Host side of both entries (detect_views.hip): form and n_views; then geometry or rows, the eight input pointers and `cap`
// into *a.  PNY_OK, or PNY_ERR_ARG with pny_last_error = who + the field.
int detect_check_form(const std::string& who, const pny_detect_views_desc* desc);
int detect_fill_inputs(const std::string& who, const pny_detect_views_desc* desc, const float* const* preds_dev,
                       const float* const* targets_dev, const float* anchors_host, const float* pred_rows_dev,
                       const int32_t* pred_offsets_dev, const float* target_rows_dev, const int32_t* target_offsets_dev,
                       DetectViewsArgs* a);

// ------------------------------------------------------------------ pny_detect_sweep (detect_sweep.hip)
// The limits of a sweep (include/pnyolo.h states them in pny_detect_sweep's comment, lib.py as DETECT_SWEEP_MAX_*): they bound
// the thresholds that travel by value in the kernel arguments (8 + 8 floats, 32 doubles and 32 bytes: 352 bytes).
constexpr int DETECT_SWEEP_MAX_NMS_IOUS = 8, DETECT_SWEEP_MAX_CUTS = 32, DETECT_SWEEP_MAX_MATCH_IOUS = 8;

struct DetectSweepArgs {
    DetectViewsArgs in;                              // lists, geometry, cap, totals; its thresholds, per_view, highest_conf, kept unused
    int n_nms, n_cuts, n_match;                      // I, T, M
    float nms_ious[DETECT_SWEEP_MAX_NMS_IOUS];       // rounded to fp32 once on the host, as DetectViewsArgs::nms_iou
    float match_ious[DETECT_SWEEP_MAX_MATCH_IOUS];
    double cuts[DETECT_SWEEP_MAX_CUTS];              // compared in double, as DetectViewsArgs::nms_thr
    unsigned char cut_order[DETECT_SWEEP_MAX_CUTS];  // the cuts' indices, lowest cut first: the order in which the grid takes them
    int32_t* counts;                                 // (V, I, T, M, 3)
    int32_t* lists;                                  // (V, I, T, 3)
};

void launch_detect_sweep(const DetectSweepArgs& s, size_t lds_bytes, hipStream_t st);

}  // namespace pny
