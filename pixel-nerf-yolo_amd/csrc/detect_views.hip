// The detection scores of all views of a YOLO metric pass in one launch (include/pnyolo.h pny_detect_views): what
// YoloTrainer.metric_step (reference train/trainlib/YoloTrainer.py:338-354) does per destination view with Python lists --
// convert_cells_to_bboxes per scale, calculate_tp_fp_fn, three running sums -- for V views at once, one workgroup per view,
// nothing decoded to global memory, no allocation, no host read.  The per-image kernels of detect.hip stay the reference's
// per-view interface; the decode and the IoU are one copy of device code (pny_detect.h), the list semantics are nms_kernel's
// and match_kernel's restated on LDS-resident candidates, so the counts are the per-view path's.
//
// Per list (targets, then predictions) of a view:
//   1. stream the view's cells (scale by scale, (y, x, anchor) within a scale) or rows 256 at a time: decode, filter, block scan,
//      compact the survivors into LDS in input order; running maximum of ALL scores and the count above the threshold;
//   2. rank sort by descending confidence, the candidate slot (= input order) breaking ties;
//   3. greedy suppression with the reference's remove-while-iterating semantics (detect.hip nms_kernel);
//   4. targets: park x, y, w, h of the survivors in LDS; predictions: match the two lists (detect.hip match_kernel);
//   5. the view's record, and integer atomic adds into the totals.
#include <cmath>

#include "dev_resource.h"
#include "pny_detect.h"

namespace pny {

namespace {

struct Lds {
    float* cand;
    float* tkept;
    int* listA;
    int* listB;
    int* kept;
    int* scan;
    float* redf;
    int* cnt;
    unsigned char* flag;
};

__device__ __forceinline__ Lds carve(int* base, int cap) {
    Lds l;
    l.cand = reinterpret_cast<float*>(base);
    l.tkept = l.cand + (size_t)cap * 6;
    l.listA = reinterpret_cast<int*>(l.tkept + (size_t)cap * 4);
    l.listB = l.listA + cap;
    l.kept = l.listB + cap;
    l.scan = l.kept + cap;
    l.redf = reinterpret_cast<float*>(l.scan + DETECT_WAVES + 1);
    l.cnt = reinterpret_cast<int*>(l.redf + DETECT_WAVES);
    l.flag = reinterpret_cast<unsigned char*>(l.cnt + 4);
    return l;
}

// Exclusive scan of one int per thread over the workgroup: the thread's offset, and the workgroup's sum in *total.
// scan: DETECT_WAVES ints of LDS, free again on return.
__device__ __forceinline__ int block_scan(int v, int* scan, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) scan[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < DETECT_WAVES; ++w) {
        const int s = scan[w];
        base += w < wave ? s : 0;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// Order-preserving compaction of src[0, m) by keep[] into dst; returns the number kept (detect.hip block_compact, with the
// scan across the workgroup done in registers).
__device__ int compact(const int* src, const unsigned char* keep, int m, int* dst, int* scan) {
    const int per = (m + DETECT_THREADS - 1) / DETECT_THREADS;
    const int lo = min(m, (int)threadIdx.x * per), hi = min(m, lo + per);
    int c = 0;
    for (int p = lo; p < hi; ++p) c += keep[p] ? 1 : 0;
    int total;
    int o = block_scan(c, scan, &total);
    for (int p = lo; p < hi; ++p)
        if (keep[p]) dst[o++] = src[p];
    __syncthreads();
    return total;
}

// Number of boxes of view v's list, or -1 for a segment that does not lie inside the rows (boxes form).
__device__ __forceinline__ int list_length(const DetectViewsArgs& a, int which, int v, int* first_row) {
    *first_row = 0;
    if (a.form == PNY_DETECT_CELLS) {
        int n = 0;
        for (int s = 0; s < a.n_scales; ++s) n += a.hs[s] * a.ws[s] * a.n_anchors;
        return n;
    }
    const DetectList& l = a.list[which];
    const int lo = l.offsets[v], hi = l.offsets[v + 1];
    if (lo < 0 || hi < lo || hi > l.n_rows) return -1;
    *first_row = lo;
    return hi - lo;
}

// Box i of view v's list -> o[6] = [class, score, x, y, w, h].
__device__ __forceinline__ void load_box(const DetectViewsArgs& a, int which, int v, int first_row, int i, float* o) {
    const DetectList& l = a.list[which];
    if (a.form == PNY_DETECT_BOXES) {
        const float* r = l.rows + (size_t)(first_row + i) * 6;
        for (int k = 0; k < 6; ++k) o[k] = r[k];
        return;
    }
    int s = 0, j = i;
    while (s + 1 < a.n_scales && j >= a.hs[s] * a.ws[s] * a.n_anchors) {
        j -= a.hs[s] * a.ws[s] * a.n_anchors;
        ++s;
    }
    const int na = a.n_anchors, w = a.ws[s], per_view = a.hs[s] * w * na;
    const int an = j % na, x = (j / na) % w, y = j / (na * w);
    const int is_pred = which == DETECT_PREDS;
    const float* c = l.cells[s] + ((size_t)v * per_view + j) * (is_pred ? 7 : 6);
    cell_to_bbox(c, is_pred, x, y, a.anchors[s][an][0], a.anchors[s][an][1], a.inv_w[s], a.inv_h[s], o);
}

// Phase 1.  Returns the number of candidates (which may exceed a.cap: then only the first a.cap are in LDS and the caller
// refuses the view); *above = boxes above the confidence threshold, *highest = the maximum score of all n boxes.
__device__ int decode_filter(const DetectViewsArgs& a, const Lds& l, int which, int v, int first_row, int n, int* above,
                             float* highest) {
    const int tid = threadIdx.x;
    int m = 0, ab = 0;
    float mx = -INFINITY;
    for (long long c0 = 0; c0 < n; c0 += DETECT_THREADS) {
        const long long i = c0 + tid;
        float b[6];
        bool ok = false;
        if (i < n) {
            load_box(a, which, v, first_row, (int)i, b);
            mx = fmaxf(mx, b[1]);
            const bool conf_ok = conf_above(b[1], a.nms_thr);
            ab += conf_ok ? 1 : 0;
            ok = conf_ok && size_ok(b[4], b[5]);
        }
        int tot;
        const int slot = m + block_scan(ok ? 1 : 0, l.scan, &tot);
        if (ok && slot < a.cap)
            for (int k = 0; k < 6; ++k) l.cand[(size_t)slot * 6 + k] = b[k];
        m += tot;                                    // <= n: never wraps
    }
    for (int d = 32; d > 0; d >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, d, 64));
        ab += __shfl_xor(ab, d, 64);
    }
    if ((tid & 63) == 0) {
        l.redf[tid >> 6] = mx;
        l.scan[tid >> 6] = ab;
    }
    __syncthreads();
    mx = -INFINITY, ab = 0;
    for (int w = 0; w < DETECT_WAVES; ++w) {
        mx = fmaxf(mx, l.redf[w]);
        ab += l.scan[w];
    }
    __syncthreads();
    *above = ab;
    *highest = mx;
    return m;
}

// Phases 2 and 3 on the m candidates in l.cand.  Leaves the survivors' slots in l.kept in the reference's output order and
// returns their number; copies the first max_kept rows to out (may be null).
__device__ int sort_suppress(const Lds& l, int m, float iou_thr, float* out, int max_kept) {
    const int tid = threadIdx.x;
    // stable sort by confidence, descending (Python sorted(..., reverse=True) keeps input order on ties)
    for (int p = tid; p < m; p += DETECT_THREADS) {
        const float ci = l.cand[(size_t)p * 6 + 1];
        int rank = 0;
        for (int q = 0; q < m; ++q) {
            const float cq = l.cand[(size_t)q * 6 + 1];
            rank += (cq > ci || (cq == ci && q < p)) ? 1 : 0;
        }
        l.listA[rank] = p;
    }
    __syncthreads();

    // greedy suppression with the reference's list semantics (util.py:709-720), as detect.hip nms_kernel
    int* cur = l.listA;
    int* nxt = l.listB;
    unsigned char* flag = l.flag;
    int n_out = 0;
    while (m > 0) {
        const int first = cur[0];
        if (tid == 0) l.kept[n_out] = first;
        if (out && n_out < max_kept && tid < 6) out[(size_t)n_out * 6 + tid] = l.cand[(size_t)first * 6 + tid];
        ++n_out;
        const float* fb = l.cand + (size_t)first * 6 + 2;
        for (int p = 1 + tid; p < m; p += DETECT_THREADS)
            flag[p] = iou_xywh(fb, l.cand + (size_t)cur[p] * 6 + 2) > iou_thr ? 1 : 0;
        __syncthreads();
        if (tid == 0) {
            // `for box in lst: if ...: lst.remove(box)`: removing shifts the tail left under the iterator, so the element after
            // a removed one is never examined in this round; `lst.remove(box)` deletes the FIRST element that compares equal: an
            // identical row further up that the iterator skipped goes instead of the row at hand.  Rows are sorted by
            // confidence, so such a twin sits in the run of equal confidences right above.
            flag[0] = 0;
            int p = 1;
            while (p < m) {
                if (flag[p]) {
                    int drop = p;
                    const float* bp = l.cand + (size_t)cur[p] * 6;
                    for (int q = p - 1; q >= 1; --q) {
                        const float* bq = l.cand + (size_t)cur[q] * 6;
                        if (bq[1] != bp[1]) break;
                        // position q is still in the list iff it was kept so far in this round (flag 1 = keep, set below)
                        if (flag[q] == 1 && bq[0] == bp[0] && bq[2] == bp[2] && bq[3] == bp[3] && bq[4] == bp[4] && bq[5] == bp[5])
                            drop = q;
                    }
                    flag[p] = 1;
                    flag[drop] = 0;  // 0 = drop
                    if (p + 1 < m) flag[p + 1] = 1;
                    p += 2;
                } else {
                    flag[p] = 1;  // 1 = keep
                    p += 1;
                }
            }
        }
        __syncthreads();
        m = compact(cur, flag, m, nxt, l.scan);
        int* t = cur;
        cur = nxt;
        nxt = t;
    }
    __syncthreads();
    return n_out;
}

__global__ __launch_bounds__(DETECT_THREADS) void detect_views_kernel(const DetectViewsArgs a) {
    extern __shared__ int lds_detect[];
    const Lds l = carve(lds_detect, a.cap);
    const int tid = threadIdx.x, v = blockIdx.x;
    int status = 0;
    int n[2], first_row[2], above[2] = {0, 0}, n_kept[2] = {0, 0};
    float highest[2] = {-INFINITY, -INFINITY};
    for (int which = 0; which < 2; ++which) {
        n[which] = list_length(a, which, v, &first_row[which]);
        if (n[which] < 0) {
            n[which] = 0;
            status |= PNY_DETECT_BAD_SEGMENT;
        }
    }
    if (tid < 4) l.cnt[tid] = 0;
    for (int which = DETECT_TARGETS; which <= DETECT_PREDS; ++which) {
        const int m = decode_filter(a, l, which, v, first_row[which], n[which], &above[which], &highest[which]);
        if (m > a.cap) status |= which == DETECT_TARGETS ? PNY_DETECT_TARGETS_OVERFLOW : PNY_DETECT_PREDS_OVERFLOW;
        if (status) continue;
        float* out = a.list[which].kept ? a.list[which].kept + (size_t)v * a.max_kept * 6 : nullptr;
        n_kept[which] = sort_suppress(l, m, a.nms_iou, out, a.max_kept);
        if (which == DETECT_TARGETS) {
            for (int k = tid; k < n_kept[which]; k += DETECT_THREADS)
                for (int j = 0; j < 4; ++j) l.tkept[(size_t)k * 4 + j] = l.cand[(size_t)l.kept[k] * 6 + 2 + j];
            __syncthreads();
        }
    }
    if (status) n_kept[0] = n_kept[1] = 0;
    const int nt = n_kept[0], np = n_kept[1];
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
        rec[5] = above[0];
        rec[6] = above[1];
        rec[7] = status;
        a.highest_conf[(size_t)v * 2] = highest[0];
        a.highest_conf[(size_t)v * 2 + 1] = highest[1];
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
    if (desc->form != PNY_DETECT_CELLS && desc->form != PNY_DETECT_BOXES)
        return fail(PNY_ERR_ARG, who + "form must be PNY_DETECT_CELLS or PNY_DETECT_BOXES, got " + std::to_string(desc->form));
    if (desc->n_views < 1) return fail(PNY_ERR_ARG, who + "n_views must be at least 1, got " + std::to_string(desc->n_views));
    if (desc->max_kept < 0 || ((kept_targets_dev || kept_preds_dev) && desc->max_kept < 1))
        return fail(PNY_ERR_ARG, who + "max_kept must be at least 1 with a kept-box output (and never negative), got " +
                                     std::to_string(desc->max_kept));
    if (!std::isfinite(desc->nms_iou) || !std::isfinite(desc->nms_threshold) || !std::isfinite(desc->match_iou))
        return fail(PNY_ERR_ARG, who + "nms_iou, nms_threshold and match_iou must be finite");
    DetectViewsArgs a = {};
    a.form = desc->form, a.n_views = desc->n_views, a.max_kept = desc->max_kept;
    a.nms_iou = (float)desc->nms_iou, a.match_iou = (float)desc->match_iou, a.nms_thr = desc->nms_threshold;
    a.per_view = per_view_dev, a.highest_conf = highest_conf_dev;
    a.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    a.list[DETECT_TARGETS].kept = kept_targets_dev, a.list[DETECT_PREDS].kept = kept_preds_dev;
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
