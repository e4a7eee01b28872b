// The device code that the one-setting scorer (detect_views.hip, pny_detect_views) and the threshold sweep (detect_sweep.hip,
// pny_detect_sweep) share: a workgroup of DETECT_THREADS turns the two lists of one view, at ONE confidence cut and ONE NMS IoU,
// into the reference's kept lists in LDS.  One copy, so that a sweep's setting gives the integers of the one-setting call by
// construction.  Included by those two files only; the LDS map is pny_detect.h detect_lds_bytes.
//
// Per list (targets, then predictions) of a view:
//   1. stream the view's cells (scale by scale, (y, x, anchor) within a scale) or rows 256 at a time: decode, filter, block scan,
//      compact the survivors into LDS in input order; running maximum of ALL scores and the count above the threshold;
//   2. rank sort by descending confidence, the candidate slot (= input order) breaking ties;
//   3. greedy suppression with the reference's remove-while-iterating semantics (detect.hip nms_kernel);
//   4. targets: park x, y, w, h of the survivors in LDS.
#pragma once
#include <cmath>

#include "pny_detect.h"

namespace pny {

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
__device__ inline int compact(const int* src, const unsigned char* keep, int m, int* dst, int* scan) {
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

// Phase 1 at the confidence cut conf_thr.  Returns the number of candidates (which may exceed a.cap: then only the first a.cap
// are in LDS and the caller refuses the view); *above = boxes above the cut, *highest = the maximum score of all n boxes.
__device__ inline int decode_filter(const DetectViewsArgs& a, const Lds& l, int which, int v, int first_row, int n, double conf_thr,
                                    int* above, float* highest) {
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
            const bool conf_ok = conf_above(b[1], conf_thr);
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
__device__ inline int sort_suppress(const Lds& l, int m, float iou_thr, float* out, int max_kept) {
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

// What suppress_view leaves of view v at one (confidence cut, NMS IoU): the slots of the kept predictions in l.kept (their rows
// in l.cand), x, y, w, h of the kept targets in l.tkept, and this.  A refused view (status != 0) has kept nothing.
struct ViewLists {
    int status;            // 0, or PNY_DETECT_* bits
    int n_kept[2];         // DETECT_TARGETS, DETECT_PREDS
    int above[2];
    float highest[2];
};

// Phases 1 - 4 for both lists of view v.  The first max_kept kept rows of a list go to a.list[which].kept when that is given.
__device__ inline ViewLists suppress_view(const DetectViewsArgs& a, const Lds& l, int v, double conf_thr, float nms_iou) {
    const int tid = threadIdx.x;
    ViewLists r = {0, {0, 0}, {0, 0}, {-INFINITY, -INFINITY}};
    int n[2], first_row[2];
    for (int which = 0; which < 2; ++which) {
        n[which] = list_length(a, which, v, &first_row[which]);
        if (n[which] < 0) {
            n[which] = 0;
            r.status |= PNY_DETECT_BAD_SEGMENT;
        }
    }
    for (int which = DETECT_TARGETS; which <= DETECT_PREDS; ++which) {
        const int m = decode_filter(a, l, which, v, first_row[which], n[which], conf_thr, &r.above[which], &r.highest[which]);
        if (m > a.cap) r.status |= which == DETECT_TARGETS ? PNY_DETECT_TARGETS_OVERFLOW : PNY_DETECT_PREDS_OVERFLOW;
        if (r.status) continue;
        float* out = a.list[which].kept ? a.list[which].kept + (size_t)v * a.max_kept * 6 : nullptr;
        r.n_kept[which] = sort_suppress(l, m, nms_iou, out, a.max_kept);
        if (which == DETECT_TARGETS) {
            for (int k = tid; k < r.n_kept[which]; k += DETECT_THREADS)
                for (int j = 0; j < 4; ++j) l.tkept[(size_t)k * 4 + j] = l.cand[(size_t)l.kept[k] * 6 + 2 + j];
            __syncthreads();
        }
    }
    if (r.status) r.n_kept[0] = r.n_kept[1] = 0;
    return r;
}

}  // namespace pny
