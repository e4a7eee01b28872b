// A YOLO metric pass's three thresholds swept in one launch (include/pnyolo.h pny_detect_sweep): the counts of
// pny_detect_views at every setting of a grid confidence cut x NMS IoU x match IoU, on lists that are decoded from a render
// made once.  The reference finds its thresholds by running the whole pass again per setting (eval/gen_images_yolo.py:110-117
// asks for them on stdin; eval/eval_yolo.py reports one setting per pass over the test loader).
//
// The reference's suppression removes rows while it iterates, so the kept lists at one (cut, NMS IoU) do not follow from those
// at another: one workgroup per (view, NMS IoU i, cut t) runs pny_detect_views_core.h suppress_view -- the device code of
// detect_views_kernel, one copy -- in the same LDS map.  The match IoU only enters the final comparison: the best IoU of every
// kept prediction over the kept targets and of every kept target over the kept predictions is computed once and compared with
// all M match IoUs in registers (reference util.py:776-797, as detect.hip match_kernel restates it).
#include <algorithm>

#include "dev_resource.h"
#include "pny_detect.h"
#include "pny_detect_views_core.h"

namespace pny {

namespace {

// The workgroup's sum of one int per thread, in every thread.  red: 2 * DETECT_WAVES words of LDS (l.scan, l.redf), free on return.
__device__ __forceinline__ void block_sum2(int& x, int& y, int* red) {
    for (int d = 32; d > 0; d >>= 1) {
        x += __shfl_xor(x, d, 64);
        y += __shfl_xor(y, d, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave] = x;
        red[DETECT_WAVES + wave] = y;
    }
    __syncthreads();
    x = y = 0;
    for (int w = 0; w < DETECT_WAVES; ++w) {
        x += red[w];
        y += red[DETECT_WAVES + w];
    }
    __syncthreads();
}

__global__ __launch_bounds__(DETECT_THREADS) void detect_sweep_kernel(const DetectSweepArgs s) {
    extern __shared__ int lds_sweep[];
    const DetectViewsArgs& a = s.in;
    const Lds l = carve(lds_sweep, a.cap);
    const int tid = threadIdx.x;
    // The lowest cut first: it passes the most boxes and its serial suppression walk is the longest of the grid.  Workgroups
    // start in grid order, one per compute unit, so a grid of more workgroups than units ends with its shortest walks.
    const int per_cut = a.n_views * s.n_nms, rest = blockIdx.x % per_cut;
    const int t = s.cut_order[blockIdx.x / per_cut], i = rest % s.n_nms, v = rest / s.n_nms;
    const ViewLists r = suppress_view(a, l, v, s.cuts[t], s.nms_ious[i]);
    const int nt = r.n_kept[0], np = r.n_kept[1];

    // tp[m]: this thread's kept predictions whose best IoU is above match IoU m; fn[m]: its kept targets whose best is below
    int tp[DETECT_SWEEP_MAX_MATCH_IOUS], fn[DETECT_SWEEP_MAX_MATCH_IOUS];
#pragma unroll
    for (int m = 0; m < DETECT_SWEEP_MAX_MATCH_IOUS; ++m) tp[m] = fn[m] = 0;
    if (nt > 0 && np > 0) {
        for (int p = tid; p < np; p += DETECT_THREADS) {
            const float* pb = l.cand + (size_t)l.kept[p] * 6 + 2;
            float best = -INFINITY;
            for (int k = 0; k < nt; ++k) best = fmaxf(best, iou_xywh(pb, l.tkept + (size_t)k * 4));
#pragma unroll
            for (int m = 0; m < DETECT_SWEEP_MAX_MATCH_IOUS; ++m) tp[m] += best > s.match_ious[m] ? 1 : 0;
        }
        for (int k = tid; k < nt; k += DETECT_THREADS) {
            const float* tb = l.tkept + (size_t)k * 4;
            float best = -INFINITY;
            for (int p = 0; p < np; ++p) best = fmaxf(best, iou_xywh(tb, l.cand + (size_t)l.kept[p] * 6 + 2));
#pragma unroll
            for (int m = 0; m < DETECT_SWEEP_MAX_MATCH_IOUS; ++m) fn[m] += best < s.match_ious[m] ? 1 : 0;
        }
    }
    const size_t setting = (size_t)i * s.n_cuts + t, record = ((size_t)v * s.n_nms + i) * s.n_cuts + t;
    int32_t* counts = s.counts + record * s.n_match * 3;
    unsigned long long* totals = a.totals + setting * s.n_match * 4;
#pragma unroll
    for (int m = 0; m < DETECT_SWEEP_MAX_MATCH_IOUS; ++m) {
        if (m >= s.n_match) break;                   // uniform over the workgroup
        int n_tp = tp[m], n_fn = fn[m];
        block_sum2(n_tp, n_fn, l.scan);              // l.scan and l.redf are contiguous: 2 * DETECT_WAVES + 1 words
        if (tid == 0) {
            // no kept target: every kept prediction is a false positive; no kept prediction: every kept target a false negative
            const int c[3] = {n_tp, np - n_tp, np == 0 ? nt : n_fn};
            for (int k = 0; k < 3; ++k) {
                counts[m * 3 + k] = c[k];
                if (c[k]) atomicAdd(totals + m * 4 + k, (unsigned long long)c[k]);
            }
            if (r.status) atomicAdd(totals + m * 4 + 3, 1ull);
        }
    }
    if (tid == 0) {
        int32_t* rec = s.lists + record * 3;
        rec[0] = nt;
        rec[1] = np;
        rec[2] = r.status;
    }
}

}  // namespace

void launch_detect_sweep(const DetectSweepArgs& s, size_t lds_bytes, hipStream_t st) {
    const unsigned grid = (unsigned)s.in.n_views * (unsigned)(s.n_nms * s.n_cuts);
    hipLaunchKernelGGL(detect_sweep_kernel, dim3(grid), dim3(DETECT_THREADS), lds_bytes, st, s);
}

hipError_t detect_sweep_lds_limit(size_t lds_bytes) {
    static LdsLimit limit;
    return limit.raise(lds_bytes, detect_sweep_kernel);
}

}  // namespace pny

using namespace pny;

namespace {

// n values of one threshold list: 1 .. most of them, all finite.
int check_thresholds(const std::string& who, const char* name, const double* values, int32_t n, int most) {
    const std::string count = std::string("n_") + name;
    if (n < 1 || n > most)
        return fail(PNY_ERR_ARG, who + count + " must be 1 .. " + std::to_string(most) + ", got " + std::to_string(n));
    if (!values) return fail(PNY_ERR_ARG, who + name + "_host is NULL");
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(values[k])) return fail(PNY_ERR_ARG, who + name + "_host[" + std::to_string(k) + "] must be finite");
    return PNY_OK;
}

}  // namespace

extern "C" {

int pny_detect_sweep(const pny_detect_views_desc* desc, const float* const* preds_dev, const float* const* targets_dev,
                     const float* anchors_host, const float* pred_rows_dev, const int32_t* pred_offsets_dev,
                     const float* target_rows_dev, const int32_t* target_offsets_dev, const double* nms_ious_host,
                     int32_t n_nms_ious, const double* conf_cuts_host, int32_t n_conf_cuts, const double* match_ious_host,
                     int32_t n_match_ious, int32_t* counts_dev, int32_t* lists_dev, int64_t* totals_dev, pny_stream stream) {
    const std::string who = "pny_detect_sweep: ";
    if (!desc) return fail(PNY_ERR_ARG, who + "desc is NULL");
    if (!counts_dev) return fail(PNY_ERR_ARG, who + "counts_dev is NULL");
    if (!lists_dev) return fail(PNY_ERR_ARG, who + "lists_dev is NULL");
    if (!totals_dev) return fail(PNY_ERR_ARG, who + "totals_dev is NULL");
    if (const int rc = detect_check_form(who, desc)) return rc;
    if (desc->max_kept != 0)
        return fail(PNY_ERR_ARG, who + "max_kept must be 0 (a sweep keeps no boxes: pny_detect_views at the chosen setting gives them), got " +
                                     std::to_string(desc->max_kept));
    if (const int rc = check_thresholds(who, "nms_ious", nms_ious_host, n_nms_ious, DETECT_SWEEP_MAX_NMS_IOUS)) return rc;
    if (const int rc = check_thresholds(who, "conf_cuts", conf_cuts_host, n_conf_cuts, DETECT_SWEEP_MAX_CUTS)) return rc;
    if (const int rc = check_thresholds(who, "match_ious", match_ious_host, n_match_ious, DETECT_SWEEP_MAX_MATCH_IOUS)) return rc;
    DetectSweepArgs s = {};
    s.n_nms = n_nms_ious, s.n_cuts = n_conf_cuts, s.n_match = n_match_ious;
    for (int k = 0; k < n_nms_ious; ++k) s.nms_ious[k] = (float)nms_ious_host[k];
    for (int k = 0; k < n_conf_cuts; ++k) s.cuts[k] = conf_cuts_host[k];
    for (int k = 0; k < n_conf_cuts; ++k) s.cut_order[k] = (unsigned char)k;
    std::stable_sort(s.cut_order, s.cut_order + n_conf_cuts, [&](unsigned char x, unsigned char y) { return s.cuts[x] < s.cuts[y]; });
    for (int k = 0; k < n_match_ious; ++k) s.match_ious[k] = (float)match_ious_host[k];
    s.counts = counts_dev, s.lists = lists_dev;
    s.in.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    const int rc = detect_fill_inputs(who, desc, preds_dev, targets_dev, anchors_host, pred_rows_dev, pred_offsets_dev, target_rows_dev,
                                      target_offsets_dev, &s.in);
    if (rc != PNY_OK) return rc;
    if ((int64_t)desc->n_views * n_nms_ious * n_conf_cuts >= (int64_t)1 << 31)
        return fail(PNY_ERR_ARG, who + "n_views * n_nms_ious * n_conf_cuts must stay below 2^31 workgroups");
    const size_t lds = detect_lds_bytes(s.in.cap);
    const hipError_t e = detect_sweep_lds_limit(lds);
    if (e != hipSuccess) {  // refuse here, not through the launch that would fail next
        (void)hipGetLastError();
        set_error(who + std::to_string(lds) + " bytes of dynamic LDS and the device refused that limit (" + hipGetErrorString(e) + ")");
        return PNY_ERR_HIP;
    }
    launch_detect_sweep(s, lds, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
