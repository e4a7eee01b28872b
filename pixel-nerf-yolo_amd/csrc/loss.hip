// The two training losses, one launch each, with the gradient w.r.t. the predictions written by the same launch:
//   rgb_loss_kernel   the NeRF trainer's rgb terms (reference train/trainlib/PixelNerfTrainer.py:147-154: MSELoss / L1Loss of the
//                     coarse and the fine pass against the ground truth, scaled by lambda_coarse / lambda_fine and added)
//   yolo_loss_kernel  YoloLoss.forward (reference src/model/loss.py:121-163 with util.iou, src/util/util.py:582-608)
//   yolo_loss_batches_kernel  the same loss for every mini-batch of a YOLO training step at once, each normalised by its own
//                     counts, and the trainer's sums over the mini-batches (reference train/trainlib/YoloTrainer.py:149-208)
// Elementwise work plus a reduction; no MFMA, nothing tuned to a large shape.  What they are for: one launch instead of ten
// (NeRF) or some forty (YOLO) ATen launches and no device -> host wait (the reference's boolean-mask gathers and .item() calls).
//
// Reduction: every thread adds its elements in index order into fp64 sums, a workgroup adds its threads' sums in a fixed
// tree, and a launch of more than one workgroup adds the workgroups' sums in workgroup order: each workgroup stores its sums
// into its row of a table and draws a ticket; the one that draws the last ticket adds the rows 0, 1, 2, ... and puts the ticket
// counter back to zero for the next launch.  No float atomics: the same inputs give the same bits on every run.
// The element -> (workgroup, thread) assignment depends on the element count only.
#include "pny_loss.h"

namespace pny {
namespace {

// Sums of the workgroup's threads in a fixed order, returned to every thread.  lds: 4 * NV doubles, free again on return.
template <int NV>
__device__ inline void block_sum(double (&v)[NV], double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double x = v[i];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) lds[wave * NV + i] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = ((lds[i] + lds[NV + i]) + lds[2 * NV + i]) + lds[3 * NV + i];
    __syncthreads();
}

// v: this workgroup's sums.  Returns true in ONE thread of the launch, thread 0 of the workgroup that finishes last (of the
// only workgroup in a launch of one), with v = the sums over all workgroups added in workgroup order.
// Hand-off: plain stores of the row, agent-scope release, relaxed agent-scope ticket add; the last arriver acquires at agent
// scope and reads the rows with agent-scope loads (the rows' writers may sit on another XCD with an L2 of its own).
template <int NV>
__device__ inline bool combine(double (&v)[NV], double* partials, unsigned* ticket) {
    if (threadIdx.x != 0) return false;
    if (gridDim.x == 1) return true;
#pragma unroll
    for (int i = 0; i < NV; ++i) partials[(size_t)blockIdx.x * NV + i] = v[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != gridDim.x - 1) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.0;
    for (unsigned g = 0; g < gridDim.x; ++g)
#pragma unroll
        for (int i = 0; i < NV; ++i)
            v[i] += __hip_atomic_load(partials + (size_t)g * NV + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch starts from zero
    return true;
}

// One pass's element: e = (x - g)^2 or |x - g| in fp32 as ATen's elementwise kernels compute it; gradient scale gs =
// lambda * 2 / n (MSE) or lambda / n (L1, times sign(x - g) with sign(0) = 0).
__device__ inline float rgb_elem(float x, float g, int l1, float gs, float* d, long long i) {
    const float diff = x - g;
    if (d) d[i] = l1 ? (diff > 0.f ? gs : diff < 0.f ? -gs : 0.f) : gs * diff;
    return l1 ? fabsf(diff) : diff * diff;
}

__global__ __launch_bounds__(LOSS_THREADS) void rgb_loss_kernel(RgbLossArgs a) {
    __shared__ double lds[4 * 2];
    double s[2] = {0.0, 0.0};
    const double inv_n = 1.0 / (double)a.n;
    const float gs_c = (float)((a.l1_coarse ? 1.0 : 2.0) * (double)a.lambda_coarse * inv_n);
    const float gs_f = (float)((a.l1_fine ? 1.0 : 2.0) * (double)a.lambda_fine * inv_n);
    const long long stride = (long long)gridDim.x * LOSS_THREADS;
    for (long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < a.n; i += stride) {
        const float g = a.gt[i];
        s[0] += (double)rgb_elem(a.coarse[i], g, a.l1_coarse, gs_c, a.d_coarse, i);
        if (a.fine) s[1] += (double)rgb_elem(a.fine[i], g, a.l1_fine, gs_f, a.d_fine, i);
    }
    block_sum<2>(s, lds);
    if (!combine<2>(s, a.partials, a.ticket)) return;
    const double rc = (double)a.lambda_coarse * (s[0] * inv_n);
    const double rf = a.fine ? (double)a.lambda_fine * (s[1] * inv_n) : 0.0;
    a.terms[0] = (float)rc;
    a.terms[1] = (float)rf;
    a.terms[2] = (float)(rc + rf);
}

__device__ inline float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---- YoloLoss: one statement of the arithmetic for yolo_loss_kernel (one loss over all items) and yolo_loss_batches_kernel
// (one loss per mini-batch): the counts and what the gradient is scaled by, one item, the means.
struct YoloScales {
    double n_obj, n_noobj;
    float g_obj, g_box, g_cls, g_noobj;   // gradient scales: weight * d mean / d element
};

// The two counts the means divide by, over `items` items from `target` on, by the whole workgroup (integers: exact, any
// order).  lds: 8 doubles.
__device__ inline YoloScales yolo_scales(const float* target, long long items, float w_box, float w_obj, float w_noobj, float w_cls,
                                         double* lds) {
    double cnt[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < items; i += LOSS_THREADS) {
        const float t0 = target[i * 6];
        cnt[0] += t0 == 1.f ? 1.0 : 0.0;
        cnt[1] += t0 == 0.f ? 1.0 : 0.0;
    }
    block_sum<2>(cnt, lds);
    YoloScales k;
    k.n_obj = cnt[0], k.n_noobj = cnt[1];
    const float inv_obj = k.n_obj > 0.0 ? (float)(1.0 / k.n_obj) : 0.f, inv_noobj = k.n_noobj > 0.0 ? (float)(1.0 / k.n_noobj) : 0.f;
    k.g_obj = w_obj * 2.f * inv_obj, k.g_box = w_box * 2.f * (float)(k.n_obj > 0.0 ? 0.25 / k.n_obj : 0.0);
    k.g_cls = w_cls * inv_obj, k.g_noobj = w_noobj * inv_noobj;
    return k;
}

// One (cell, anchor) pair: p its 5 + C predictions, t its 6 target values, anchors the (A, 2) of its scale, i its index
// (anchor i % A), d its gradient row or null.  Adds to s = {box, object, no_object, class}.
__device__ inline void yolo_item(const float* p, const float* t, const float* anchors, long long i, int A, float* d, int C,
                                 const YoloScales& k, double (&s)[4]) {
    const int row = 5 + C;
    const float g_obj = k.g_obj, g_box = k.g_box, g_cls = k.g_cls, g_noobj = k.g_noobj;
    const float t0 = t[0];
    if (t0 == 0.f) {
        // BCELoss against target 0 (loss.py:128-130): -max(log(1 - p), -100); backward (p - 0) / max(p (1 - p), 1e-12)
        const float pp = p[0];
        s[2] += (double)(-fmaxf(log1pf(-pp), -100.f));
        if (d) {
            d[0] = g_noobj * (pp / fmaxf((1.f - pp) * pp, 1e-12f));
            for (int j = 1; j < row; ++j) d[j] = 0.f;
        }
    } else if (t0 == 1.f) {
        const int an = (int)(i % A);
        const float aw = anchors[2 * an], ah = anchors[2 * an + 1];
        const float sx = sigmoidf_(p[1]), sy = sigmoidf_(p[2]);
        // IoU of [sigmoid(x), sigmoid(y), exp(w) aw, exp(h) ah] and target[1:5] (loss.py:135-139, util.py:582-608); a constant
        // for the gradient (.detach())
        const float bw = expf(p[3]) * aw, bh = expf(p[4]) * ah;
        const float b1x1 = sx - bw / 2.f, b1y1 = sy - bh / 2.f, b1x2 = sx + bw / 2.f, b1y2 = sy + bh / 2.f;
        const float b2x1 = t[1] - t[3] / 2.f, b2y1 = t[2] - t[4] / 2.f, b2x2 = t[1] + t[3] / 2.f, b2y2 = t[2] + t[4] / 2.f;
        const float ix = fmaxf(fminf(b1x2, b2x2) - fmaxf(b1x1, b2x1), 0.f), iy = fmaxf(fminf(b1y2, b2y2) - fmaxf(b1y1, b2y1), 0.f);
        const float inter = ix * iy;
        const float area1 = fabsf((b1x2 - b1x1) * (b1y2 - b1y1)), area2 = fabsf((b2x2 - b2x1) * (b2y2 - b2y1));
        const float iou = inter / (area1 + area2 - inter + 1e-6f);
        const float eo = p[0] - iou * t0;                                   // object term (loss.py:141-142)
        s[1] += (double)(eo * eo);
        // box term (loss.py:145-150): sigmoid(x, y) against the target centre, raw w, h against log(1e-6 + size / anchor)
        const float e1 = sx - t[1], e2 = sy - t[2];
        const float e3 = p[3] - logf(1e-6f + t[3] / aw), e4 = p[4] - logf(1e-6f + t[4] / ah);
        s[0] += (double)(e1 * e1) + (double)(e2 * e2) + (double)(e3 * e3) + (double)(e4 * e4);
        // class term (loss.py:153-154): cross entropy of the C logits; a class outside [0, C) reads nothing and gives NaN
        const float tc = truncf(t[5]);
        const bool valid = tc >= 0.f && tc < (float)C;
        const int cls = valid ? (int)tc : 0;
        float mx = p[5];
        for (int j = 1; j < C; ++j) mx = fmaxf(mx, p[5 + j]);
        float se = 0.f;
        for (int j = 0; j < C; ++j) se += expf(p[5 + j] - mx);
        const float lse = mx + logf(se);
        const float nanv = __int_as_float(0x7fc00000);
        s[3] += valid ? (double)(lse - p[5 + cls]) : (double)nanv;
        if (d) {
            d[0] = g_obj * eo;
            d[1] = g_box * e1 * (sx * (1.f - sx));
            d[2] = g_box * e2 * (sy * (1.f - sy));
            d[3] = g_box * e3;
            d[4] = g_box * e4;
            for (int j = 0; j < C; ++j)
                d[5 + j] = valid ? g_cls * (expf(p[5 + j] - lse) - (j == cls ? 1.f : 0.f)) : nanv;
        }
    } else if (d) {   // ignored anchor (the dataset writes -1): no term, zero gradient
        for (int j = 0; j < row; ++j) d[j] = 0.f;
    }
}

// Means of the sums s (no_object over nothing: 0 / 0 = NaN, as ATen's mean; no object cell: the three object terms are exactly
// 0) -> terms[5] = {total, box, object, no_object, class}, counts[2] (or null) = {n_obj, n_noobj}.  One thread.
__device__ inline void yolo_means(const double (&s)[4], const YoloScales& k, float w_box, float w_obj, float w_noobj, float w_cls,
                                  float* terms, int* counts) {
    const double n_obj = k.n_obj, n_noobj = k.n_noobj;
    const bool any = n_obj > 0.0;
    const double box = any ? s[0] / (4.0 * n_obj) : 0.0, obj = any ? s[1] / n_obj : 0.0, cls = any ? s[3] / n_obj : 0.0;
    const double noobj = s[2] / n_noobj;
    terms[0] = (float)((double)w_box * box + (double)w_obj * obj + (double)w_noobj * noobj + (double)w_cls * cls);
    terms[1] = (float)box;
    terms[2] = (float)obj;
    terms[3] = (float)noobj;
    terms[4] = (float)cls;
    if (counts) {
        counts[0] = (int)n_obj;
        counts[1] = (int)n_noobj;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void yolo_loss_kernel(YoloLossArgs a) {
    __shared__ double lds[4 * 4];
    const int A = a.A, C = a.C, row = 5 + C;
    // 1. the two counts the means divide by.  The gradient needs them, so every workgroup counts ALL items for itself
    //    instead of waiting for the others.
    const YoloScales k = yolo_scales(a.target, a.items, a.w_box, a.w_obj, a.w_noobj, a.w_cls, lds);
    // 2. terms and gradient of this workgroup's items: s = {box, object, no_object, class} sums
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const long long stride = (long long)gridDim.x * LOSS_THREADS;
    for (long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < a.items; i += stride)
        yolo_item(a.pred + i * row, a.target + i * 6, a.anchors, i, A, a.d_pred ? a.d_pred + i * row : nullptr, C, k, s);
    block_sum<4>(s, lds);
    if (!combine<4>(s, a.partials, a.ticket)) return;
    yolo_means(s, k, a.w_box, a.w_obj, a.w_noobj, a.w_cls, a.terms, a.counts);
}

// One workgroup per mini-batch ("segment") of a training step.  Thread t takes the segment's items t, t + 256, ... in that
// order and the sums go through block_sum: a one-workgroup launch of yolo_loss_kernel on the segment's slice.
// Step values: thread 0 stores its segment's terms and hands them off as combine<> does (plain stores, agent-scope release,
// relaxed agent-scope ticket add); the workgroup that draws the last ticket acquires, reads all rows of terms_seg with
// agent-scope loads (256 rows at a time into LDS), thread 0 adds them in segment order in fp64, and the ticket goes back to 0.
__global__ __launch_bounds__(LOSS_THREADS) void yolo_loss_batches_kernel(YoloBatchesArgs a) {
    __shared__ double lds[4 * 4];
    __shared__ float rows_lds[LOSS_THREADS * 5];
    __shared__ int last_lds;
    const int A = a.A, C = a.C, row = 5 + C;
    // this workgroup's segment: its scale, first row and row count
    long long m = blockIdx.x, row0 = 0, n_rows = 0;
    int scale = 0;
    for (int sc = 0; sc < a.n_scales; ++sc) {
        const long long segs = a.rows[sc] / a.batch_rows + (a.rows[sc] % a.batch_rows != 0);
        if (m < segs) {
            scale = sc;
            row0 += m * a.batch_rows;
            n_rows = a.rows[sc] - m * a.batch_rows < a.batch_rows ? a.rows[sc] - m * a.batch_rows : a.batch_rows;
            break;
        }
        m -= segs;
        row0 += a.rows[sc];
    }
    const long long items = n_rows * A, item0 = row0 * A;     // (n_rows == 0: blockIdx.x >= M, which the launcher never gives)
    const float* pred = a.pred + item0 * row;
    const float* target = a.target + item0 * 6;
    const float* anchors = a.anchors + (size_t)scale * A * 2;
    float* d_pred = a.d_pred ? a.d_pred + item0 * row : nullptr;
    const YoloScales k = yolo_scales(target, items, a.w_box, a.w_obj, a.w_noobj, a.w_cls, lds);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < items; i += LOSS_THREADS)
        yolo_item(pred + i * row, target + i * 6, anchors, i, A, d_pred ? d_pred + i * row : nullptr, C, k, s);
    block_sum<4>(s, lds);
    if (threadIdx.x == 0) {
        yolo_means(s, k, a.w_box, a.w_obj, a.w_noobj, a.w_cls, a.terms_seg + (size_t)blockIdx.x * 5,
                   a.counts_seg ? a.counts_seg + (size_t)blockIdx.x * 2 : nullptr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_lds = t == (unsigned)a.segments - 1u;
    }
    __syncthreads();
    if (!last_lds) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int base = 0; base < a.segments; base += LOSS_THREADS) {
        const int n = a.segments - base < LOSS_THREADS ? a.segments - base : LOSS_THREADS;
        if ((int)threadIdx.x < n)
#pragma unroll
            for (int j = 0; j < 5; ++j)
                rows_lds[threadIdx.x * 5 + j] =
                    __hip_atomic_load(a.terms_seg + (size_t)(base + threadIdx.x) * 5 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (threadIdx.x == 0)
            for (int r = 0; r < n; ++r)
#pragma unroll
                for (int j = 0; j < 5; ++j) sum[j] += (double)rows_lds[r * 5 + j];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double M = (double)a.segments;
    a.step[0] = (float)sum[0];
#pragma unroll
    for (int j = 0; j < 5; ++j) a.step[1 + j] = (float)(sum[j] / M);
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch starts from zero
}

}  // namespace

int loss_grid(long long items, int per_group) {
    const long long g = (items + per_group - 1) / per_group;
    return (int)(g < 1 ? 1 : g > LOSS_MAX_GRID ? LOSS_MAX_GRID : g);
}

void launch_rgb_loss(const RgbLossArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(rgb_loss_kernel, dim3(loss_grid(a.n, LOSS_RGB_PER_GROUP)), dim3(LOSS_THREADS), 0, st, a);
}

void launch_yolo_loss(const YoloLossArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(yolo_loss_kernel, dim3(loss_grid(a.items, LOSS_YOLO_PER_GROUP)), dim3(LOSS_THREADS), 0, st, a);
}

void launch_yolo_loss_batches(const YoloBatchesArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(yolo_loss_batches_kernel, dim3(a.segments), dim3(LOSS_THREADS), 0, st, a);
}

}  // namespace pny
