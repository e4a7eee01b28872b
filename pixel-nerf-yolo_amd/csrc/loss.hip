// The two training losses, one launch each, with the gradient w.r.t. the predictions written by the same launch:
//   rgb_loss_kernel   the NeRF trainer's rgb terms (reference train/trainlib/PixelNerfTrainer.py:147-154: MSELoss / L1Loss of the
//                     coarse and the fine pass against the ground truth, scaled by lambda_coarse / lambda_fine and added)
//   yolo_loss_kernel  YoloLoss.forward (reference src/model/loss.py:121-163 with util.iou, src/util/util.py:582-608)
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

__global__ __launch_bounds__(LOSS_THREADS) void yolo_loss_kernel(YoloLossArgs a) {
    __shared__ double lds[4 * 4];
    const int A = a.A, C = a.C, row = 5 + C;
    // 1. the two counts the means divide by.  The gradient needs them, so every workgroup counts ALL items for itself
    //    (integers: exact, any order) instead of waiting for the others.
    double cnt[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < a.items; i += LOSS_THREADS) {
        const float t0 = a.target[i * 6];
        cnt[0] += t0 == 1.f ? 1.0 : 0.0;
        cnt[1] += t0 == 0.f ? 1.0 : 0.0;
    }
    block_sum<2>(cnt, lds);
    const double n_obj = cnt[0], n_noobj = cnt[1];
    const float inv_obj = n_obj > 0.0 ? (float)(1.0 / n_obj) : 0.f, inv_noobj = n_noobj > 0.0 ? (float)(1.0 / n_noobj) : 0.f;
    const float g_obj = a.w_obj * 2.f * inv_obj, g_box = a.w_box * 2.f * (float)(n_obj > 0.0 ? 0.25 / n_obj : 0.0),
                g_cls = a.w_cls * inv_obj, g_noobj = a.w_noobj * inv_noobj;
    // 2. terms and gradient of this workgroup's items: s = {box, object, no_object, class} sums
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const long long stride = (long long)gridDim.x * LOSS_THREADS;
    for (long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x; i < a.items; i += stride) {
        const float* p = a.pred + i * row;
        const float* t = a.target + i * 6;
        float* d = a.d_pred ? a.d_pred + i * row : nullptr;
        const float t0 = t[0];
        if (t0 == 0.f) {
            // BCELoss against target 0 (loss.py:128-130): -max(log(1 - p), -100); backward (p - 0) / max(p (1 - p), 1e-12)
            const float pp = p[0];
            s[2] += (double)(-fmaxf(log1pf(-pp), -100.f));
            if (d) {
                d[0] = g_noobj * (pp / fmaxf((1.f - pp) * pp, 1e-12f));
                for (int k = 1; k < row; ++k) d[k] = 0.f;
            }
        } else if (t0 == 1.f) {
            const int an = (int)(i % A);
            const float aw = a.anchors[2 * an], ah = a.anchors[2 * an + 1];
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
            for (int k = 1; k < C; ++k) mx = fmaxf(mx, p[5 + k]);
            float se = 0.f;
            for (int k = 0; k < C; ++k) se += expf(p[5 + k] - mx);
            const float lse = mx + logf(se);
            const float nanv = __int_as_float(0x7fc00000);
            s[3] += valid ? (double)(lse - p[5 + cls]) : (double)nanv;
            if (d) {
                d[0] = g_obj * eo;
                d[1] = g_box * e1 * (sx * (1.f - sx));
                d[2] = g_box * e2 * (sy * (1.f - sy));
                d[3] = g_box * e3;
                d[4] = g_box * e4;
                for (int k = 0; k < C; ++k)
                    d[5 + k] = valid ? g_cls * (expf(p[5 + k] - lse) - (k == cls ? 1.f : 0.f)) : nanv;
            }
        } else if (d) {   // ignored anchor (the dataset writes -1): no term, zero gradient
            for (int k = 0; k < row; ++k) d[k] = 0.f;
        }
    }
    block_sum<4>(s, lds);
    if (!combine<4>(s, a.partials, a.ticket)) return;
    // means (no_object over nothing: 0 / 0 = NaN, as ATen's mean; no object cell: the three object terms are exactly 0)
    const bool any = n_obj > 0.0;
    const double box = any ? s[0] / (4.0 * n_obj) : 0.0, obj = any ? s[1] / n_obj : 0.0, cls = any ? s[3] / n_obj : 0.0;
    const double noobj = s[2] / n_noobj;
    a.terms[0] = (float)((double)a.w_box * box + (double)a.w_obj * obj + (double)a.w_noobj * noobj + (double)a.w_cls * cls);
    a.terms[1] = (float)box;
    a.terms[2] = (float)obj;
    a.terms[3] = (float)noobj;
    a.terms[4] = (float)cls;
    if (a.counts) {
        a.counts[0] = (int)n_obj;
        a.counts[1] = (int)n_noobj;
    }
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

}  // namespace pny
