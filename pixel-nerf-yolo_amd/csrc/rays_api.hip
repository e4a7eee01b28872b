// Stateless C entry points that produce rays (include/pnyolo.h): ray generation from host poses and the two one-launch
// training batches.  Kernels in render_kernels.hip.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"

using namespace pny;

// 3x3 / 4x4 inverses on the host in double precision (reference uses torch.inverse on fp32).
static bool invert4(const float* m, double* inv) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            a[i][j] = m[4 * i + j];
            a[i][4 + j] = (i == j) ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (std::fabs(a[piv][c]) < 1e-30) return false;
        if (piv != c)
            for (int j = 0; j < 8; ++j) std::swap(a[piv][j], a[c][j]);
        const double d = a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] /= d;
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const double f = a[r][c];
                for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j];
            }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv[4 * i + j] = a[i][4 + j];
    return true;
}

extern "C" {

int pny_gen_rays_range(const float* poses_host, int b, int width, int height, const float focal[2], const float c[2],
                       float z_near, float z_far, int yolo_mode, int64_t first_ray, int64_t n_rays, float* out_dev,
                       pny_stream stream) {
    if (!poses_host || !focal || !c || (!out_dev && n_rays > 0)) return fail(PNY_ERR_ARG, "pny_gen_rays: null argument");
    if (b < 0 || width < 1 || height < 1) return fail(PNY_ERR_ARG, "pny_gen_rays: bad shape");
    const int64_t total = (int64_t)b * width * height;
    if (first_ray < 0 || n_rays < 0 || first_ray + n_rays > total) return fail(PNY_ERR_ARG, "pny_gen_rays: ray range outside the (b, h, w) grid");
    if (n_rays == 0) return PNY_OK;
    if (reinterpret_cast<uintptr_t>(out_dev) & 15) return fail(PNY_ERR_ARG, "pny_gen_rays: out_dev must be 16-byte aligned");
    std::vector<float> cam((size_t)b * 16);
    for (int i = 0; i < b; ++i) {
        const float* P = poses_host + 16 * i;
        float* o = cam.data() + 16 * i;
        if (!yolo_mode) {
            for (int r = 0; r < 3; ++r) {
                for (int q = 0; q < 3; ++q) o[3 * r + q] = P[4 * r + q];
                o[9 + r] = P[4 * r + 3];
            }
            o[12] = focal[0];
            o[13] = focal[1];
            o[14] = c[0];
            o[15] = c[1];
        } else {
            double inv[16];
            if (!invert4(P, inv)) return fail(PNY_ERR_ARG, "pny_gen_rays: singular extrinsic matrix");
            for (int r = 0; r < 3; ++r) {
                for (int q = 0; q < 3; ++q) o[3 * r + q] = (float)inv[4 * r + q];
                o[9 + r] = (float)inv[4 * r + 3];
            }
            if (focal[0] == 0.f || focal[1] == 0.f) return fail(PNY_ERR_ARG, "pny_gen_rays: zero focal length");
            o[12] = (float)(1.0 / focal[0]);
            o[13] = (float)(1.0 / focal[1]);
            o[14] = (float)(-(double)c[0] / focal[0]);
            o[15] = (float)(-(double)c[1] / focal[1]);
        }
    }
    // the per-image parameter blocks travel as kernel arguments: nothing is staged, allocated or synchronised here
    launch_gen_rays(cam.data(), b, width, height, z_near, z_far, yolo_mode, out_dev, (hipStream_t)stream, first_ray, n_rays);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_gen_rays(const float* poses_host, int b, int width, int height, const float focal[2], const float c[2],
                 float z_near, float z_far, int yolo_mode, float* out_dev, pny_stream stream) {
    if (b < 0 || width < 1 || height < 1) return fail(PNY_ERR_ARG, "pny_gen_rays: bad shape");
    return pny_gen_rays_range(poses_host, b, width, height, focal, c, z_near, z_far, yolo_mode, 0,
                              (int64_t)b * width * height, out_dev, stream);
}

int pny_sample_train_batch(const pny_train_batch_desc* d, const float* images_dev, const float* poses_dev,
                           const float* focal_dev, const float* c_dev, const float* bboxes_dev,
                           const pny_train_batch_draws* draws, float* rays_dev, float* rgb_gt_dev, int32_t* pix_dev,
                           pny_stream stream) {
    const char* who = "pny_sample_train_batch: ";
    if (!d || !images_dev || !poses_dev || !focal_dev || !rays_dev || !rgb_gt_dev)
        return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (d->n_objs < 1 || d->n_views < 1 || d->height < 1 || d->width < 1 || d->n_rays < 1)
        return fail(PNY_ERR_ARG, std::string(who) + "bad shape");
    if ((int64_t)d->n_objs * d->n_rays > INT32_MAX) return fail(PNY_ERR_ARG, std::string(who) + "more than 2^31 - 1 rays");
    // (also what keeps a seeded flat index inside one 32-bit Philox word's reach)
    if ((int64_t)d->n_views * d->height * d->width > (int64_t)UINT32_MAX)
        return fail(PNY_ERR_ARG, std::string(who) + "NV * H * W must be below 2^32");
    if ((d->focal_rows != 1 && d->focal_rows != d->n_objs) || (d->focal_cols != 1 && d->focal_cols != 2))
        return fail(PNY_ERR_ARG, std::string(who) + "focal must be (1 | SB, 1 | 2)");
    if (c_dev && d->c_rows != 1 && d->c_rows != d->n_objs) return fail(PNY_ERR_ARG, std::string(who) + "c must be (1 | SB, 2)");
    if (draws && (bboxes_dev ? (!draws->image_ids_dev || !draws->u_x_dev || !draws->u_y_dev) : !draws->pix_inds_dev))
        return fail(PNY_ERR_ARG, std::string(who) + (bboxes_dev ? "bbox mode replays image_ids_dev, u_x_dev and u_y_dev"
                                                                : "uniform mode replays pix_inds_dev"));
    if (reinterpret_cast<uintptr_t>(rays_dev) & 15) return fail(PNY_ERR_ARG, std::string(who) + "rays_dev must be 16-byte aligned");
    TrainBatchArgs a;
    a.sb = d->n_objs, a.nv = d->n_views, a.h = d->height, a.w = d->width, a.b = d->n_rays;
    a.znear = d->z_near, a.zfar = d->z_far;
    a.focal_rows = d->focal_rows, a.focal_cols = d->focal_cols, a.c_rows = c_dev ? d->c_rows : 1;
    a.seed = d->seed, a.draw_offset = draws ? 0 : d->draw_offset;
    a.images = images_dev, a.poses = poses_dev, a.focal = focal_dev, a.c = c_dev, a.bboxes = bboxes_dev;
    a.pix_inds = draws && !bboxes_dev ? draws->pix_inds_dev : nullptr;
    a.image_ids = draws && bboxes_dev ? draws->image_ids_dev : nullptr;
    a.u_x = draws && bboxes_dev ? draws->u_x_dev : nullptr;
    a.u_y = draws && bboxes_dev ? draws->u_y_dev : nullptr;
    a.rays = rays_dev, a.rgb = rgb_gt_dev, a.pix = pix_dev;
    launch_train_batch(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_yolo_train_batch(const pny_yolo_batch_desc* d, const float* poses_host, const int64_t* view_ids_host, const float focal[2],
                         const float c[2], const float* const* targets_dev, float* rays_dev, float* targets_out_dev,
                         int64_t* offsets_host, pny_stream stream) {
    const std::string who = "pny_yolo_train_batch: ";
    if (!d || !offsets_host) return fail(PNY_ERR_ARG, who + "null argument");
    const bool query = !rays_dev && !targets_out_dev;   // size query: offsets_host only
    if (!query && (!poses_host || !view_ids_host || !focal || !c || !targets_dev || !rays_dev || !targets_out_dev))
        return fail(PNY_ERR_ARG, who + "null argument");
    if (d->n_scales < 1 || d->n_scales > PNY_YOLO_BATCH_MAX_SCALES) return fail(PNY_ERR_ARG, who + "n_scales must be 1 .. 4");
    if (d->n_views < 1 || d->n_views > PNY_YOLO_BATCH_MAX_VIEWS)
        return fail(PNY_ERR_ARG, who + "n_views must be 1 .. 16 (one launch carries at most 16 selected cameras)");
    if (d->n_views_all < 1 || d->height < 1 || d->width < 1) return fail(PNY_ERR_ARG, who + "bad shape");
    if (d->n_anchors < 1 || d->n_anchors > 64) return fail(PNY_ERR_ARG, who + "bad shape: n_anchors must be 1 .. 64");
    if ((reinterpret_cast<uintptr_t>(rays_dev) & 15) || (reinterpret_cast<uintptr_t>(targets_out_dev) & 3))
        return fail(PNY_ERR_ARG, who + "rays_dev must be 16-byte aligned (targets_out_dev 4-byte)");
    YoloBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.n_scales = d->n_scales, a.row = d->n_anchors * 6;
    a.znear = d->z_near, a.zfar = d->z_far;
    a.rays = rays_dev, a.targets_out = targets_out_dev;
    if (!query && (focal[0] == 0.f || focal[1] == 0.f)) return fail(PNY_ERR_ARG, who + "zero focal length");
    for (int s = 0; s < d->n_scales; ++s) {
        const int cell = d->cell_sizes[s];
        if (cell < 1 || cell > d->height || cell > d->width)
            return fail(PNY_ERR_ARG, who + "every cell size must be 1 .. min(height, width)");
        a.hs[s] = d->height / cell, a.ws[s] = d->width / cell;
        a.off[s + 1] = a.off[s] + (long long)d->n_views * a.hs[s] * a.ws[s];
        if ((long long)d->n_views_all * a.hs[s] * a.ws[s] > INT32_MAX) return fail(PNY_ERR_ARG, who + "more than 2^31 - 1 cells in a grid");
        if (query) continue;
        if (!targets_dev[s] || (reinterpret_cast<uintptr_t>(targets_dev[s]) & 3)) return fail(PNY_ERR_ARG, who + "null or unaligned target grid");
        a.targets[s] = targets_dev[s];
        // the scale's intrinsics in fp32 (YoloTrainer.py:107-108), then Kinv's entries exactly as pny_gen_rays_range forms them
        const float fx = focal[0] / (float)cell, fy = focal[1] / (float)cell, cx = c[0] / (float)cell, cy = c[1] / (float)cell;
        a.kinv[s][0] = (float)(1.0 / fx);
        a.kinv[s][1] = (float)(1.0 / fy);
        a.kinv[s][2] = (float)(-(double)cx / fx);
        a.kinv[s][3] = (float)(-(double)cy / fy);
    }
    if (a.off[d->n_scales] * a.row > INT32_MAX) return fail(PNY_ERR_ARG, who + "more than 2^31 - 1 target values");
    if (query) {
        for (int s = 0; s <= d->n_scales; ++s) offsets_host[s] = a.off[s];
        return PNY_OK;
    }
    for (int i = 0; i < d->n_views; ++i) {
        const int64_t v = view_ids_host[i];
        if (v < 0 || v >= d->n_views_all) return fail(PNY_ERR_ARG, who + "view id outside [0, n_views_all)");
        double inv[16];
        if (!invert4(poses_host + 16 * v, inv)) return fail(PNY_ERR_ARG, who + "singular extrinsic matrix");
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) a.pose[i][3 * r + q] = (float)inv[4 * r + q];
            a.pose[i][9 + r] = (float)inv[4 * r + 3];
        }
        a.view_id[i] = (int)v;
    }
    for (int s = 0; s <= d->n_scales; ++s) offsets_host[s] = a.off[s];
    launch_yolo_train_batch(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
