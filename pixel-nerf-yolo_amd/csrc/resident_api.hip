// C entry points of the resident views (include/pnyolo.h, "resident views" section; kernels in resident.hip): argument checks
// that name the argument, then one launch each.  No workspace, no allocation, no copy, no synchronisation.
//
// pny_resident_train_batch stands where the reference's train/trainlib/PixelNerfTrainer.py:76-133 reads its ray batch and
// ground truth out of the (SB, NV, 3, H, W) tensor that SRNDataset.__getitem__ (src/data/SRNDataset.py:61-136) and
// DVRDataset.__getitem__ (src/data/DVRDataset.py:110-275) decoded and normalised in full; pny_ingest_views_indexed stands where
// :125-133 selects the NS source views of each object from that tensor.
#include <string>

#include "api_internal.h"
#include "pny_resident.h"

namespace pny {
void launch_resident_batch(const ResidentBatchArgs& a, hipStream_t st);
void launch_resident_ingest(const ResidentIngestArgs& a, int n_out, hipStream_t st);
}  // namespace pny

using namespace pny;

static_assert(INGEST_RESIZE_NONE == PNY_RESIZE_NONE && INGEST_RESIZE_BILINEAR_U8 == PNY_RESIZE_BILINEAR_U8 &&
                  INGEST_RESIZE_AREA == PNY_RESIZE_AREA, "pny_ingest.h and pnyolo.h disagree on the resize modes");

namespace {

// the store's geometry, checked: 0, or PNY_ERR_ARG with the argument named
int store_geom(const std::string& who, int h, int w, int ch, int oh, int ow, int resize, ResidentGeom* g) {
    if (h <= 0 || w <= 0) return fail(PNY_ERR_ARG, who + "height and width must be positive");
    if (oh <= 0 || ow <= 0) return fail(PNY_ERR_ARG, who + "out_height and out_width must be positive");
    if (ch != 3 && ch != 4) return fail(PNY_ERR_ARG, who + "channels must be 3 or 4");
    if (resize != PNY_RESIZE_NONE && resize != PNY_RESIZE_BILINEAR_U8 && resize != PNY_RESIZE_AREA)
        return fail(PNY_ERR_ARG, who + "unknown resize");
    if (resize == PNY_RESIZE_NONE && (oh != h || ow != w))
        return fail(PNY_ERR_ARG, who + "PNY_RESIZE_NONE needs out_height == height and out_width == width");
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)h * w * ch >= lim) return fail(PNY_ERR_ARG, who + "height * width * channels: 2^31 bytes or more in a view");
    if ((int64_t)oh * ow * 3 >= lim) return fail(PNY_ERR_ARG, who + "out_height * out_width: 2^31 elements or more in a view");
    g->h = h, g->w = w, g->c = ch, g->oh = oh, g->ow = ow, g->resize = resize;
    g->scale_y = (float)h / (float)oh, g->scale_x = (float)w / (float)ow;
    return PNY_OK;
}

}  // namespace

extern "C" {

int pny_resident_train_batch(const pny_train_batch_desc* d, int32_t channels, int32_t out_height, int32_t out_width, int32_t resize,
                             const void* objs_dev, int32_t n_store_objs, const int32_t* obj_ids_dev, const float* poses_dev,
                             int64_t n_rows, const float* focal_dev, const float* c_dev, const float* bboxes_dev,
                             const pny_train_batch_draws* draws, float* rays_dev, float* rgb_gt_dev, int32_t* pix_dev,
                             pny_stream stream) {
    const std::string who = "pny_resident_train_batch: ";
    if (!d) return fail(PNY_ERR_ARG, who + "desc is null");
    if (!objs_dev) return fail(PNY_ERR_ARG, who + "objs_dev is null");
    if (!obj_ids_dev) return fail(PNY_ERR_ARG, who + "obj_ids_dev is null");
    if (!poses_dev) return fail(PNY_ERR_ARG, who + "poses_dev is null");
    if (!focal_dev) return fail(PNY_ERR_ARG, who + "focal_dev is null");
    if (!rays_dev) return fail(PNY_ERR_ARG, who + "rays_dev is null");
    if (!rgb_gt_dev) return fail(PNY_ERR_ARG, who + "rgb_gt_dev is null");
    if (d->n_objs < 1) return fail(PNY_ERR_ARG, who + "desc.n_objs must be positive");
    if (d->n_views < 1) return fail(PNY_ERR_ARG, who + "desc.n_views (the store's largest view count) must be positive");
    if (d->n_rays < 1) return fail(PNY_ERR_ARG, who + "desc.n_rays must be positive");
    if (n_store_objs < 1) return fail(PNY_ERR_ARG, who + "n_store_objs must be positive");
    if (n_rows < 1) return fail(PNY_ERR_ARG, who + "n_rows must be positive");
    ResidentBatchArgs a;
    if (int rc = store_geom(who, d->height, d->width, channels, out_height, out_width, resize, &a.g)) return rc;
    if ((int64_t)d->n_objs * d->n_rays > INT32_MAX) return fail(PNY_ERR_ARG, who + "desc.n_objs * desc.n_rays: more than 2^31 - 1 rays");
    // (what keeps a seeded flat index inside one 32-bit Philox word's reach, as in pny_sample_train_batch)
    if ((int64_t)d->n_views * out_height * out_width > (int64_t)UINT32_MAX)
        return fail(PNY_ERR_ARG, who + "desc.n_views * out_height * out_width must be below 2^32");
    if (draws && (bboxes_dev ? (!draws->image_ids_dev || !draws->u_x_dev || !draws->u_y_dev) : !draws->pix_inds_dev))
        return fail(PNY_ERR_ARG, who + (bboxes_dev ? "bbox mode replays draws.image_ids_dev, u_x_dev and u_y_dev"
                                                   : "uniform mode replays draws.pix_inds_dev"));
    if (reinterpret_cast<uintptr_t>(rays_dev) & 15) return fail(PNY_ERR_ARG, who + "rays_dev must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(objs_dev) & 7) return fail(PNY_ERR_ARG, who + "objs_dev must be 8-byte aligned");
    a.objs = static_cast<const ResidentObj*>(objs_dev), a.n_store_objs = n_store_objs;
    a.n_rows = n_rows;
    a.max_views = (int64_t)d->n_views < n_rows ? d->n_views : (int)n_rows;   // a record's views all have a row
    a.obj_ids = obj_ids_dev, a.sb = d->n_objs, a.b = d->n_rays;
    a.znear = d->z_near, a.zfar = d->z_far;
    a.seed = d->seed, a.draw_offset = draws ? 0 : d->draw_offset;
    a.poses = poses_dev, a.focal = focal_dev, a.c = c_dev, a.bboxes = bboxes_dev;
    a.pix_inds = draws && !bboxes_dev ? draws->pix_inds_dev : nullptr;
    a.image_ids = draws && bboxes_dev ? draws->image_ids_dev : nullptr;
    a.u_x = draws && bboxes_dev ? draws->u_x_dev : nullptr;
    a.u_y = draws && bboxes_dev ? draws->u_y_dev : nullptr;
    a.rays = rays_dev, a.rgb = rgb_gt_dev, a.pix = pix_dev;
    launch_resident_batch(a, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_ingest_views_indexed(const pny_ingest_desc* d, const void* objs_dev, int32_t n_store_objs, int32_t max_views,
                             const int32_t* obj_of_dev, const int32_t* view_of_dev, float* out_dev, pny_stream stream) {
    const std::string who = "pny_ingest_views_indexed: ";
    if (!d) return fail(PNY_ERR_ARG, who + "desc is null");
    if (!objs_dev) return fail(PNY_ERR_ARG, who + "objs_dev is null");
    if (!obj_of_dev) return fail(PNY_ERR_ARG, who + "obj_of_dev is null");
    if (!view_of_dev) return fail(PNY_ERR_ARG, who + "view_of_dev is null");
    if (!out_dev) return fail(PNY_ERR_ARG, who + "out_dev is null");
    if (d->n_views < 1) return fail(PNY_ERR_ARG, who + "desc.n_views must be positive");
    if (n_store_objs < 1) return fail(PNY_ERR_ARG, who + "n_store_objs must be positive");
    if (max_views < 1) return fail(PNY_ERR_ARG, who + "max_views must be positive");
    if (d->white_mask != 0) return fail(PNY_ERR_ARG, who + "desc.white_mask must be 0 (the store's boxes are made when it is filled)");
    ResidentIngestArgs a;
    if (int rc = store_geom(who, d->height, d->width, d->channels, d->out_height, d->out_width, d->resize, &a.g)) return rc;
    if ((int64_t)max_views * d->out_height * d->out_width > (int64_t)UINT32_MAX)
        return fail(PNY_ERR_ARG, who + "max_views * out_height * out_width must be below 2^32");
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)d->out_height * d->out_width * 3 * d->n_views >= lim)
        return fail(PNY_ERR_ARG, who + "desc.n_views * out_height * out_width: 2^31 output elements or more");
    if (reinterpret_cast<uintptr_t>(objs_dev) & 7) return fail(PNY_ERR_ARG, who + "objs_dev must be 8-byte aligned");
    a.objs = static_cast<const ResidentObj*>(objs_dev), a.n_store_objs = n_store_objs, a.max_views = max_views;
    a.obj_of = obj_of_dev, a.view_of = view_of_dev, a.out = out_dev;
    a.tiles_x = (a.g.ow + INGEST_TILE_X - 1) / INGEST_TILE_X, a.tiles_y = (a.g.oh + INGEST_TILE_Y - 1) / INGEST_TILE_Y;
    if ((int64_t)a.tiles_x * a.tiles_y * d->n_views >= lim)
        return fail(PNY_ERR_ARG, who + "desc.n_views * out_height * out_width: 2^31 output elements or more");
    launch_resident_ingest(a, d->n_views, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
