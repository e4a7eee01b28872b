// A dataset's decoded views resident on the device (resident.hip; entry points in resident_api.hip): which object, view and
// pixel a ray of a training batch reads from the store, and that pixel's colour.  Nothing here is new arithmetic: the pixel
// choice is pny_train_batch.h's (the object's own view count standing where NV stands there), the colour is the fp32 value
// pny_ingest_views writes at that output pixel (pny_ingest.h ingest_pixel), times 0.5 plus 0.5 as train_batch_kernel has it.
// Like those two headers it also compiles for the host (__host__ / __device__ defined away), which is how
// tests/test_cpu_resident.py runs it without a GPU.
#pragma once
#include <stdint.h>

#include "pny_ingest.h"
#include "pny_train_batch.h"

namespace pny {

constexpr int RESIDENT_BATCH_THREADS = 256;   // resident_batch_kernel: one thread per ray

// One object of the store, 16 bytes, as include/pnyolo.h describes the table (the ABI takes it as const void*)
struct ResidentObj {
    const uint8_t* views;   // (n_views, H, W, C) bytes
    int32_t n_views;
    int32_t first_row;      // the object's first row of the store's concatenated poses / boxes
};
static_assert(sizeof(ResidentObj) == 16, "the resident store's record is 16 bytes");

// the store's one decoded and one output geometry (the fields ingest_pixel reads)
struct ResidentGeom {
    int h, w, c, oh, ow, resize;
    float scale_y, scale_x;   // bilinear: (float)in / (float)out
};

// Indices from device memory are clamped into range, never trusted (the call cannot look at them without waiting): an
// object id into [0, n_store_objs), a view id into [0, n_views), a record's view count into [1, max_views] and its first row
// into [0, n_rows - n_views] (max_views <= n_rows: resident_api.hip).
__host__ __device__ inline int resident_clamp(int64_t v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : (int)v); }
__host__ __device__ inline int resident_view_count(int32_t n_views, int max_views) {
    return n_views < 1 ? 1 : (n_views > max_views ? max_views : n_views);
}
__host__ __device__ inline int64_t resident_first_row(int32_t first_row, int nv, int64_t n_rows) {
    return first_row < 0 ? 0 : (first_row > n_rows - nv ? n_rows - nv : (int64_t)first_row);
}

// The pixel of the ray with draw index di (= draw_offset + s * B + r) or with the replayed draws given, on an object of nv
// views of oh x ow: what train_batch_kernel picks for a one-object call on that object.  boxes: the object's (nv, 4), or
// null for uniform mode.
__device__ __forceinline__ BatchPixel resident_pick(int nv, int oh, int ow, const float* boxes, uint64_t seed, uint64_t di,
                                                     const int64_t* pix_ind, const int64_t* image_id, const float* u_x,
                                                     const float* u_y) {
    if (!boxes) {
        const int64_t flat = pix_ind ? *pix_ind : seeded_flat(seed, di, (uint32_t)((int64_t)nv * oh * ow));
        return pixel_from_flat(flat, nv, oh, ow);
    }
    const int view = image_id ? clamp_view(*image_id, nv) : seeded_view(seed, di, nv);
    const float ux = u_x ? *u_x : seeded_u_x(seed, di);
    const float uy = u_y ? *u_y : seeded_u_y(seed, di);
    return pixel_from_bbox(view, ux, uy, boxes + (size_t)view * 4, oh, ow);
}

// rgb_gt of output pixel (y, x) of the view at img: v * 0.5 + 0.5 with v the fp32 the ingest writes there
template <class Load>
__host__ __device__ inline void resident_rgb(const uint8_t* img, const ResidentGeom& g, int y, int x, Load load, float* rgb) {
    float r, gg, b, m;
    ingest_pixel(img, g, y, x, load, r, gg, b, m);
    rgb[0] = r * 0.5f + 0.5f, rgb[1] = gg * 0.5f + 0.5f, rgb[2] = b * 0.5f + 0.5f;
}

// resident_batch_kernel's argument block; every pointer is a device pointer
struct ResidentBatchArgs {
    ResidentGeom g;
    const ResidentObj* objs;    // (n_store_objs)
    int n_store_objs, max_views;
    int64_t n_rows;             // N_total: rows of poses / bboxes
    const int32_t* obj_ids;     // (SB)
    int sb, b;
    float znear, zfar;
    uint64_t seed, draw_offset;
    const float *poses, *focal, *c, *bboxes;   // (N_total, 4, 4), (n_store_objs, 2), (n_store_objs, 2) | null, (N_total, 4) | null
    const int64_t *pix_inds, *image_ids;       // replayed draws (SB, B); null: Philox draws from seed
    const float *u_x, *u_y;
    float *rays, *rgb;          // (SB, B, 8), (SB, B, 3)
    int32_t* pix;               // (SB, B, 3) or null
};

// resident_ingest_kernel's argument block
struct ResidentIngestArgs {
    ResidentGeom g;
    const ResidentObj* objs;
    int n_store_objs, max_views;
    const int32_t *obj_of, *view_of;   // (n_out) each
    float* out;                        // (n_out, 3, OH, OW)
    int tiles_x, tiles_y;              // workgroups per view along x and y (INGEST_TILE_X x INGEST_TILE_Y output pixels each)
};

}  // namespace pny
