// A step's ray batch, ground truth and source views drawn straight from decoded views that stay on the device as bytes
// (arithmetic in pny_resident.h, pny_ingest.h, pny_train_batch.h, pny_ray.h; entry points in resident_api.hip).  What the
// reference does per step on the host before its trainer starts -- SRNDataset.__getitem__ / DVRDataset.__getitem__ decode,
// normalise and resize ALL views of every object of the super-batch, the DataLoader copies them over, and
// train/trainlib/PixelNerfTrainer.py:76-133 reads 128 pixels and at most 3 views per object from them -- for the pixels and
// views the step keeps.
//
// Launches: pny_resident_train_batch is ONE launch (resident_batch_kernel), pny_ingest_views_indexed is ONE launch
// (resident_ingest_kernel).  No atomics: every output element has one writer and every sum a fixed order, so a call gives the
// same bits on every run.  Object ids, view ids, view counts and draws come from device memory and are clamped into range.
//
// resident_batch_kernel: one thread per (share s, ray r), bound by latency, not by traffic (SB * B is a few hundred to a few
// thousand rays): it reads the share's record, picks its pixel as train_batch_kernel does on an object of the record's own
// view count, builds that pixel's ray from the object's pose row, and computes the ingest's fp32 value of that ONE output
// pixel: a byte triple, four of them, or an area window in ingest's order.  64-bit offsets throughout.
//
// resident_ingest_kernel: ingest_kernel (ingest.hip) with the view's base pointer looked up per workgroup: the grid runs over
// output views x tiles of 4 rows x 64 columns, a wave per row with its lanes along output x; the source pixel comes through
// aligned dword loads.
#include <hip/hip_runtime.h>

#include "pny_ray.h"
#include "pny_resident.h"

namespace pny {
namespace {

// the record of store object `id` (clamped), with its view count clamped
__device__ __forceinline__ ResidentObj resident_obj(const ResidentObj* objs, int n_store_objs, int max_views, int32_t id, int& obj) {
    obj = resident_clamp(id, n_store_objs);
    ResidentObj o = objs[obj];
    o.n_views = resident_view_count(o.n_views, max_views);
    return o;
}

__global__ __launch_bounds__(RESIDENT_BATCH_THREADS) void resident_batch_kernel(const ResidentBatchArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)a.sb * a.b) return;
    const int s = (int)(i / a.b);
    int obj;
    const ResidentObj o = resident_obj(a.objs, a.n_store_objs, a.max_views, a.obj_ids[s], obj);
    const int nv = o.n_views;
    const size_t row0 = (size_t)resident_first_row(o.first_row, nv, a.n_rows);
    const BatchPixel p = resident_pick(nv, a.g.oh, a.g.ow, a.bboxes ? a.bboxes + row0 * 4 : nullptr, a.seed,
                                       a.draw_offset + (uint64_t)i, a.pix_inds ? a.pix_inds + i : nullptr,
                                       a.image_ids ? a.image_ids + i : nullptr, a.u_x ? a.u_x + i : nullptr,
                                       a.u_y ? a.u_y + i : nullptr);
    const float* f = a.focal + (size_t)obj * 2;
    const float* cc = a.c ? a.c + (size_t)obj * 2 : nullptr;
    float c[16];
    cam16_from_pose(a.poses + (row0 + (size_t)p.view) * 16, f[0], f[1], cc ? cc[0] : (float)a.g.ow * 0.5f,
                    cc ? cc[1] : (float)a.g.oh * 0.5f, c);
    float d0, d1, d2;
    pinhole_dir(c, p.x, p.y, d0, d1, d2);
    store_ray(c, d0, d1, d2, a.znear, a.zfar, a.rays + i * 8);
    const uint8_t* img = o.views + (size_t)p.view * a.g.h * a.g.w * a.g.c;
    float rgb[3];
    resident_rgb(img, a.g, p.y, p.x, IngestLoadDwords(), rgb);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) a.rgb[i * 3 + ch] = rgb[ch];
    if (a.pix) {
        a.pix[i * 3 + 0] = p.view;
        a.pix[i * 3 + 1] = p.y;
        a.pix[i * 3 + 2] = p.x;
    }
}

__global__ __launch_bounds__(INGEST_TILE_X* INGEST_TILE_Y) void resident_ingest_kernel(const ResidentIngestArgs a) {
    const unsigned per_view = (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    const unsigned view = blockIdx.x / per_view, tile = blockIdx.x - view * per_view;
    const int ty = (int)(tile / (unsigned)a.tiles_x), tx = (int)(tile - (unsigned)ty * (unsigned)a.tiles_x);
    const int x = tx * INGEST_TILE_X + (int)threadIdx.x, y = ty * INGEST_TILE_Y + (int)threadIdx.y;
    if (x >= a.g.ow || y >= a.g.oh) return;
    int obj;
    const ResidentObj o = resident_obj(a.objs, a.n_store_objs, a.max_views, a.obj_of[view], obj);
    const int v = resident_clamp(a.view_of[view], o.n_views);
    const uint8_t* img = o.views + (size_t)v * a.g.h * a.g.w * a.g.c;
    const size_t plane = (size_t)a.g.oh * a.g.ow;
    float* out = a.out + (size_t)view * 3 * plane + (size_t)y * a.g.ow + x;
    float r, g, b, m;
    ingest_pixel(img, a.g, y, x, IngestLoadDwords(), r, g, b, m);
    out[0] = r, out[plane] = g, out[2 * plane] = b;
}

}  // namespace

void launch_resident_batch(const ResidentBatchArgs& a, hipStream_t st) {
    const long long n = (long long)a.sb * a.b;
    const unsigned blocks = (unsigned)((n + RESIDENT_BATCH_THREADS - 1) / RESIDENT_BATCH_THREADS);
    hipLaunchKernelGGL(resident_batch_kernel, dim3(blocks), dim3(RESIDENT_BATCH_THREADS), 0, st, a);
}

void launch_resident_ingest(const ResidentIngestArgs& a, int n_out, hipStream_t st) {
    const unsigned blocks = (unsigned)n_out * (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    hipLaunchKernelGGL(resident_ingest_kernel, dim3(blocks), dim3(INGEST_TILE_X, INGEST_TILE_Y), 0, st, a);
}

}  // namespace pny
