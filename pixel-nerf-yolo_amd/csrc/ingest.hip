// From decoded bytes to the tensors the trainer uses, on the device (arithmetic in pny_ingest.h): what data.YOLODataset and
// data.SRNDataset do per view on the host after imread -- resize, normalise, white-background mask and its bounding box -- and
// the YOLO target grids of YOLODataset._get_all_bboxes.
//
// Launches: pny_ingest_views is ONE launch (ingest_kernel), TWO with white_mask (ingest_box_kernel after it, one workgroup per
// view); pny_yolo_build_targets is ONE launch (targets_kernel).  No atomics anywhere: every output element has one writer and
// every sum a fixed order, so a view gives the same bits alone as inside a batch, on every run.
//
// ingest_kernel: bound by memory traffic.  The grid runs over views x output tiles of 4 rows x 64 columns, a wave per row with
// its lanes along output x, so a single 400 x 400 view is 700 workgroups and the three planar fp32 stores of a wave are 256
// contiguous bytes each.  A source pixel is three bytes at any alignment (channels = 3 rows start anywhere): it is fetched as
// the one or two ALIGNED dwords that hold it and shifted out, never as byte loads.  Both dwords hold at least one byte of the
// pixel, so they lie in pages the buffer owns.  channels = 4 on a 4-byte aligned base is one dword per pixel.
//   none      one pixel per thread
//   bilinear  four pixels per thread, blended per channel to a byte (rows first, round half to even), then the byte map
//   area      the window's pixels in row-major order, mapped, summed in fp32, one division; the mask rides the same windows
//
// ingest_box_kernel: the one reduction.  A workgroup scans its view at decoded resolution with integer min / max per thread, a
// wave shuffle tree and an LDS tree over the four waves; thread 0 writes [cmin, rmin, cmax, rmax], scaled where the view was
// resized, or [W, H, -1, -1] for an empty mask.  Integer min / max are order independent: bit-reproducible.  SRN views are
// 128 x 128: 64 pixels per thread.
//
// targets_kernel: one workgroup per view.  All threads zero the view's grids; a workgroup-scope fence and a barrier order the
// fill before the walk; thread 0 then walks the view's boxes in file order (each depends on the slots the earlier ones took),
// reading back only slots that the fill or it itself has written.
#include <hip/hip_runtime.h>

#include "pny_ingest.h"

namespace pny {
namespace {

// the three bytes at p, through aligned dword loads
__device__ __forceinline__ IngestPx load_px(const uint8_t* p) { return IngestLoadDwords()(p); }

__global__ __launch_bounds__(INGEST_TILE_X* INGEST_TILE_Y) void ingest_kernel(IngestArgs a) {
    const unsigned per_view = (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    const unsigned view = blockIdx.x / per_view, tile = blockIdx.x - view * per_view;
    const int ty = (int)(tile / (unsigned)a.tiles_x), tx = (int)(tile - (unsigned)ty * (unsigned)a.tiles_x);
    const int x = tx * INGEST_TILE_X + (int)threadIdx.x, y = ty * INGEST_TILE_Y + (int)threadIdx.y;
    if (x >= a.ow || y >= a.oh) return;
    const uint8_t* img = a.in + (size_t)view * a.h * a.w * a.c;
    const size_t plane = (size_t)a.oh * a.ow;
    const size_t o = (size_t)y * a.ow + x;
    float* out = a.out + (size_t)view * 3 * plane + o;
    float r, g, b, m;
    ingest_pixel(img, a, y, x, IngestLoadDwords(), r, g, b, m);
    out[0] = r, out[plane] = g, out[2 * plane] = b;
    if (a.mask) a.mask[(size_t)view * plane + o] = m;
}

__global__ __launch_bounds__(INGEST_BOX_THREADS) void ingest_box_kernel(IngestBoxArgs a) {
    constexpr int WAVES = INGEST_BOX_THREADS / 64;
    __shared__ int red[WAVES][4];
    const int tid = (int)threadIdx.x;
    const uint8_t* img = a.in + (size_t)blockIdx.x * a.h * a.w * a.c;
    const unsigned hw = (unsigned)a.h * (unsigned)a.w;
    int cmin = a.w, rmin = a.h, cmax = -1, rmax = -1;
#pragma unroll 4
    for (unsigned i = (unsigned)tid; i < hw; i += INGEST_BOX_THREADS) {     // consecutive lanes, consecutive pixels
        const IngestPx p = load_px(img + (size_t)i * a.c);
        if (ingest_white_mask(p.r, p.g, p.b) != 0.0f) {
            const int y = (int)(i / (unsigned)a.w), x = (int)(i - (unsigned)y * (unsigned)a.w);
            cmin = min(cmin, x), cmax = max(cmax, x);
            rmin = min(rmin, y), rmax = max(rmax, y);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        cmin = min(cmin, __shfl_xor(cmin, o, 64)), rmin = min(rmin, __shfl_xor(rmin, o, 64));
        cmax = max(cmax, __shfl_xor(cmax, o, 64)), rmax = max(rmax, __shfl_xor(rmax, o, 64));
    }
    if ((tid & 63) == 0) red[tid >> 6][0] = cmin, red[tid >> 6][1] = rmin, red[tid >> 6][2] = cmax, red[tid >> 6][3] = rmax;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < WAVES; ++w) {
            cmin = min(cmin, red[w][0]), rmin = min(rmin, red[w][1]);
            cmax = max(cmax, red[w][2]), rmax = max(rmax, red[w][3]);
        }
        float v[4] = {(float)cmin, (float)rmin, (float)cmax, (float)rmax};
        if (a.scaled && cmax >= 0)
            for (int i = 0; i < 4; ++i) v[i] = v[i] * a.scale;
        float* o = a.bbox + (size_t)blockIdx.x * 4;
        for (int i = 0; i < 4; ++i) o[i] = v[i];
    }
}

__global__ __launch_bounds__(TARGETS_THREADS) void targets_kernel(TargetsArgs a) {
    __shared__ float iou[TARGETS_MAX_ANCHORS];
    const size_t view = blockIdx.x;
    float* grid[TARGETS_MAX_SCALES];
#pragma unroll
    for (int s = 0; s < TARGETS_MAX_SCALES; ++s) {
        grid[s] = nullptr;
        if (s < a.g.n_scales) {
            const size_t n = (size_t)a.g.hs[s] * a.g.ws[s] * a.g.n_anchors * 6;
            grid[s] = a.grid[s] + view * n;
            for (size_t i = threadIdx.x; i < n; i += TARGETS_THREADS) grid[s][i] = 0.0f;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    int n = a.n_boxes[view];
    n = n < 0 ? 0 : (n > a.max_boxes ? a.max_boxes : n);
    const double* boxes = a.boxes + view * (size_t)a.max_boxes * 5;
    for (int b = 0; b < n; ++b) targets_assign_box(a.g, boxes + (size_t)b * 5, grid, iou);
}

}  // namespace

void launch_ingest(const IngestArgs& a, int n_views, hipStream_t st) {
    const unsigned blocks = (unsigned)n_views * (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    hipLaunchKernelGGL(ingest_kernel, dim3(blocks), dim3(INGEST_TILE_X, INGEST_TILE_Y), 0, st, a);
}

void launch_ingest_box(const IngestBoxArgs& a, int n_views, hipStream_t st) {
    hipLaunchKernelGGL(ingest_box_kernel, dim3((unsigned)n_views), dim3(INGEST_BOX_THREADS), 0, st, a);
}

void launch_targets(const TargetsArgs& a, int n_views, hipStream_t st) {
    hipLaunchKernelGGL(targets_kernel, dim3((unsigned)n_views), dim3(TARGETS_THREADS), 0, st, a);
}

}  // namespace pny
