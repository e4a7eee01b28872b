// The arithmetic between "PNG decoded" and "tensor the trainer uses" (ingest.hip; entry points in ingest_api.hip), all in fp32:
//   byte map    t = b / 255, out = (t - 0.5) / 0.5: data.image_to_tensor_balanced, bit for bit for all 256 bytes
//   bilinear    data.resize_bilinear_u8: half-pixel centres, src = max(scale (dst + 0.5) - 0.5, 0) (fused) with scale = in / out,
//               i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), lambda = src - i0; the four taps blended rows first,
//               rounded half to even back to a byte, clamped to 0 .. 255, then the byte map
//   area        F.interpolate(mode="area") of the mapped values: window [floor(i in / out), ceil((i + 1) in / out)) per axis, an
//               fp32 sum in row-major order and one division by the element count
//   white mask  SRNDataset.__getitem__ (data.py:112): 1 where none of the three bytes is 255, else 0
//   yolo walk   YOLODataset._get_all_bboxes (data.py:203-227) over the boxes of one view, in file order
// Like pny_augment.h it also compiles for the host (__host__ / __device__ defined away), which is how tests/test_cpu_ingest.py
// runs it without a GPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace pny {

constexpr int INGEST_TILE_X = 64, INGEST_TILE_Y = 4;   // output pixels of one workgroup: a wave per row, lanes along x
constexpr int INGEST_BOX_THREADS = 256;                // the box kernel: one workgroup per view
constexpr int TARGETS_THREADS = 256;                   // the target kernel: one workgroup per view
constexpr int TARGETS_MAX_SCALES = 4;                  // include/pnyolo.h PNY_YOLO_BATCH_MAX_SCALES
constexpr int TARGETS_MAX_ANCHORS = 64;                // n_scales * n_anchors

// pny_ingest_desc::resize (include/pnyolo.h PNY_RESIZE_*)
enum { INGEST_RESIZE_NONE = 0, INGEST_RESIZE_BILINEAR_U8 = 1, INGEST_RESIZE_AREA = 2 };

__host__ __device__ inline float ingest_byte_map(uint32_t b) {
    const float t = (float)b / 255.0f;
    return (t - 0.5f) / 0.5f;
}

// 1 inside the object: none of the three bytes is 255, `(img != 255).all(axis=-1)`
__host__ __device__ inline float ingest_white_mask(uint32_t r, uint32_t g, uint32_t b) {
    return (r != 255u && g != 255u && b != 255u) ? 1.0f : 0.0f;
}

// the two taps and the weight of the second for output index dst; scale = (float)in / (float)out
__host__ __device__ inline void ingest_bilinear_taps(int dst, float scale, int in, int& i0, int& i1, float& lambda) {
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);   // one rounding, as torch's kernels on the host
    src = src < 0.0f ? 0.0f : src;
    const int f = (int)src;                       // src >= 0: truncation is floor
    i0 = f < in - 1 ? f : in - 1;
    i1 = i0 + 1 < in - 1 ? i0 + 1 : in - 1;
    lambda = src - (float)i0;
}

// the byte of four taps (a b in row y0, c d in row y1)
__host__ __device__ inline uint32_t ingest_bilinear_u8(uint32_t a, uint32_t b, uint32_t c, uint32_t d, float lx, float ly) {
    const float wx0 = 1.0f - lx, wy0 = 1.0f - ly;
    const float top = wx0 * (float)a + lx * (float)b, bot = wx0 * (float)c + lx * (float)d;
    float v = rintf(wy0 * top + ly * bot);        // round half to even
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return (uint32_t)v;
}

// the window of output index i: [start, end), never empty
__host__ __device__ inline void ingest_area_window(int i, int in, int out, int& start, int& end) {
    start = (int)(((int64_t)i * in) / out);
    end = (int)((((int64_t)i + 1) * in + out - 1) / out);
}

// ---- one output pixel of the ingest, for ingest_kernel (ingest.hip) and the resident store's kernels (resident.hip)
struct IngestPx {
    uint32_t r, g, b;
};

// the three bytes at p, one byte load each (the host's loader; any alignment, nothing beyond the pixel is read)
struct IngestLoadBytes {
    __host__ __device__ inline IngestPx operator()(const uint8_t* p) const {
        IngestPx px;
        px.r = p[0], px.g = p[1], px.b = p[2];
        return px;
    }
};

// the three bytes at p, through the one or two ALIGNED dwords that hold them (the kernels' loader): both dwords hold at least
// one byte of the pixel, so they lie in pages the buffer owns
struct IngestLoadDwords {
    __host__ __device__ inline IngestPx operator()(const uint8_t* p) const {
        const uintptr_t a = (uintptr_t)p;
        const unsigned sh = (unsigned)(a & 3);
        const uint32_t* q = (const uint32_t*)(a - sh);
        uint32_t v = q[0] >> (8 * sh);
        if (sh > 1) v |= q[1] << (32 - 8 * sh);        // bytes sh .. sh + 2 run into the next dword
        IngestPx px;
        px.r = v & 255u, px.g = (v >> 8) & 255u, px.b = (v >> 16) & 255u;
        return px;
    }
};

// Output pixel (y, x) of the view at img (H, W, C bytes): r g b as pny_ingest_views writes them and the mask value m (none and
// area only; 0 under bilinear).  Geom carries h, w, c, oh, ow, resize, scale_y, scale_x (IngestArgs, ResidentGeom).
template <class Geom, class Load>
__host__ __device__ inline void ingest_pixel(const uint8_t* img, const Geom& a, int y, int x, Load load, float& r, float& g,
                                             float& b, float& m) {
    const size_t row_bytes = (size_t)a.w * a.c;
    m = 0.0f;
    if (a.resize == INGEST_RESIZE_NONE) {
        const IngestPx p = load(img + (size_t)y * row_bytes + (size_t)x * a.c);
        r = ingest_byte_map(p.r), g = ingest_byte_map(p.g), b = ingest_byte_map(p.b);
        m = ingest_white_mask(p.r, p.g, p.b);
    } else if (a.resize == INGEST_RESIZE_BILINEAR_U8) {
        int y0, y1, x0, x1;
        float ly, lx;
        ingest_bilinear_taps(y, a.scale_y, a.h, y0, y1, ly);
        ingest_bilinear_taps(x, a.scale_x, a.w, x0, x1, lx);
        const uint8_t *r0 = img + (size_t)y0 * row_bytes, *r1 = img + (size_t)y1 * row_bytes;
        const IngestPx p00 = load(r0 + (size_t)x0 * a.c), p01 = load(r0 + (size_t)x1 * a.c);
        const IngestPx p10 = load(r1 + (size_t)x0 * a.c), p11 = load(r1 + (size_t)x1 * a.c);
        r = ingest_byte_map(ingest_bilinear_u8(p00.r, p01.r, p10.r, p11.r, lx, ly));
        g = ingest_byte_map(ingest_bilinear_u8(p00.g, p01.g, p10.g, p11.g, lx, ly));
        b = ingest_byte_map(ingest_bilinear_u8(p00.b, p01.b, p10.b, p11.b, lx, ly));
    } else {
        int ys, ye, xs, xe;
        ingest_area_window(y, a.h, a.oh, ys, ye);
        ingest_area_window(x, a.w, a.ow, xs, xe);
        r = g = b = 0.0f;
        for (int yy = ys; yy < ye; ++yy) {
            const uint8_t* row = img + (size_t)yy * row_bytes;
            for (int xx = xs; xx < xe; ++xx) {
                const IngestPx p = load(row + (size_t)xx * a.c);
                r += ingest_byte_map(p.r), g += ingest_byte_map(p.g), b += ingest_byte_map(p.b);
                m += ingest_white_mask(p.r, p.g, p.b);
            }
        }
        const float count = (float)((ye - ys) * (xe - xs));
        r = r / count, g = g / count, b = b / count, m = m / count;
    }
}

// ---- YOLO target grids
struct TargetsGeom {
    int n_scales, n_anchors;                      // anchors per scale
    int hs[TARGETS_MAX_SCALES], ws[TARGETS_MAX_SCALES];
    float thresh;
    float anchors[TARGETS_MAX_ANCHORS * 2];       // (n_scales * n_anchors, 2) w h
};

// util.iou(..., is_pred=False) of one (w, h) pair against one anchor, as data.iou_wh orders it
__host__ __device__ inline float targets_iou_wh(float w, float h, float aw, float ah) {
    const float inter = (w < aw ? w : aw) * (h < ah ? h : ah);
    const float uni = (w * h + aw * ah) - inter;
    return inter / uni;
}

// One box {cx, cy, w, h, cls} into one view's grids (zero filled before the first box; grid[s] is (hs, ws, A, 6)).  Anchors are
// visited by descending IoU, ties by ascending index.  A box whose cell lies outside a grid is left out of that grid.
// iou: n_scales * n_anchors floats of scratch.
__host__ __device__ inline void targets_assign_box(const TargetsGeom& g, const double* box, float* const* grid, float* iou) {
    const double x = box[0], y = box[1], bw = box[2], bh = box[3];
    const float wf = (float)bw, hf = (float)bh;
    const int na = g.n_scales * g.n_anchors;
    for (int a = 0; a < na; ++a) iou[a] = targets_iou_wh(wf, hf, g.anchors[2 * a], g.anchors[2 * a + 1]);
    uint64_t visited = 0;
    uint32_t has_anchor = 0;
    for (int k = 0; k < na; ++k) {
        int best = -1;
        for (int a = 0; a < na; ++a)
            if (!((visited >> a) & 1) && (best < 0 || iou[a] > iou[best])) best = a;
        visited |= (uint64_t)1 << best;
        const int s = best / g.n_anchors, on_scale = best % g.n_anchors;
        const int hs = g.hs[s], ws = g.ws[s];
        const double fy = (double)hs * y, fx = (double)ws * x;
        if (!(fy >= 0.0 && fy < (double)hs && fx >= 0.0 && fx < (double)ws)) continue;
        const int i = (int)fy, j = (int)fx;
        float* slot = grid[s] + (((size_t)i * ws + j) * g.n_anchors + on_scale) * 6;
        if (slot[0] != 0.0f) continue;             // taken, or marked ignored
        if (!((has_anchor >> s) & 1)) {
            slot[0] = 1.0f;
            slot[1] = (float)(fx - (double)j);
            slot[2] = (float)(fy - (double)i);
            slot[3] = (float)(bw * (double)ws);
            slot[4] = (float)(bh * (double)hs);
            slot[5] = (float)(int64_t)box[4];
            has_anchor |= 1u << s;
        } else if (iou[best] > g.thresh) {
            slot[0] = -1.0f;
        }
    }
}

struct IngestArgs {
    const uint8_t* in;       // (NV, H, W, C) bytes
    float* out;              // (NV, 3, OH, OW)
    float* mask;             // (NV, 1, OH, OW) or null
    int h, w, c, oh, ow, resize;
    int tiles_x, tiles_y;    // workgroups per view along x and y
    float scale_y, scale_x;  // bilinear: (float)in / (float)out
};

struct IngestBoxArgs {
    const uint8_t* in;
    float* bbox;             // (NV, 4) cmin rmin cmax rmax
    int h, w, c;
    int scaled;              // multiply a non-empty box by `scale`
    float scale;
};

struct TargetsArgs {
    TargetsGeom g;
    const double* boxes;     // (NV, max_boxes, 5)
    const int32_t* n_boxes;  // (NV)
    float* grid[TARGETS_MAX_SCALES];   // (NV, hs, ws, A, 6) per scale
    int max_boxes;
};

}  // namespace pny
