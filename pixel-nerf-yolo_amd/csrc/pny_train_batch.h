// Which pixel a ray of a training batch looks through (reference train/trainlib/PixelNerfTrainer.py:108-112 and
// src/util/util.py:222-237 bbox_sample, restated per ray).  Used by train_batch_kernel (render_kernels.hip); like pny_rng.h it
// also compiles for the host (__device__ defined away), which is how tests/test_cpu_train_batch.py runs it without a GPU.
#pragma once
#include <stdint.h>

#include "pny_rng.h"

namespace pny {

struct BatchPixel {
    int view, y, x;
};

// uniform mode: a flat index into the (NV, H, W) pixel grid (PixelNerfTrainer.py:112).  An index outside [0, NV*H*W) is
// clamped to the grid (memory safety for replayed draws only; a seeded draw is always inside).
__device__ __forceinline__ BatchPixel pixel_from_flat(int64_t flat, int nv, int h, int w) {
    const int64_t per = (int64_t)h * w, total = per * nv;
    flat = flat < 0 ? 0 : (flat >= total ? total - 1 : flat);
    BatchPixel p;
    p.view = (int)(flat / per);
    const int64_t rem = flat - p.view * per;   // (one image may hold more than 2^31 pixels)
    p.y = (int)(rem / w);
    p.x = (int)(rem - (int64_t)p.y * w);
    return p;
}

// bbox mode: one coordinate of util.py:228-235, `(u * (max + 1 - min) + min).long()` -- fp32, the product rounded before
// the sum (no fused multiply-add), truncated toward zero.  The clamp to [0, size - 1] is a memory-safety guard that a box
// inside the image never reaches; it is applied before the conversion, where it gives the same integer as truncating first
// (trunc of a value in (-1, 0) is 0) and keeps a NaN or huge coordinate out of the float -> int conversion.
__device__ __forceinline__ int bbox_coord(float u, float lo, float hi, int size) {
    const float span = hi + 1.0f - lo;
    const float prod = u * span;
    float t = prod + lo;
    t = t >= 0.0f ? t : 0.0f;   // also catches NaN
    t = t <= (float)(size - 1) ? t : (float)(size - 1);
    return (int)t;
}

// box: cmin rmin cmax rmax of image `view` (already clamped to [0, nv))
__device__ __forceinline__ BatchPixel pixel_from_bbox(int view, float u_x, float u_y, const float* box, int h, int w) {
    BatchPixel p;
    p.view = view;
    p.x = bbox_coord(u_x, box[0], box[2], w);
    p.y = bbox_coord(u_y, box[1], box[3], h);
    return p;
}

__device__ __forceinline__ int clamp_view(int64_t v, int nv) { return v < 0 ? 0 : (v >= nv ? nv - 1 : (int)v); }

// The seeded draws of ray `idx` (= draw_offset + s * B + r): one integer or one integer and two uniforms, each from its own
// stream at the same position, so an object's batch does not depend on how many other objects the call holds.
__device__ __forceinline__ int64_t seeded_flat(uint64_t seed, uint64_t idx, uint32_t n_pixels) {
    return (int64_t)index_at(seed, STREAM_BATCH_PIX, idx, n_pixels);
}
__device__ __forceinline__ int seeded_view(uint64_t seed, uint64_t idx, int nv) {
    return (int)index_at(seed, STREAM_BATCH_VIEW, idx, (uint32_t)nv);
}
__device__ __forceinline__ float seeded_u_x(uint64_t seed, uint64_t idx) { return uniform_at(seed, STREAM_BATCH_X, idx); }
__device__ __forceinline__ float seeded_u_y(uint64_t seed, uint64_t idx) { return uniform_at(seed, STREAM_BATCH_Y, idx); }

}  // namespace pny
