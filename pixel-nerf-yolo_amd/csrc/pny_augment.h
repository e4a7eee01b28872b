// The arithmetic of the colour jitter (augment.hip; entry point in augment_api.hip): data.ColorJitterDataset's chain on one
// image, as data.adjust_saturation / adjust_hue / adjust_contrast / adjust_brightness define it, all in fp32:
//   input       t = (x + 1) * 0.5 of the dataset's [-1, 1] floats, or t = x / 255 of imread's bytes
//   grey        0.2989 r + 0.587 g + 0.114 b, left to right
//   blend       blend(a, b, ratio) = clamp(ratio a + (1 - ratio) b, 0, 1)
//   saturation  blend(t, grey(t), sat) per channel
//   hue         RGB -> HSV (maxc == minc gives s = 0, h = 0; the cases maxc == r, g, b in that order), h = fmod(h / 6 + 1, 1),
//               h = (h + hue) mod 1 >= 0, HSV -> RGB by the six-sector table with p, q, t clamped to [0, 1]
//   contrast    blend(t, mean, con), mean = the image's mean grey level after saturation and hue
//   brightness  blend(t, 0, bri)
//   output      t * 2 - 1
// The chain is continuous across each of its branches (grey pixels, the hue wrap, the sector boundaries, the clamps), so two
// implementations that take different branches on a boundary pixel still agree to rounding.
// Like pny_metrics.h it also compiles for the host (__device__ defined away), which is how tests/test_cpu_augment.py runs it
// without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

namespace pny {

constexpr int JITTER_THREADS = 1024;        // one workgroup owns one image
constexpr int JITTER_MAX_OBJS = 64;         // objects per launch (include/pnyolo.h PNY_JITTER_MAX_OBJS)

// pny_color_jitter_desc::in_format (include/pnyolo.h PNY_IMG_*)
enum { JITTER_F32_NCHW_PM1 = 0, JITTER_U8_NHWC = 1 };

__device__ __forceinline__ float jitter_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__device__ __forceinline__ float jitter_from_pm1(float x) { return (x + 1.0f) * 0.5f; }
__device__ __forceinline__ float jitter_from_byte(uint8_t x) { return (float)x / 255.0f; }
__device__ __forceinline__ float jitter_to_pm1(float t) { return t * 2.0f - 1.0f; }

__device__ __forceinline__ float jitter_grey(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

__device__ __forceinline__ float jitter_blend(float a, float b, float ratio) {
    return jitter_clamp01(ratio * a + (1.0f - ratio) * b);
}

// x - floor(x): fmod(x, 1) for x >= 0 and the non-negative remainder for x < 0, both exact
__device__ __forceinline__ float jitter_frac(float x) { return x - floorf(x); }

__device__ __forceinline__ void jitter_saturation(float& r, float& g, float& b, float sat) {
    const float y = jitter_grey(r, g, b);
    r = jitter_blend(r, y, sat), g = jitter_blend(g, y, sat), b = jitter_blend(b, y, sat);
}

// data.adjust_hue on one pixel in [0, 1].  Of rc, gc, bc only the two the taken case uses are formed: the same quotients.
__device__ __forceinline__ void jitter_hue(float& r, float& g, float& b, float hue) {
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float crd = eqc ? 1.0f : cr;
    // h = off + n1 / crd - n2 / crd; selects, not branches: neighbouring pixels take different cases
    const bool is_r = maxc == r, is_g = maxc == g;
    const float off = is_r ? 0.0f : (is_g ? 2.0f : 4.0f);
    const float n1 = maxc - (is_r ? b : (is_g ? r : g)), n2 = maxc - (is_r ? g : (is_g ? b : r));
    float h = (off + n1 / crd) - n2 / crd;
    h = jitter_frac(h / 6.0f + 1.0f);
    h = jitter_frac(h + hue);
    const float h6 = h * 6.0f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    const int sector = fl >= 6.0f ? 0 : (int)fl;   // h rounds to 1 for a tiny negative h + hue: sector 6 is sector 0
    const float v = maxc;
    const float p = jitter_clamp01(v * (1.0f - s));
    const float q = jitter_clamp01(v * (1.0f - s * f));
    const float t = jitter_clamp01(v * (1.0f - s * (1.0f - f)));
    // the six-sector table r: v q p p t v, g: t v v q p p, b: p p t v v q
    r = (sector == 0 || sector == 5) ? v : (sector == 1 ? q : (sector == 4 ? t : p));
    g = (sector == 1 || sector == 2) ? v : (sector == 0 ? t : (sector == 3 ? q : p));
    b = (sector == 3 || sector == 4) ? v : (sector == 2 ? t : (sector == 5 ? q : p));
}

// Saturation and hue of one pixel in [0, 1]; returns its grey level, one term of the contrast mean.
__device__ __forceinline__ float jitter_first(float& r, float& g, float& b, float hue, float sat) {
    jitter_saturation(r, g, b, sat);
    jitter_hue(r, g, b, hue);
    return jitter_grey(r, g, b);
}

// Contrast against the image's mean grey level, brightness, and the map back to [-1, 1].
__device__ __forceinline__ float jitter_second(float t, float mean, float con, float bri) {
    t = jitter_blend(t, mean, con);
    t = jitter_blend(t, 0.0f, bri);
    return jitter_to_pm1(t);
}

// the mean grey level from the fp64 sum over the image's pixels, rounded once to fp32
__device__ __forceinline__ float jitter_mean(double sum, int pixels) { return (float)(sum / (double)pixels); }

struct JitterFactors {
    float hue, sat, bri, con;
};

struct JitterArgs {
    const void* in;          // (n_objs * n_views, 3, H, W) fp32 or (n_objs * n_views, H, W, 3) bytes
    float* out;              // (n_objs * n_views, 3, H, W); may be `in` for the float format
    int n_views, hw, format; // views per object, H * W, JITTER_*
    JitterFactors f[JITTER_MAX_OBJS];   // per object, in the kernel-argument segment (as MlpArgs carries the cameras)
};

}  // namespace pny
