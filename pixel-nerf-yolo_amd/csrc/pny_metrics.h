// The arithmetic of the view metrics (metrics.hip; entry point in metrics_api.hip): what the reference's eval scripts compute
// on the host for every rendered view (eval/eval.py:288-345, eval/calc_metrics.py:189-191, src/util/util.py:502-509).
//   prediction  x = clamp(rgb, 0, 1) in fp32 (eval.py:288); a NaN stays a NaN
//   byte        (uint8) trunc(fl32(x * 255)), numpy's (all_rgb * 255).astype(np.uint8) on fp32 (eval.py:291); a NaN gives 0
//   ground truth  taken as given (calc_metrics.py), or fl32(g * 0.5 + 0.5) of the dataset's [-1, 1] images (eval.py:315)
//   SSIM        skimage's compare_ssim(multichannel=True, data_range=1): win_size 7, uniform window, sample covariance,
//               K1 = 0.01, K2 = 0.03; the mean of S over the windows that lie wholly inside the image (skimage crops 3 pixels
//               of its filtered map, so its boundary mode never reaches the result), per channel, then over the 3 channels
//   PSNR        10 log10(1 / mean((x - y)^2)), everything in fp64; identical images give +inf
// Like pny_train_batch.h it also compiles for the host (__device__ defined away), which is how tests/test_cpu_metrics.py runs
// it without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

namespace pny {

constexpr int METRICS_WIN = 7;              // SSIM window (win_size); the only one this build has
constexpr int METRICS_APRON = METRICS_WIN - 1;
// One workgroup's tile of output windows (window = its top-left pixel).  It stages (TILE_H + 6) x (TILE_W + 6) pixels of both
// images in LDS as fp32 (2 x 10 032 bytes) and one channel's row sums of 7, five fp64 moments of (TILE_H + 6) x TILE_W
// positions (28 160 bytes): 48 KiB, three workgroups per CU.  TILE_W = 32 doubles = one 256-byte row of the row-sum
// image: a wave's two rows of 32 consecutive 8-byte elements are read conflict-free (ds_read_b64: 64 banks of 4 bytes), and
// the fp32 staging image is read at a stride of 3 floats (channel-interleaved), which is coprime with the bank count.
constexpr int METRICS_TILE_H = 16;
constexpr int METRICS_TILE_W = 32;
constexpr int METRICS_THREADS = 256;
constexpr int METRICS_FLAT_CHUNK = 4096;    // elements per workgroup of the flat form (PNY_GT_FLAT)
constexpr int METRICS_SUMS = 2;             // partial sums per workgroup: {sum of squared errors, sum of S}

// pny_view_metrics_desc::gt_layout (include/pnyolo.h PNY_GT_*)
enum { METRICS_GT_NHWC_01 = 0, METRICS_GT_NCHW_PM1 = 1, METRICS_GT_FLAT = 2 };

// eval.py:288.  Comparisons, not fminf / fmaxf: a NaN passes through (as torch.clamp and np.clip pass it).
__device__ __forceinline__ float metrics_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// eval.py:291 on a clamped value: the fp32 product (one rounding, no reciprocal), truncated.  NaN -> 0.
__device__ __forceinline__ uint8_t metrics_byte(float x) {
    const float p = x * 255.0f;
    return p == p ? (uint8_t)(int)p : (uint8_t)0;
}

// eval.py:315 `images * 0.5 + 0.5` in fp32: g * 0.5 is exact, so the sum is the only rounding, fused or not.
__device__ __forceinline__ float metrics_gt_from_pm1(float g) { return g * 0.5f + 0.5f; }

// S of one window from its five sums over the 49 pixels (skimage structural_similarity, use_sample_covariance=True).
__device__ __forceinline__ double metrics_ssim_window(double sx, double sy, double sxx, double syy, double sxy) {
    const double NP = (double)(METRICS_WIN * METRICS_WIN), cov_norm = NP / (NP - 1.0);
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;      // (K data_range)^2, data_range = 1
    const double ux = sx / NP, uy = sy / NP;
    const double vx = cov_norm * (sxx / NP - ux * ux), vy = cov_norm * (syy / NP - uy * uy), vxy = cov_norm * (sxy / NP - ux * uy);
    const double a1 = 2.0 * ux * uy + C1, a2 = 2.0 * vxy + C2, b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
    return (a1 * a2) / (b1 * b2);
}

// compare_psnr(data_range=1) / util.psnr from the sum of squared errors over n elements
__device__ __forceinline__ double metrics_psnr(double sse, double n) { return 10.0 * log10(1.0 / (sse / n)); }

// tiles along one axis of `size` pixels: its size - 6 window positions in tiles of `tile`
constexpr int metrics_tiles(int size, int tile) { return (size - METRICS_APRON + tile - 1) / tile; }

struct ViewMetricsArgs {
    const float* rgb;        // (NV, H, W, 3); flat form: (NV, n)
    const float* gt;         // (NV, H, W, 3) or (NV, 3, H, W); flat form: (NV, n)
    double* metrics;         // (NV, 2) {psnr, ssim}, or null: convert only
    uint8_t* rgb8;           // (NV, H, W, 3), or null
    int nv, h, w;            // flat form: h = 1, w = n elements per view
    int layout;              // METRICS_GT_*
    int tiles_y, tiles_x;    // workgroups per view = tiles_y * tiles_x (flat form: 1 x chunks)
    unsigned* ticket;
    double* partials;        // (NV * tiles_y * tiles_x, METRICS_SUMS)
};

}  // namespace pny
