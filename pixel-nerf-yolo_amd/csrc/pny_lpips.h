// LPIPS v0.1 on VGG-16 (lpips.hip; entry points in lpips_api.hip): the third number of the reference's eval tail
// (eval/calc_metrics.py:186-246), restated from the published definition with net="vgg", normalize=False, spatial=False.
//   input       x in [-1, 1] per channel; a byte is fl32(b / 255), a [0, 1] value t is fl32(fl32(t * 2) - 1)
//   scaling     fl32(fl32(x - shift) / scale), shift = (-.030, -.088, -.188), scale = (.458, .448, .450), IEEE division
//   features    torchvision's VGG-16 `features` 0 .. 29: 13 convolutions 3x3 / stride 1 / pad 1 with bias and relu, a
//               max_pool2d(2, 2) in floor mode in front of convolutions 2, 4, 7 and 10; the taps are the outputs of
//               convolutions 1, 3, 6, 9 and 12 (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3)
//   per tap     f^ = f / (sqrt(sum_c f^2) + 1e-10) per pixel, d = sum_c w[c] (f^0[c] - f^1[c])^2, mean of d over the pixels;
//               in fp64 on the fp32 features
//   value       the sum of the five taps' means
// The convolutions run on conv_mfma_kernel (encoder.hip) with scale 1, shift = bias, relu.  The header also compiles for the
// host alone (its functions are then plain inline ones).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pny {

constexpr int LPIPS_CONVS = 13, LPIPS_TAPS = 5;
constexpr int LPIPS_MIN_SIZE = 16;          // below it relu5_3 (size >> 4) is empty
constexpr int LPIPS_CIN[LPIPS_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LPIPS_COUT[LPIPS_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
// the stage of a convolution: its input has (H >> stage) x (W >> stage) pixels; a stage's first convolution reads the pool
constexpr int LPIPS_STAGE[LPIPS_CONVS] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int LPIPS_TAP_CONV[LPIPS_TAPS] = {1, 3, 6, 9, 12};
constexpr int LPIPS_TAP_CH[LPIPS_TAPS] = {64, 128, 256, 512, 512};
constexpr double LPIPS_EPS = 1e-10;

// pny_lpips_desc::pred_kind / gt_kind (include/pnyolo.h PNY_LPIPS_*)
enum { LPIPS_F32_NHWC_01 = 0, LPIPS_F32_NCHW_PM1 = 1, LPIPS_U8_NHWC = 2, LPIPS_F32_NCHW_01 = 3 };

constexpr int LPIPS_DIST_GROUP = 16;        // lanes that share one pixel: 16 x 16 bytes = 64 channels per step
constexpr int lpips_dist_threads(int c) { return c >= 512 ? 512 : 1024; }   // one workgroup per pair

// The workspace of a batch of n pairs, in floats, each buffer rounded up to 64 floats (encoder.h Carver):
//   img4   2n H W 4     the prepared images, channel-last with a zero 4th channel
//   a, b   2n H W 64    each: the largest activation (relu1_*); the layers alternate between them, and a tap is scored
//                       before the pool overwrites the other buffer
// bytes = 4 (r64(2n H W 4) + 2 r64(2n H W 64)).
constexpr size_t lpips_r64(size_t count) { return (count + 63) & ~(size_t)63; }
constexpr size_t lpips_workspace_floats(size_t n, size_t h, size_t w) {
    return lpips_r64(2 * n * h * w * 4) + 2 * lpips_r64(2 * n * h * w * 64);
}
// the largest activation must be addressable with 32-bit element indices
constexpr bool lpips_fits_32bit(long long n, long long h, long long w) { return 2 * n * h * w * 64 < (1ll << 31); }

// The conv_mfma_kernel instantiation (100 SPLIT + 10 NT + MT) of VGG convolution `layer` whose input has h x w pixels, in a
// pass configured for n_images images.  The K split changes the order of a dot product's sum, so it follows from the layer
// and the image size alone (the tiles ONE pair would give): a pair's bits do not depend on the batch it is scored in.  The
// tile size does not change any sum; it follows the configured batch as run_conv_ex's own choice follows the launch, on the
// MI355X's 256 CUs.
constexpr int LPIPS_CUS = 256;
constexpr int lpips_conv_J(int layer) { return (9 * ((LPIPS_CIN[layer] + 3) / 4 * 4) + 7) / 8; }
constexpr int lpips_conv_variant(int layer, int h, int w, int n_images) {
    const long long cout = LPIPS_COUT[layer], pair = 2ll * h * w, all = (long long)n_images * h * w;
    const bool split = lpips_conv_J(layer) >= 32 && ((pair + 31) / 32) * (cout / 32) <= 4 * LPIPS_CUS;
    const bool small = ((all + 63) / 64) * (cout / 64) < 2 * LPIPS_CUS;
    return split ? (small ? 811 : 822) : (small ? 111 : 122);
}

struct LpipsPrepareArgs {
    const void* pred;        // (n, H, W, 3) fp32 or uint8, or (n, 3, H, W) fp32
    const void* gt;
    float* out;              // (2n, H, W, 4): predictions [0, n), ground truths [n, 2n)
    double* zero;            // (n) values to clear (the batch's results), or null
    int n, h, w;
    int pred_kind, gt_kind;  // LPIPS_*
    int clamp;               // clamp a float prediction to [0, 1] first
};

// One channel of one pixel: the value in [-1, 1] from its stored form, then the scaling layer.
#if defined(__HIPCC__)
#define PNY_LPIPS_FN __host__ __device__ __forceinline__
#else
#define PNY_LPIPS_FN inline
#endif
PNY_LPIPS_FN float lpips_scale_channel(float x, int c) {
    const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
    const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
    return (x - shift) / scale;
}
PNY_LPIPS_FN float lpips_from_01(float t) {
    const float d = t * 2.0f;
    return d - 1.0f;
}
PNY_LPIPS_FN float lpips_from_byte(uint8_t b) { return lpips_from_01((float)b / 255.0f); }

}  // namespace pny
