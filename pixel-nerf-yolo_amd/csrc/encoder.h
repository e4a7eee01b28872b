// ResNet-34 trunk of SpatialEncoder (reference src/model/encoder.py:139-173) on gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "dev_resource.h"

namespace pny {

// Geometry of one convolution and where its operands are.  The pointers own nothing: they point into buffers someone else
// holds (EncoderWeights::allocs, pny_model::zproj_allocs, a caller's tensors), and layers are copied freely.
struct ConvLayer {
    float* w = nullptr;      // packed MFMA A-operand order [Cout/32][J][64][4], K = (ky,kx,ci)
    float* scale = nullptr;  // eval-mode batch norm: gamma / sqrt(var + eps)
    float* shift = nullptr;  // beta - mean * scale
    int cin = 0, cin_p = 0, cout = 0, k = 0, stride = 1, pad = 0, J = 0;
};

// ---------------------------------------------------------------------------------- the trunk, described once
// torchvision's ResNet-34 up to layer3 as its convolution + batch-norm units in execution order: the stem, then per BasicBlock
// [downsample,] conv1, conv2.  Inference (encoder.hip) and training (encoder_train.hip) both walk this table:
//   downsample  idt = bn(conv(x))              (else idt = x)
//   conv1       a   = relu(bn(conv(x)))
//   conv2       x   = relu(bn(conv(a)) + idt); the last unit of a level is that level's output
enum class TrunkRole { stem, downsample, conv1, conv2 };
struct TrunkConv {
    std::string conv, bn;   // state-dict names below the trunk's prefix ("layer2.0.conv1", "layer2.0.bn1")
    int cin, cout, k, stride, pad;
    int level;              // pyramid level 1..3, 0 for the stem
    TrunkRole role;
    bool level_end;         // its output is the level's output
};
const std::vector<TrunkConv>& trunk_table();   // built once
ConvLayer conv_geometry(const TrunkConv& c);   // a unit as conv_mfma_kernel runs it: ci padded to fours, K to eights; no operands yet

// pyramid level channels and their offsets in the 512-channel latent
constexpr int TRUNK_CH[4] = {64, 64, 128, 256}, TRUNK_COFF[4] = {0, 64, 128, 256}, TRUNK_LATENT = 512;
struct Pyramid {
    int h[4], w[4];
};
Pyramid pyramid(int height, int width, bool use_first_pool);
int conv_out(int in, int k, int s, int p);
void encoder_latent_size(int height, int width, int* hl, int* wl);

// Packed A operand of a convolution, [rows/32][J][64][4]: element r of lane l in k-iteration j of row tile nt is row
// n = 32 nt + (l & 31), reduction index kk = 8 j + 4 (l >> 5) + r.  These give its source offset in the (cout, cin, k, k)
// weight tensor, or -1 where the operand is zero padding.
//   forward image:    rows = co, K = (ky, kx, ci) with ci padded to cin_p
//   transposed image: rows = ci, K = (ky', kx', co) with FLIPPED taps, W_t[ci][(ky', kx', co)] = W[co][ci][k-1-ky'][k-1-kx']
__host__ __device__ inline long long conv_pack_src(int n, int kk, int cin, int cin_p, int k) {
    const int tap = kk / cin_p, ci = kk - tap * cin_p;
    return tap < k * k && ci < cin ? ((long long)n * cin + ci) * (k * k) + tap : -1;
}
__host__ __device__ inline long long conv_pack_src_t(int n, int kk, int cin, int cout, int k) {
    const int tap = kk / cout, co = kk - tap * cout;
    return tap < k * k ? ((long long)co * cin + n) * (k * k) + (k * k - 1 - tap) : -1;
}

// Lays buffers of floats out in one allocation, each rounded up to 64 floats.  With a null base it only counts: the sizing and
// the carving of a workspace are one pass.
struct Carver {
    float* base = nullptr;
    size_t off = 0;
    float* take(size_t count) {
        float* p = base ? base + off : nullptr;
        off += (count + 63) & ~(size_t)63;
        return p;
    }
};

// Inference weights: one folded conv + bn layer per entry of trunk_table(), in its order
struct EncoderWeights {
    std::vector<ConvLayer> convs;
    std::vector<DevBuf> allocs;   // what the layers point into
    using Getter = std::function<bool(const std::string&, const float**, std::vector<int64_t>*)>;
    bool build(const Getter& get, const std::string& prefix, std::string* err);
};

// Pixel-wise linear map over a channel-last tensor, out[p][n] = sum_k W[n][k] in[p][k], run by the
// same implicit-GEMM kernel as a 1x1 convolution (scale 1, shift 0, no relu).  W is nmat row-major (rows x k) matrices
// stacked along n; rows*nmat must be a multiple of 64, k of 8.  Allocates the layer; the caller fills `w` (pack.hip PACK_NT).
bool build_pixel_linear(int nmat, int rows, int k, ConvLayer* out, std::vector<DevBuf>* allocs, std::string* err);
// f16x2: split-f16 matrix products (pixel_linear_h2_kernel) instead of the fp32 MFMA
// route (optional): the kernel that was launched -- PL_ROUTE_TILED_F32 / PL_ROUTE_TILED_H2 for the tiled GEMM, else the
// 1x1-convolution path's conv_mfma_kernel instantiation as run_conv_ex reports it (100 SPLIT + 10 NT + MT, >= 111).
constexpr int PL_ROUTE_TILED_F32 = 1, PL_ROUTE_TILED_H2 = 2;
bool run_pixel_linear(const ConvLayer& L, const float* in, long long npix, float* out, hipStream_t st, bool f16x2 = false,
                      int* route = nullptr);

// One convolution through conv_mfma_kernel (encoder.hip): out = relu?(conv(in) * L.scale + L.shift + resid), channel-last.
// hout / wout explicit; dil_shift > 0 reads the input as if 2^dil_shift - 1 zeros stood between its samples.
// variant (optional): the conv_mfma_kernel<SPLIT, NT, MT> instantiation that was launched, as 100 SPLIT + 10 NT + MT.
// force_variant (optional): launch that instantiation (811, 822, 111 or 122) instead of choosing one from the launch's tile
// count; 0 keeps the choice.  811 and 822 need L.J >= 32, as the unforced choice does; anything else fails.  For callers whose bits must not depend on how many images share the launch (pny_lpips.h).
bool run_conv_ex(const ConvLayer& L, const float* in, int n, int hin, int win, int hout, int wout, int dil_shift, const float* resid,
                 int relu, float* out, hipStream_t st, int* variant = nullptr, int force_variant = 0);
// The trunk's other forward kernels (encoder.hip), shared by inference and training:
// images (n,3,H,W) NCHW -> (n,H,W,4) channel-last with a zero 4th channel
void launch_image_to_nhwc4(const float* images, float* out, int n, int height, int width, hipStream_t st);
// max_pool2d(3, stride 2, pad 1) in front of layer1: level 0 of the pyramid -> level 1's size
void launch_first_pool(const float* l0, float* out, int n, const Pyramid& d, hipStream_t st);
// ... which is this on level 0: max_pool2d(3, stride 2, pad 1) of a channel-last (n, hin, win, c) tensor
void launch_maxpool(const float* in, float* out, int n, int hin, int win, int c, hipStream_t st);
// every pyramid level resampled (bilinear, align_corners=True) to level 0's size into the channel-last latent
void launch_pyramid_to_latent(const float* const level_out[4], float* latent_nhwc, int n, const Pyramid& d, hipStream_t st);
// ... one level of it: (n, hin, win, TRUNK_CH[lv]) -> channels [TRUNK_COFF[lv], + TRUNK_CH[lv]) of the (n, h0, w0, 512) latent
void launch_upsample_level(const float* in, float* latent_nhwc, int n, int hin, int win, int lv, int h0, int w0, hipStream_t st);

size_t encoder_workspace_bytes(int ns, int height, int width, bool use_first_pool);
// images (ns,3,H,W) NCHW -> latent (ns, H0, W0, 512) channel-last
bool encoder_forward(const EncoderWeights& w, const float* images, int ns, int height, int width, bool use_first_pool,
                     float* work, float* latent_nhwc, hipStream_t st, std::string* err);

}  // namespace pny
