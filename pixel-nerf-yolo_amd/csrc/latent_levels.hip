// The latent of a backbone that returns a LIST of feature maps (reference src/model/encoder.py:126-137, backbone = "custom":
// every map resized to the first map's size, bilinear with align_corners = True, and concatenated along the channels), and its
// adjoint.  Maps are fp32 NCHW as the backbone leaves them, the latent is channel-last (n, h0, w0, sum C_i) as every kernel of
// the library reads it: one launch assembles all levels, one launch takes d loss / d latent back to all levels.
//
//   latent_levels_kernel      a workgroup owns 32 latent pixels x 32 channels of one level.  It resamples along the pixels
//                             (lanes run along a map's row, so a wave reads contiguous runs of the NCHW plane), parks the
//                             values in a 32 x 33 LDS tile and writes them out along the channels (128-byte runs of the
//                             channel-last latent), as transpose_kernel (render_kernels.hip) does for a plain repack.
//   latent_levels_bwd_kernel  the adjoint as a gather (upsample_bwd_kernel's form, encoder_train.hip): a workgroup owns 32 map
//                             pixels x 32 channels; every map pixel collects w_y w_x d_latent[oy][ox] from the latent pixels
//                             whose footprint holds it, with the weights the forward computes, reading along the channels;
//                             the tile is written out along the pixels of the NCHW gradient.  No atomics, a fixed order of
//                             summation: the same bits on every run.
//
// A level whose channel count and channel offset are multiples of 4 (and the latent's total too, in a 16-byte aligned buffer)
// moves its channel-last side as float4; any other level takes the scalar path of the same kernels.
//
// Resampling is ATen's upsample_bilinear2d(align_corners = True) in float32: scale = (h_i - 1) / (h_0 - 1) (0 when h_0 == 1),
// src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < h_i - 1), l1 = src - i0, l0 = 1 - l1,
// l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11).  A level of the latent's own size is therefore copied bit for bit.
#include <stdint.h>

#include <string>

#include "api_internal.h"

namespace pny {

struct LevelsArgs {
    const float* map[PNY_MAX_LATENT_LEVELS];     // forward: the maps; backward: unused
    float* d_map[PNY_MAX_LATENT_LEVELS];         // backward: the maps' gradients (NULL: level skipped, it owns no tiles)
    int c[PNY_MAX_LATENT_LEVELS], h[PNY_MAX_LATENT_LEVELS], w[PNY_MAX_LATENT_LEVELS];
    int coff[PNY_MAX_LATENT_LEVELS];             // first channel of the level in the latent
    int vec[PNY_MAX_LATENT_LEVELS];              // the level's channel-last side moves as float4
    unsigned tile0[PNY_MAX_LATENT_LEVELS + 1];   // first workgroup of the level; [n_levels] = the grid
    int n_levels, n, L;
};

constexpr int LV_TILE = 32;

struct Tap {
    int i0, i1;
    float l0, l1;
};

// source taps of output index o (ATen area_pixel_compute_source_index + guard, align_corners = True)
__device__ __forceinline__ Tap level_tap(float scale, int o, int size_in) {
    Tap t;
    const float f = scale * (float)o;
    t.i0 = (int)f;
    t.i0 = t.i0 < size_in - 1 ? t.i0 : size_in - 1;      // (never taken while scale * o rounds below size_in; keeps every tap inside)
    t.i1 = t.i0 + (t.i0 < size_in - 1 ? 1 : 0);
    t.l1 = f - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

__device__ __forceinline__ float level_scale(int size_in, int size_out) {
    return size_out > 1 ? (float)(size_in - 1) / (float)(size_out - 1) : 0.f;
}

// the level that owns workgroup b (tile0 ascends; levels without tiles have tile0[l] == tile0[l + 1])
__device__ __forceinline__ int level_of(const LevelsArgs& a, unsigned b) {
    int lv = 0;
    while (lv + 1 < a.n_levels && b >= a.tile0[lv + 1]) ++lv;
    return lv;
}

__global__ __launch_bounds__(256) void latent_levels_kernel(const LevelsArgs a, float* __restrict__ lat) {
    __shared__ float tile[LV_TILE][LV_TILE + 1];          // [channel][pixel]
    const int lv = level_of(a, blockIdx.x);
    const int C = a.c[lv], hi = a.h[lv], wi = a.w[lv], h0 = a.h[0], w0 = a.w[0];
    const int hw0 = h0 * w0;
    const unsigned ptiles = (unsigned)((hw0 + LV_TILE - 1) / LV_TILE), ctiles = (unsigned)((C + LV_TILE - 1) / LV_TILE);
    unsigned t = blockIdx.x - a.tile0[lv];
    const int c0 = (int)(t % ctiles) * LV_TILE;
    t /= ctiles;
    const int p0 = (int)(t % ptiles) * LV_TILE, img = (int)(t / ptiles);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    // resample: lane tx owns latent pixel p0 + tx, the 8 lane rows walk the tile's channels
    const int p = p0 + tx;
    if (p < hw0) {
        const int oy = p / w0, ox = p - oy * w0;
        const Tap ty_ = level_tap(level_scale(hi, h0), oy, hi), tx_ = level_tap(level_scale(wi, w0), ox, wi);
        const size_t o00 = (size_t)ty_.i0 * wi + tx_.i0, o01 = (size_t)ty_.i0 * wi + tx_.i1;
        const size_t o10 = (size_t)ty_.i1 * wi + tx_.i0, o11 = (size_t)ty_.i1 * wi + tx_.i1;
        const float* src = a.map[lv] + (size_t)img * C * hi * wi;
        for (int i = ty; i < LV_TILE; i += 8) {
            const int c = c0 + i;
            if (c >= C) break;
            const float* pl = src + (size_t)c * hi * wi;
            tile[i][tx] = ty_.l0 * (tx_.l0 * pl[o00] + tx_.l1 * pl[o01]) + ty_.l1 * (tx_.l0 * pl[o10] + tx_.l1 * pl[o11]);
        }
    }
    __syncthreads();
    float* dst = lat + (size_t)img * hw0 * a.L + a.coff[lv];
    if (a.vec[lv]) {       // 8 lanes x float4 = the tile's 32 channels of one pixel; C % 4 == 0: a quad is whole or absent
        const int q = threadIdx.x & 7, pp = threadIdx.x >> 3;
        const int c = c0 + 4 * q;
        if (p0 + pp < hw0 && c < C)
            *reinterpret_cast<float4*>(dst + (size_t)(p0 + pp) * a.L + c) =
                make_float4(tile[4 * q][pp], tile[4 * q + 1][pp], tile[4 * q + 2][pp], tile[4 * q + 3][pp]);
    } else {
        for (int i = ty; i < LV_TILE; i += 8)
            if (p0 + i < hw0 && c0 + tx < C) dst[(size_t)(p0 + i) * a.L + c0 + tx] = tile[tx][i];
    }
}

// candidate latent indices of map index i: those o with scale * o in (i - 1, i + 1), one more on each side against the
// rounding of the quotient (the weights below are exact zeros outside the footprint)
__device__ __forceinline__ void level_candidates(float scale, int i, int size_out, int& lo, int& hi) {
    lo = 0, hi = size_out - 1;
    if (scale > 0.f) {
        const int l = (int)fmaxf(floorf((float)(i - 1) / scale), 0.f) - 1;               // (clamped as floats: the quotients can pass 2^31)
        const int h = (int)fminf(ceilf((float)(i + 1) / scale), (float)(size_out - 1)) + 1;
        lo = l > 0 ? l : 0;
        hi = h < size_out - 1 ? h : size_out - 1;
    }
}

// weight of map index i in latent index o (both taps when they coincide at the border)
__device__ __forceinline__ float level_weight(float scale, int o, int size_in, int i) {
    const Tap t = level_tap(scale, o, size_in);
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

template <int V>     // V channels per lane on the channel-last side: 4 (float4) or 1
__device__ __forceinline__ void level_gather(const LevelsArgs& a, int lv, const float* __restrict__ g, int y, int x, float (&acc)[4]) {
    const int hi = a.h[lv], wi = a.w[lv], h0 = a.h[0], w0 = a.w[0];
    const float sy = level_scale(hi, h0), sx = level_scale(wi, w0);
    int oy_lo, oy_hi, ox_lo, ox_hi;
    level_candidates(sy, y, h0, oy_lo, oy_hi);
    level_candidates(sx, x, w0, ox_lo, ox_hi);
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        const float wy = level_weight(sy, oy, hi, y);
        if (wy == 0.f) continue;
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const float wx = level_weight(sx, ox, wi, x);
            if (wx == 0.f) continue;
            const float wgt = wy * wx;
            const float* q = g + ((size_t)oy * w0 + ox) * a.L;
            if (V == 4) {
                const float4 v = *reinterpret_cast<const float4*>(q);
                acc[0] += wgt * v.x, acc[1] += wgt * v.y, acc[2] += wgt * v.z, acc[3] += wgt * v.w;
            } else {
                acc[0] += wgt * q[0];
            }
        }
    }
}

__global__ __launch_bounds__(256) void latent_levels_bwd_kernel(const LevelsArgs a, const float* __restrict__ d_lat) {
    __shared__ float tile[LV_TILE][LV_TILE + 1];          // [pixel][channel]
    const int lv = level_of(a, blockIdx.x);
    const int C = a.c[lv], hi = a.h[lv], wi = a.w[lv];
    const int hwi = hi * wi;
    const unsigned ptiles = (unsigned)((hwi + LV_TILE - 1) / LV_TILE), ctiles = (unsigned)((C + LV_TILE - 1) / LV_TILE);
    unsigned t = blockIdx.x - a.tile0[lv];
    const int c0 = (int)(t % ctiles) * LV_TILE;
    t /= ctiles;
    const int p0 = (int)(t % ptiles) * LV_TILE, img = (int)(t / ptiles);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* g = d_lat + (size_t)img * a.h[0] * a.w[0] * a.L + a.coff[lv];
    if (a.vec[lv]) {       // lane = (map pixel, channel quad)
        const int q = threadIdx.x & 7, pp = threadIdx.x >> 3;
        const int p = p0 + pp, c = c0 + 4 * q;
        if (p < hwi && c < C) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const int y = p / wi;
            level_gather<4>(a, lv, g + c, y, p - y * wi, acc);
            for (int j = 0; j < 4; ++j) tile[pp][4 * q + j] = acc[j];
        }
    } else {               // lane tx = channel, the 8 lane rows walk the tile's map pixels
        for (int i = ty; i < LV_TILE; i += 8) {
            const int p = p0 + i, c = c0 + tx;
            if (p < hwi && c < C) {
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                const int y = p / wi;
                level_gather<1>(a, lv, g + c, y, p - y * wi, acc);
                tile[i][tx] = acc[0];
            }
        }
    }
    __syncthreads();
    float* dst = a.d_map[lv] + (size_t)img * C * hwi;
    for (int i = ty; i < LV_TILE; i += 8)          // lane tx = map pixel: runs along the NCHW plane
        if (c0 + i < C && p0 + tx < hwi) dst[(size_t)(c0 + i) * hwi + p0 + tx] = tile[tx][i];
}

// ------------------------------------------------------------------------------------------------ host side
// The shape checks every entry shares; fills everything of LevelsArgs but the pointers and the tiling.
static int latent_levels_shape(const char* who, const int* channels, const int* h, const int* w, int n_levels, int n, LevelsArgs* a) {
    const std::string me = std::string(who) + ": ";
    if (!channels || !h || !w) return fail(PNY_ERR_ARG, me + "null argument");
    if (n_levels < 1 || n_levels > PNY_MAX_LATENT_LEVELS) return fail(PNY_ERR_ARG, me + "n_levels must be 1 .. 8");
    if (n < 1) return fail(PNY_ERR_ARG, me + "n must be at least 1");
    long long L = 0;
    for (int i = 0; i < n_levels; ++i) {
        if (channels[i] < 1 || h[i] < 1 || w[i] < 1) return fail(PNY_ERR_ARG, me + "every level needs a size and a channel count of at least 1");
        if ((long long)h[i] * w[i] >= (1ll << 31)) return fail(PNY_ERR_ARG, me + "a level of 2^31 pixels or more");
        a->c[i] = channels[i], a->h[i] = h[i], a->w[i] = w[i], a->coff[i] = (int)L;
        L += channels[i];
        if (L >= (1ll << 31)) return fail(PNY_ERR_ARG, me + "2^31 channels or more");
    }
    for (int i = 0; i < n_levels; ++i) a->vec[i] = (a->c[i] % 4 == 0 && a->coff[i] % 4 == 0 && L % 4 == 0) ? 1 : 0;
    a->n_levels = n_levels, a->n = n, a->L = (int)L;
    return 0;
}

// tiles of 32 pixels x 32 channels per level: of the latent (forward) or of the level's own plane (backward, levels with a
// destination only)
static int latent_levels_tiling(const char* who, LevelsArgs* a, bool backward) {
    unsigned long long total = 0;
    for (int i = 0; i < a->n_levels; ++i) {
        a->tile0[i] = (unsigned)total;
        if (backward && !a->d_map[i]) continue;
        const long long px = backward ? (long long)a->h[i] * a->w[i] : (long long)a->h[0] * a->w[0];
        total += (unsigned long long)a->n * ((px + LV_TILE - 1) / LV_TILE) * ((a->c[i] + LV_TILE - 1) / LV_TILE);
        if (total >= (1ull << 31)) return fail(PNY_ERR_ARG, std::string(who) + ": too large (2^31 tiles of 32 x 32 or more)");
    }
    a->tile0[a->n_levels] = (unsigned)total;
    return 0;
}

static int launch_latent_levels(const char* who, LevelsArgs& a, const float* const* maps, float* latent, hipStream_t st) {
    for (int i = 0; i < a.n_levels; ++i) a.map[i] = maps[i], a.d_map[i] = nullptr;
    if (reinterpret_cast<uintptr_t>(latent) % 16)
        for (int i = 0; i < a.n_levels; ++i) a.vec[i] = 0;
    if (int rc = latent_levels_tiling(who, &a, false)) return rc;
    hipLaunchKernelGGL(latent_levels_kernel, dim3(a.tile0[a.n_levels]), dim3(256), 0, st, a, latent);
    PNY_HIP(hipGetLastError());
    return 0;
}

int latent_levels_check(const char* who, const float* const* maps, const int* channels, const int* h, const int* w, int n_levels, int n,
                        long long* total_channels) {
    if (!maps) return fail(PNY_ERR_ARG, std::string(who) + ": null argument");
    LevelsArgs a;
    if (int rc = latent_levels_shape(who, channels, h, w, n_levels, n, &a)) return rc;
    for (int i = 0; i < n_levels; ++i)
        if (!maps[i]) return fail(PNY_ERR_ARG, std::string(who) + ": null map");
    if (total_channels) *total_channels = a.L;
    return 0;
}

int latent_levels_assemble(const char* who, const float* const* maps, const int* channels, const int* h, const int* w, int n_levels, int n,
                           float* latent_nhwc, hipStream_t st) {
    if (!latent_nhwc) return fail(PNY_ERR_ARG, std::string(who) + ": null argument");
    if (int rc = latent_levels_check(who, maps, channels, h, w, n_levels, n, nullptr)) return rc;
    LevelsArgs a;
    if (int rc = latent_levels_shape(who, channels, h, w, n_levels, n, &a)) return rc;
    return launch_latent_levels(who, a, maps, latent_nhwc, st);
}

}  // namespace pny

using namespace pny;

extern "C" {

int pny_latent_levels(const float* const* maps_dev, const int* channels, const int* h, const int* w, int n_levels, int n,
                      float* latent_nhwc_dev, pny_stream stream) {
    return latent_levels_assemble("pny_latent_levels", maps_dev, channels, h, w, n_levels, n, latent_nhwc_dev, (hipStream_t)stream);
}

int pny_latent_levels_backward(const float* d_latent_nhwc_dev, float* const* d_maps_dev, const int* channels, const int* h, const int* w,
                               int n_levels, int n, pny_stream stream) {
    const char* who = "pny_latent_levels_backward";
    if (!d_latent_nhwc_dev || !d_maps_dev) return fail(PNY_ERR_ARG, std::string(who) + ": null argument");
    LevelsArgs a;
    if (int rc = latent_levels_shape(who, channels, h, w, n_levels, n, &a)) return rc;
    for (int i = 0; i < n_levels; ++i) {
        a.map[i] = nullptr, a.d_map[i] = d_maps_dev[i];
        if (reinterpret_cast<uintptr_t>(d_latent_nhwc_dev) % 16) a.vec[i] = 0;
    }
    if (int rc = latent_levels_tiling(who, &a, true)) return rc;
    if (a.tile0[n_levels] == 0) return PNY_OK;      // every level skipped
    hipLaunchKernelGGL(latent_levels_bwd_kernel, dim3(a.tile0[n_levels]), dim3(256), 0, (hipStream_t)stream, a, d_latent_nhwc_dev);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
