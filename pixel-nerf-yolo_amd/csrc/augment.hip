// The colour jitter of the training views in ONE launch for all objects and views (data.ColorJitterDataset.apply_color_jitter,
// reference src/data/data_util.py:34-47; arithmetic in pny_augment.h).  The reference runs four passes per view on CPU tensors
// in every __getitem__; here the un-jittered batch is uploaded and jittered where the trainer uses it.
//
// One workgroup owns one image, so the one image-wide quantity -- the mean grey level that the contrast step blends with --
// never leaves the workgroup: no workgroup waits for another, no tickets, no atomics.
//   pass 1   saturation and hue of every pixel, its grey level added to the thread's fp64 partial sum.  A thread visits the
//            quads (4 consecutive pixels) tid, tid + 1024, ... and then at most one of the H*W % 4 trailing pixels: an order
//            that depends on H*W alone, not on where the image lies in memory, so an image gives the same mean in a batch,
//            alone, and at any alignment.  The partials are reduced by a wave shuffle tree and a fixed LDS tree over the 16
//            waves (metrics.hip block_sum); the mean is rounded to fp32.
//   pass 2   after that one __syncthreads(): the input again (L2-resident: 1.4 MB for 300 x 400), saturation and hue recomputed
//            rather than kept, then contrast, brightness, the map back to [-1, 1] and the store.
// out == in is allowed for the float format: every load of an image's pass 1 has been consumed before the barrier, and in
// pass 2 a thread stores only the pixels it has just loaded.
//
// Memory: a quad of a float plane is one 16-byte load / store when the image's base is 16-byte aligned and H*W % 4 == 0 (then
// all three planes of all quads are), four 4-byte ones otherwise; a quad of the byte format is 12 bytes, three 4-byte loads
// when the image's base is 4-byte aligned (images follow each other at H*W*3 bytes: odd strides are not), twelve byte loads
// otherwise.
#include <hip/hip_runtime.h>

#include "pny_augment.h"

namespace pny {
namespace {

constexpr int WAVES = JITTER_THREADS / 64;

__device__ inline double wave_sum(double x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

// The sum over the workgroup's threads in a fixed order, in every thread.  lds: WAVES doubles.
__device__ inline double block_sum(double v, double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double x = wave_sum(v);
    if (lane == 0) lds[wave] = x;
    __syncthreads();
    double s[WAVES];
#pragma unroll
    for (int i = 0; i < WAVES; ++i) s[i] = lds[i];
#pragma unroll
    for (int w = WAVES / 2; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) s[i] += s[i + w];
    return s[0];
}

struct Quad {
    float r[4], g[4], b[4];
};

// one image of either format: pixels as [0, 1] floats
template <int FORMAT>
struct Image;

template <>
struct Image<JITTER_F32_NCHW_PM1> {
    const float* p;
    int hw;
    bool vec;
    __device__ Image(const void* in, size_t img, int hw_) : p((const float*)in + img * 3 * (size_t)hw_), hw(hw_) {
        vec = ((uintptr_t)p & 15) == 0 && (hw & 3) == 0;
    }
    __device__ void pixel(int i, float& r, float& g, float& b) const {
        r = jitter_from_pm1(p[i]), g = jitter_from_pm1(p[(size_t)hw + i]), b = jitter_from_pm1(p[2 * (size_t)hw + i]);
    }
    __device__ void quad(int k, Quad& q) const {
        const float* a = p + 4 * (size_t)k;
        if (vec) {
            const float4 r = *(const float4*)a, g = *(const float4*)(a + hw), b = *(const float4*)(a + 2 * (size_t)hw);
            q.r[0] = r.x, q.r[1] = r.y, q.r[2] = r.z, q.r[3] = r.w;
            q.g[0] = g.x, q.g[1] = g.y, q.g[2] = g.z, q.g[3] = g.w;
            q.b[0] = b.x, q.b[1] = b.y, q.b[2] = b.z, q.b[3] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) q.r[j] = a[j], q.g[j] = a[(size_t)hw + j], q.b[j] = a[2 * (size_t)hw + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            q.r[j] = jitter_from_pm1(q.r[j]), q.g[j] = jitter_from_pm1(q.g[j]), q.b[j] = jitter_from_pm1(q.b[j]);
    }
};

template <>
struct Image<JITTER_U8_NHWC> {
    const uint8_t* p;
    bool vec;
    __device__ Image(const void* in, size_t img, int hw) : p((const uint8_t*)in + img * 3 * (size_t)hw) {
        vec = ((uintptr_t)p & 3) == 0;
    }
    __device__ void pixel(int i, float& r, float& g, float& b) const {
        const uint8_t* a = p + 3 * (size_t)i;
        r = jitter_from_byte(a[0]), g = jitter_from_byte(a[1]), b = jitter_from_byte(a[2]);
    }
    __device__ void quad(int k, Quad& q) const {
        const uint8_t* a = p + 12 * (size_t)k;
        uint8_t c[12];
        if (vec) {
            const uint32_t* w = (const uint32_t*)a;
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                c[j] = (uint8_t)(w0 >> (8 * j)), c[4 + j] = (uint8_t)(w1 >> (8 * j)), c[8 + j] = (uint8_t)(w2 >> (8 * j));
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) c[j] = a[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            q.r[j] = jitter_from_byte(c[3 * j]), q.g[j] = jitter_from_byte(c[3 * j + 1]), q.b[j] = jitter_from_byte(c[3 * j + 2]);
    }
};

template <int FORMAT>
__device__ void jitter_image(const JitterArgs& a, double* red) {
    const int tid = threadIdx.x;
    const int hw = a.hw, quads = hw >> 2, rest = hw & 3;
    const size_t img = blockIdx.x;
    const JitterFactors f = a.f[blockIdx.x / a.n_views];
    const Image<FORMAT> in(a.in, img, hw);

    double sum = 0.0;
    for (int k = tid; k < quads; k += JITTER_THREADS) {
        Quad q;
        in.quad(k, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += (double)jitter_first(q.r[j], q.g[j], q.b[j], f.hue, f.sat);
    }
    if (tid < rest) {
        float r, g, b;
        in.pixel(4 * quads + tid, r, g, b);
        sum += (double)jitter_first(r, g, b, f.hue, f.sat);
    }
    const float mean = jitter_mean(block_sum(sum, red), hw);

    float* out = a.out + img * 3 * (size_t)hw;
    const bool vec_out = ((uintptr_t)out & 15) == 0 && rest == 0;
    for (int k = tid; k < quads; k += JITTER_THREADS) {
        Quad q;
        in.quad(k, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            jitter_first(q.r[j], q.g[j], q.b[j], f.hue, f.sat);
            q.r[j] = jitter_second(q.r[j], mean, f.con, f.bri);
            q.g[j] = jitter_second(q.g[j], mean, f.con, f.bri);
            q.b[j] = jitter_second(q.b[j], mean, f.con, f.bri);
        }
        float* o = out + 4 * (size_t)k;
        if (vec_out) {
            *(float4*)o = make_float4(q.r[0], q.r[1], q.r[2], q.r[3]);
            *(float4*)(o + hw) = make_float4(q.g[0], q.g[1], q.g[2], q.g[3]);
            *(float4*)(o + 2 * (size_t)hw) = make_float4(q.b[0], q.b[1], q.b[2], q.b[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = q.r[j], o[(size_t)hw + j] = q.g[j], o[2 * (size_t)hw + j] = q.b[j];
        }
    }
    if (tid < rest) {
        const int i = 4 * quads + tid;
        float r, g, b;
        in.pixel(i, r, g, b);
        jitter_first(r, g, b, f.hue, f.sat);
        out[i] = jitter_second(r, mean, f.con, f.bri);
        out[(size_t)hw + i] = jitter_second(g, mean, f.con, f.bri);
        out[2 * (size_t)hw + i] = jitter_second(b, mean, f.con, f.bri);
    }
}

__global__ __launch_bounds__(JITTER_THREADS) void color_jitter_kernel(JitterArgs a) {
    __shared__ double red[WAVES];
    if (a.format == JITTER_U8_NHWC) jitter_image<JITTER_U8_NHWC>(a, red);
    else jitter_image<JITTER_F32_NCHW_PM1>(a, red);
}

}  // namespace

void launch_color_jitter(const JitterArgs& a, int n_images, hipStream_t st) {
    hipLaunchKernelGGL(color_jitter_kernel, dim3((unsigned)n_images), dim3(JITTER_THREADS), 0, st, a);
}

}  // namespace pny
