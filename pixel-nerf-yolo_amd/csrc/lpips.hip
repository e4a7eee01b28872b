// LPIPS (VGG-16) kernels for gfx950 that the trunk does not already have (pny_lpips.h states the definition; the 13
// convolutions are conv_mfma_kernel in encoder.hip): the input preparation, the 2x2 max pool, the distance of one tap, and the
// packing of a convolution's weights into the MFMA A-operand order.
#include "encoder.h"
#include "pny_common.h"
#include "pny_lpips.h"
#include "pny_metrics.h"

namespace pny {

// One thread per pixel of the 2n images: reads the pixel in its stored form, writes float4 {r, g, b, 0} after the scaling layer.
// The first n threads also clear the batch's results, which the five distance launches then add to in stream order.
__global__ __launch_bounds__(256) void lpips_prepare_kernel(const LpipsPrepareArgs a) {
    const long long hw = (long long)a.h * a.w;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.zero && i < a.n) a.zero[i] = 0.0;
    if (i >= 2 * a.n * hw) return;
    const int img = (int)(i / hw);
    const long long p = i - (long long)img * hw;
    const bool is_gt = img >= a.n;
    const int kind = is_gt ? a.gt_kind : a.pred_kind;
    const long long v = is_gt ? img - a.n : img;           // view within its own tensor
    const void* base = is_gt ? a.gt : a.pred;
    float x[3];
    if (kind == LPIPS_U8_NHWC) {
        const uint8_t* s = static_cast<const uint8_t*>(base) + (v * hw + p) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = lpips_from_byte(s[c]);
    } else {
        const float* s = static_cast<const float*>(base);
        const bool nchw = kind == LPIPS_F32_NCHW_PM1 || kind == LPIPS_F32_NCHW_01;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = nchw ? s[(v * 3 + c) * hw + p] : s[(v * hw + p) * 3 + c];
            if (kind != LPIPS_F32_NCHW_PM1) {
                if (a.clamp && !is_gt) t = metrics_clamp01(t);
                t = lpips_from_01(t);
            }
            x[c] = t;
        }
    }
    *reinterpret_cast<float4*>(a.out + i * 4) =
        make_float4(lpips_scale_channel(x[0], 0), lpips_scale_channel(x[1], 1), lpips_scale_channel(x[2], 2), 0.f);
}

// max_pool2d(2, 2), floor mode, channel-last: one thread per output pixel and channel quad.  fmaxf drops a NaN where
// torch.max_pool2d propagates it; its input here is a relu's output, which holds none unless the convolution produced one.
__global__ __launch_bounds__(256) void maxpool2_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int hin, int win, int c,
                                                       int hout, int wout) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int cq = c / 4;
    if (i >= (long long)n * hout * wout * cq) return;
    const int q = (int)(i % cq);
    long long p = i / cq;
    const int ox = (int)(p % wout);
    p /= wout;
    const int oy = (int)(p % hout), img = (int)(p / hout);
    const float* b = in + (((size_t)img * hin + 2 * oy) * win + 2 * ox) * c + 4 * q;
    const float4 v00 = *reinterpret_cast<const float4*>(b);
    const float4 v01 = *reinterpret_cast<const float4*>(b + c);
    const float4 v10 = *reinterpret_cast<const float4*>(b + (size_t)win * c);
    const float4 v11 = *reinterpret_cast<const float4*>(b + (size_t)win * c + c);
    float4 m;
    m.x = fmaxf(fmaxf(v00.x, v01.x), fmaxf(v10.x, v11.x));
    m.y = fmaxf(fmaxf(v00.y, v01.y), fmaxf(v10.y, v11.y));
    m.z = fmaxf(fmaxf(v00.z, v01.z), fmaxf(v10.z, v11.z));
    m.w = fmaxf(fmaxf(v00.w, v01.w), fmaxf(v10.w, v11.w));
    *reinterpret_cast<float4*>(out + i * 4) = m;
}

// sum over the 16 lanes that share a pixel; every lane ends with the same bits (each step adds the same two numbers in both
// partners)
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = LPIPS_DIST_GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LPIPS_DIST_GROUP);
    return v;
}

__device__ __forceinline__ double sum_sq(const float4 v) {   // products of two floats are exact in fp64
    return (double)v.x * (double)v.x + (double)v.y * (double)v.y + (double)v.z * (double)v.z + (double)v.w * (double)v.w;
}

// The distance of one tap: workgroup `pair` owns images pair and n + pair of the (2n, npix, C) tap tensor.  A group of 16
// lanes takes one pixel at a time, pixels group, group + groups, ...: each lane holds KC float4 of both images' features (lane l
// of step k: channels 64 k + 4 l ..), the two norms are summed over the lane's own values and then over the group, and so is
// the weighted squared difference of the unit features.  All of it is fp64 on the fp32 features: the kernel is bound by
// the one CU's memory traffic, not by its arithmetic, and the value then carries the convolutions' rounding alone.  The
// unit feature is f * (1 / (sqrt(sum) + 1e-10)), one division per pixel and image.  The group's pixels are summed in order;
// thread 0 adds the groups' sums in order, divides by the pixel count and writes or adds.
// 1024 threads (64 groups) up to 256 channels, 512 threads at 512 channels (64 operand registers per lane and image).
template <int KC>
__global__ __launch_bounds__(lpips_dist_threads(64 * KC)) void lpips_distance_kernel(const float* __restrict__ feat, const float* __restrict__ wl,
                                                                            double* __restrict__ out, int n, int npix, int accumulate) {
    constexpr int C = 64 * KC, GROUPS = lpips_dist_threads(C) / LPIPS_DIST_GROUP;
    __shared__ double part[GROUPS];
    const int pair = blockIdx.x;
    const int group = threadIdx.x / LPIPS_DIST_GROUP, l = threadIdx.x % LPIPS_DIST_GROUP;
    const float* f0 = feat + (size_t)pair * npix * C + 4 * l;
    const float* f1 = feat + (size_t)(n + pair) * npix * C + 4 * l;
    double acc = 0.0;
    for (int p = group; p < npix; p += GROUPS) {
        float4 a[KC], b[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            a[k] = *reinterpret_cast<const float4*>(f0 + (size_t)p * C + 64 * k);
            b[k] = *reinterpret_cast<const float4*>(f1 + (size_t)p * C + 64 * k);
        }
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            sa += sum_sq(a[k]);
            sb += sum_sq(b[k]);
        }
        const double ia = 1.0 / (sqrt(group_sum(sa)) + LPIPS_EPS), ib = 1.0 / (sqrt(group_sum(sb)) + LPIPS_EPS);
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const float4 w = *reinterpret_cast<const float4*>(wl + 64 * k + 4 * l);
            const double dx = a[k].x * ia - b[k].x * ib, dy = a[k].y * ia - b[k].y * ib;
            const double dz = a[k].z * ia - b[k].z * ib, dw = a[k].w * ia - b[k].w * ib;
            d += w.x * (dx * dx) + w.y * (dy * dy) + w.z * (dz * dz) + w.w * (dw * dw);
        }
        acc += group_sum(d);
    }
    if (l == 0) part[group] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int g = 0; g < GROUPS; ++g) s += part[g];
        const double mean = s / (double)npix;
        out[pair] = accumulate ? out[pair] + mean : mean;
    }
}

// (cout, cin, 3, 3) -> the A operand of conv_mfma_kernel, [cout/32][J][64][4] (encoder.h conv_pack_src)
__global__ __launch_bounds__(256) void lpips_pack_conv_kernel(const float* __restrict__ w, float* __restrict__ packed, int cin, int cin_p,
                                                              int cout, int J) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (long long)(cout / 32) * J * 256) return;
    const int r = (int)(o & 3), l = (int)((o >> 2) & 63);
    const long long t = o >> 8;
    const int j = (int)(t % J), nt = (int)(t / J);
    const long long src = conv_pack_src(32 * nt + (l & 31), 8 * j + 4 * (l >> 5) + r, cin, cin_p, 3);
    packed[o] = src >= 0 ? w[src] : 0.f;
}

// ----------------------------------------------------------------------------------- launchers (lpips_api.hip)
void launch_lpips_prepare(const LpipsPrepareArgs& a, hipStream_t st) {
    const long long npx = 2ll * a.n * a.h * a.w;
    hipLaunchKernelGGL(lpips_prepare_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, st, a);
}

void launch_maxpool2(const float* in, float* out, int n, int hin, int win, int c, hipStream_t st) {
    const int hout = hin / 2, wout = win / 2;
    const long long np = (long long)n * hout * wout * (c / 4);
    hipLaunchKernelGGL(maxpool2_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, in, out, n, hin, win, c, hout, wout);
}

bool launch_lpips_distance(const float* feat, const float* wl, double* out, int n, int npix, int c, int accumulate, hipStream_t st) {
    const dim3 grid((unsigned)n), block(lpips_dist_threads(c));
    switch (c) {
        case 64: hipLaunchKernelGGL(lpips_distance_kernel<1>, grid, block, 0, st, feat, wl, out, n, npix, accumulate); break;
        case 128: hipLaunchKernelGGL(lpips_distance_kernel<2>, grid, block, 0, st, feat, wl, out, n, npix, accumulate); break;
        case 256: hipLaunchKernelGGL(lpips_distance_kernel<4>, grid, block, 0, st, feat, wl, out, n, npix, accumulate); break;
        case 512: hipLaunchKernelGGL(lpips_distance_kernel<8>, grid, block, 0, st, feat, wl, out, n, npix, accumulate); break;
        default: return false;
    }
    return true;
}

void launch_lpips_pack_conv(const float* w, float* packed, int cin, int cin_p, int cout, int J, hipStream_t st) {
    const long long total = (long long)(cout / 32) * J * 256;
    hipLaunchKernelGGL(lpips_pack_conv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, packed, cin, cin_p, cout, J);
}

}  // namespace pny
