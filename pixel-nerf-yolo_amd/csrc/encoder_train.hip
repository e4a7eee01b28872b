// ResNet-34 trunk of SpatialEncoder in TRAINING mode, forward and backward, as HIP kernels (gfx950).
//
// The reference trains the encoder by default (train/train.py:66-73 freezes it only with --freeze_enc;
// loss.backward() at train/trainlib/PixelNerfTrainer.py:156 differentiates src/model/encoder.py:139-173 through torchvision's
// BasicBlocks): convolutions, batch norm on BATCH statistics (the trunk is in train() mode), relu, residual adds, the 3x3/2
// max-pool and the bilinear pyramid.  Until round 3 that graph ran through ATen / MIOpen (11 ms of a
// 23.7 ms step, naive_conv_* kernels); here every piece is this library's:
//   forward  per convolution: conv_mfma_kernel (encoder.hip, the inference kernel with scale 1 / shift 0) on weights repacked
//            from the live parameters by ONE launch per step (trunk_pack_kernel), bn_stats_kernel (per-channel shifted sums over
//            fixed pixel ranges, deterministic), bn_apply_kernel (finalises the statistics in every workgroup in the same order,
//            normalises, adds the residual, relu; workgroup 0 also updates running_mean / running_var as nn.BatchNorm2d does);
//   backward per convolution: bn_bwd_stats_kernel (sum g, sum g x^ over the same pixel ranges, g = upstream gradient through the
//            relu mask), bn_bwd_apply_kernel (dy of the convolution output, d gamma, d beta), conv_dw_kernel (weight gradient:
//            a split-K GEMM over PIXELS on the fp32 MFMA, dW[co][(tap, ci)] = sum_p dy[p][co] patch[p][(tap, ci)], partials
//            reduced in a fixed order straight into the (cout, cin, k, k) gradient tensor), and the input gradient as a
//            transposed convolution through conv_mfma_kernel again (flipped, transposed filters from the same repack launch;
//            a stride-2 convolution's gradient is read as a dilated input);
//   maxpool_bwd_kernel and upsample_bwd_kernel are gathers (every input position collects from the windows / output pixels it
//            fed), so nothing in this file uses atomics: the trunk's gradients are bit-reproducible.
// All GEMMs are exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).  Activations channel-last, as in encoder.hip.
// Parity: tests/test_gpu_backward.py::test_encoder_training_gradients_vs_oracle_autograd (87 tensors against torch.autograd
// through the oracle's trunk, <= 1e-4 of each tensor's max).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"

namespace pny {

typedef float f32x16t __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------ weight repack
// kind 0: the forward A-operand image, kind 1: the transposed convolution's (rows = cin of the convolution, J = k k cout / 8);
// both layouts: encoder.h conv_pack_src / conv_pack_src_t
struct TrunkPackJob {
    const float* src;   // (cout, cin, k, k) as PyTorch keeps it
    float* dst;
    int kind, cout, cin, cin_p, k, J, count;   // count = 16-byte elements
};

__global__ __launch_bounds__(256) void trunk_pack_kernel(const TrunkPackJob* __restrict__ jobs) {
    const TrunkPackJob jb = jobs[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < jb.count; i += gridDim.x * blockDim.x) {
        const int l = i & 63, j = (i >> 6) % jb.J, nt = (i >> 6) / jb.J;
        const int n = 32 * nt + (l & 31), k0 = 8 * j + 4 * (l >> 5);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long src = jb.kind == 0 ? conv_pack_src(n, k0 + r, jb.cin, jb.cin_p, jb.k) : conv_pack_src_t(n, k0 + r, jb.cin, jb.cout, jb.k);
            v[r] = src >= 0 ? jb.src[src] : 0.f;
        }
        reinterpret_cast<float4*>(jb.dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ------------------------------------------------------------------------------------------------ batch norm, forward
// Per-channel statistics over P = N H W pixels of a channel-last (P, C) tensor.  A workgroup reduces the pixel range
// [b chunk, (b + 1) chunk); thread t owns channel quad t % (C / 4) and pixel lane t / (C / 4).  Sums are SHIFTED by the
// channel's value at pixel 0 (s1 = sum (y - K), s2 = sum (y - K)^2: var = s2 / P - (s1 / P)^2 without the cancellation of the
// plain sum of squares).  part[b][0 | 1][C].
constexpr int BN_THREADS = 256, BN_MAXB = 64;
constexpr size_t BN_PART_FLOATS = (size_t)BN_MAXB * 2 * 256;   // the partial-sum scratch of a batch-norm launch pair, C <= 256

__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const float* __restrict__ y, long long P, int C, long long chunk,
                                                              float* __restrict__ part) {
    __shared__ float4 red[2][BN_THREADS];
    const int cq = C / 4, rows = BN_THREADS / cq;
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    const float4 K = *reinterpret_cast<const float4*>(y + 4 * q);
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    // four pixels per trip: the loads are independent, the sums stay in pixel order (the result does not depend on the unroll)
    for (long long p = p0 + r; p < p1; p += 4 * rows) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long pp = p + (long long)u * rows;
            v[u] = pp < p1 ? *reinterpret_cast<const float4*>(y + (size_t)pp * C + 4 * q) : K;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float dx = v[u].x - K.x, dy = v[u].y - K.y, dz = v[u].z - K.z, dw = v[u].w - K.w;
            s1.x += dx; s1.y += dy; s1.z += dz; s1.w += dw;
            s2.x += dx * dx; s2.y += dy * dy; s2.z += dz * dz; s2.w += dw * dw;
        }
    }
    red[0][threadIdx.x] = s1;
    red[1][threadIdx.x] = s2;
    __syncthreads();
    if (r == 0) {
        for (int i = 1; i < rows; ++i) {   // fixed order
            const float4 a = red[0][i * cq + q], b = red[1][i * cq + q];
            s1.x += a.x; s1.y += a.y; s1.z += a.z; s1.w += a.w;
            s2.x += b.x; s2.y += b.y; s2.z += b.z; s2.w += b.w;
        }
        *reinterpret_cast<float4*>(part + ((size_t)blockIdx.x * 2 + 0) * C + 4 * q) = s1;
        *reinterpret_cast<float4*>(part + ((size_t)blockIdx.x * 2 + 1) * C + 4 * q) = s2;
    }
}

// out = relu?((y - mean) invstd gamma + beta + resid).  Every workgroup finalises the statistics itself from the B partials
// (same order everywhere); workgroup 0 stores mean / invstd for the backward and steps the running statistics
// (nn.BatchNorm2d, momentum 0.1, unbiased variance).
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ part, int B,
                                                              long long P, int C, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ resid,
                                                              int relu, float* __restrict__ out, float* __restrict__ mean_out,
                                                              float* __restrict__ invstd_out, float* run_mean, float* run_var,
                                                              float momentum, float eps, int use_running) {
    __shared__ float s_mean[256], s_scale[256], s_shift[256];
    for (int c = threadIdx.x; c < C; c += BN_THREADS) {
        float s1 = 0.f, s2 = 0.f;
        for (int b = 0; b < B; ++b) {
            s1 += part[((size_t)b * 2 + 0) * C + c];
            s2 += part[((size_t)b * 2 + 1) * C + c];
        }
        const float m = s1 / (float)P;
        float mean = y[c] + m;
        float var = s2 / (float)P - m * m;
        var = var > 0.f ? var : 0.f;
        if (use_running) {   // eval()-mode batch norm under autograd: the running statistics, which stay as they are
            mean = run_mean[c];
            var = run_var[c];
        }
        const float invstd = 1.0f / sqrtf(var + eps);
        s_mean[c] = mean;
        s_scale[c] = invstd * gamma[c];
        s_shift[c] = beta[c];
        if (blockIdx.x == 0) {
            mean_out[c] = mean;
            invstd_out[c] = invstd;
            if (run_mean && !use_running && momentum > 0.f) {
                run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * mean;
                const float unbiased = P > 1 ? var * ((float)P / (float)(P - 1)) : var;
                run_var[c] = (1.0f - momentum) * run_var[c] + momentum * unbiased;
            }
        }
    }
    __syncthreads();
    const int cq = C / 4;
    const long long total = P * cq;
    for (long long i = (long long)blockIdx.x * BN_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * BN_THREADS) {
        const int q = (int)(i % cq);
        const float4 v = *reinterpret_cast<const float4*>(y + i * 4);
        float4 o;
        o.x = (v.x - s_mean[4 * q + 0]) * s_scale[4 * q + 0] + s_shift[4 * q + 0];
        o.y = (v.y - s_mean[4 * q + 1]) * s_scale[4 * q + 1] + s_shift[4 * q + 1];
        o.z = (v.z - s_mean[4 * q + 2]) * s_scale[4 * q + 2] + s_shift[4 * q + 2];
        o.w = (v.w - s_mean[4 * q + 3]) * s_scale[4 * q + 3] + s_shift[4 * q + 3];
        if (resid) {
            const float4 r = *reinterpret_cast<const float4*>(resid + i * 4);
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        if (relu) {
            o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
        }
        *reinterpret_cast<float4*>(out + i * 4) = o;
    }
}

// ------------------------------------------------------------------------------------------------ batch norm, backward
// g = d_out * (out > 0) (out == nullptr: no relu behind this batch norm);  x^ = (y - mean) invstd;
// part[b][0][c] = sum g, part[b][1][c] = sum g x^ over the workgroup's pixel range.
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_stats_kernel(const float* __restrict__ d_out, const float* __restrict__ out,
                                                                  const float* __restrict__ y, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, long long P, int C,
                                                                  long long chunk, float* __restrict__ part) {
    __shared__ float4 red[2][BN_THREADS];
    const int cq = C / 4, rows = BN_THREADS / cq;
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    const float4 mu = *reinterpret_cast<const float4*>(mean + 4 * q), is = *reinterpret_cast<const float4*>(invstd + 4 * q);
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    for (long long p = p0 + r; p < p1; p += 4 * rows) {
        float4 gg[4], aa[4], vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long pp = p + (long long)u * rows;
            const bool ok = pp < p1;
            const size_t o = (size_t)(ok ? pp : p) * C + 4 * q;
            gg[u] = *reinterpret_cast<const float4*>(d_out + o);
            aa[u] = out ? *reinterpret_cast<const float4*>(out + o) : make_float4(1.f, 1.f, 1.f, 1.f);
            vv[u] = *reinterpret_cast<const float4*>(y + o);
            if (!ok) gg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float4 g = gg[u];
            const float4 a = aa[u], v = vv[u];
            g.x = a.x > 0.f ? g.x : 0.f; g.y = a.y > 0.f ? g.y : 0.f; g.z = a.z > 0.f ? g.z : 0.f; g.w = a.w > 0.f ? g.w : 0.f;
            s1.x += g.x; s1.y += g.y; s1.z += g.z; s1.w += g.w;
            s2.x += g.x * ((v.x - mu.x) * is.x); s2.y += g.y * ((v.y - mu.y) * is.y);
            s2.z += g.z * ((v.z - mu.z) * is.z); s2.w += g.w * ((v.w - mu.w) * is.w);
        }
    }
    red[0][threadIdx.x] = s1;
    red[1][threadIdx.x] = s2;
    __syncthreads();
    if (r == 0) {
        for (int i = 1; i < rows; ++i) {
            const float4 a = red[0][i * cq + q], b = red[1][i * cq + q];
            s1.x += a.x; s1.y += a.y; s1.z += a.z; s1.w += a.w;
            s2.x += b.x; s2.y += b.y; s2.z += b.z; s2.w += b.w;
        }
        *reinterpret_cast<float4*>(part + ((size_t)blockIdx.x * 2 + 0) * C + 4 * q) = s1;
        *reinterpret_cast<float4*>(part + ((size_t)blockIdx.x * 2 + 1) * C + 4 * q) = s2;
    }
}

// dy = gamma invstd (g - mean(g) - x^ mean(g x^));  d gamma = sum g x^, d beta = sum g (workgroup 0; written, not added: the
// gradient buffers are fresh);  g_out (optional) = the masked upstream gradient, which is also the gradient of the block's
// identity branch.
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const float* __restrict__ d_out, const float* __restrict__ out,
                                                                  const float* __restrict__ y, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ part, int B, long long P, int C,
                                                                  float* __restrict__ dy, float* __restrict__ g_out,
                                                                  float* __restrict__ d_gamma, float* __restrict__ d_beta,
                                                                  int use_running) {
    __shared__ float s_mean[256], s_is[256], s_a[256], s_mg[256], s_mgx[256];
    for (int c = threadIdx.x; c < C; c += BN_THREADS) {
        float s1 = 0.f, s2 = 0.f;
        for (int b = 0; b < B; ++b) {
            s1 += part[((size_t)b * 2 + 0) * C + c];
            s2 += part[((size_t)b * 2 + 1) * C + c];
        }
        s_mean[c] = mean[c];
        s_is[c] = invstd[c];
        s_a[c] = gamma[c] * invstd[c];
        // eval()-mode statistics do not depend on the batch: dy = gamma invstd g, no mean terms
        s_mg[c] = use_running ? 0.f : s1 / (float)P;
        s_mgx[c] = use_running ? 0.f : s2 / (float)P;
        if (blockIdx.x == 0) {
            if (d_gamma) d_gamma[c] = s2;
            if (d_beta) d_beta[c] = s1;
        }
    }
    __syncthreads();
    const int cq = C / 4;
    const long long total = P * cq;
    for (long long i = (long long)blockIdx.x * BN_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * BN_THREADS) {
        const int c0 = 4 * (int)(i % cq);
        float4 g = *reinterpret_cast<const float4*>(d_out + i * 4);
        if (out) {
            const float4 a = *reinterpret_cast<const float4*>(out + i * 4);
            g.x = a.x > 0.f ? g.x : 0.f; g.y = a.y > 0.f ? g.y : 0.f; g.z = a.z > 0.f ? g.z : 0.f; g.w = a.w > 0.f ? g.w : 0.f;
        }
        const float4 v = *reinterpret_cast<const float4*>(y + i * 4);
        float4 o;
        o.x = s_a[c0 + 0] * (g.x - s_mg[c0 + 0] - (v.x - s_mean[c0 + 0]) * s_is[c0 + 0] * s_mgx[c0 + 0]);
        o.y = s_a[c0 + 1] * (g.y - s_mg[c0 + 1] - (v.y - s_mean[c0 + 1]) * s_is[c0 + 1] * s_mgx[c0 + 1]);
        o.z = s_a[c0 + 2] * (g.z - s_mg[c0 + 2] - (v.z - s_mean[c0 + 2]) * s_is[c0 + 2] * s_mgx[c0 + 2]);
        o.w = s_a[c0 + 3] * (g.w - s_mg[c0 + 3] - (v.w - s_mean[c0 + 3]) * s_is[c0 + 3] * s_mgx[c0 + 3]);
        *reinterpret_cast<float4*>(dy + i * 4) = o;
        if (g_out) *reinterpret_cast<float4*>(g_out + i * 4) = g;
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// dW[co][(tap, ci)] = sum over pixels p of dy[p][co] x[pixel of tap (ky, kx) at p][ci]: a GEMM whose contraction runs over the
// N H W output pixels.  A wave owns a 64 (co) x 128 (tap, ci) tile of the result for one slice of the pixels: 2 x 4 accumulator
// tiles of v_mfma_f32_32x32x2_f32; a k-step is TWO pixels (lane half hh takes pixel p + hh).  The row / column a lane feeds is
// free as long as the epilogue agrees, so a lane takes CONSECUTIVE channels -- 2 of co (one 8-byte load of dy), 4 of (tap, ci)
// (one 16-byte load of x: cin_p is a multiple of 4, so the four share a tap) -- and MFMA (i, j) multiplies component i of the
// one by component j of the other: rows 2 m + i, columns 4 m + j.  Partials [split][co][Kp] are summed by
// conv_dw_reduce_kernel in a fixed order.
struct DwcArgs {
    const float* dy;   // (P, cout)
    const float* x;    // (n, hin, win, cin_p)
    float* partial;    // [splits][cout][Kp]
    int n, hin, win, cin_p, hout, wout, cout, k, stride, pad, Kp, ntiles, splits;
    long long npix, chunk;
};

__global__ __launch_bounds__(256) void conv_dw_kernel(const DwcArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 31, hh = lane >> 5;
    const long long item = (long long)blockIdx.x * 4 + wave;
    const int mtiles = a.cout / 64;
    const long long n_items = (long long)mtiles * a.ntiles * a.splits;
    if (item >= n_items) return;
    const int split = (int)(item / (mtiles * a.ntiles));
    const int rem = (int)(item - (long long)split * mtiles * a.ntiles);
    const int mt = rem / a.ntiles, nt = rem - mt * a.ntiles;
    const int co = 64 * mt + 2 * m;
    const int nn = 128 * nt + 4 * m;
    const bool n_ok = nn < a.Kp;
    const int tap = n_ok ? nn / a.cin_p : 0, ci = n_ok ? nn - tap * a.cin_p : 0;
    const int ky = tap / a.k, kx = tap - ky * a.k;
    const long long p_lo = (long long)split * a.chunk, p_hi = p_lo + a.chunk < a.npix ? p_lo + a.chunk : a.npix;
    const int per = a.hout * a.wout;
    f32x16t acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    auto fetch = [&](long long p, float2& A, float4& Bv) {
        A = make_float2(0.f, 0.f);
        Bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < p_hi) {
            A = *reinterpret_cast<const float2*>(a.dy + (size_t)p * a.cout + co);
            const int img = (int)(p / per), r = (int)(p - (long long)img * per);
            const int oy = r / a.wout, ox = r - oy * a.wout;
            const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
            if (n_ok && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win)
                Bv = *reinterpret_cast<const float4*>(a.x + (((size_t)img * a.hin + iy) * a.win + ix) * a.cin_p + ci);
        }
    };
    // eight pixels (four k-steps) per trip, the next trip's operands in flight underneath: the slices are short (tens of
    // pixels), so what a launch costs is the latency of its dependent loads
    float2 A0[4], A1[4];
    float4 B0[4], B1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) fetch(p_lo + 2 * u + hh, A0[u], B0[u]);
#define PNY_DW_STEP(A, Bv)                                                                                   \
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.x, Bv.x, acc[0][0], 0, 0, 0);                           \
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.x, Bv.y, acc[0][1], 0, 0, 0);                           \
    acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.x, Bv.z, acc[0][2], 0, 0, 0);                           \
    acc[0][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.x, Bv.w, acc[0][3], 0, 0, 0);                           \
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.y, Bv.x, acc[1][0], 0, 0, 0);                           \
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.y, Bv.y, acc[1][1], 0, 0, 0);                           \
    acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.y, Bv.z, acc[1][2], 0, 0, 0);                           \
    acc[1][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(A.y, Bv.w, acc[1][3], 0, 0, 0);
    for (long long p = p_lo; p < p_hi; p += 16) {
#pragma unroll
        for (int u = 0; u < 4; ++u) fetch(p + 8 + 2 * u + hh, A1[u], B1[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) { PNY_DW_STEP(A0[u], B0[u]) }
        if (p + 8 < p_hi) {
#pragma unroll
            for (int u = 0; u < 4; ++u) fetch(p + 16 + 2 * u + hh, A0[u], B0[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) { PNY_DW_STEP(A1[u], B1[u]) }
        }
    }
#undef PNY_DW_STEP
    // accumulator (i, j), register 4 q + r of lane (m, hh): row (A lane) 8 q + 4 hh + r, column (B lane) m
    //   -> co = 64 mt + 2 (8 q + 4 hh + r) + i,  (tap, ci) = 128 nt + 4 m + j
    if (!n_ok) return;
    float* dst = a.partial + ((size_t)split * a.cout) * a.Kp;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 64 * mt + 2 * (8 * q + 4 * hh + r) + i;
                const float4 v = make_float4(acc[i][0][4 * q + r], acc[i][1][4 * q + r], acc[i][2][4 * q + r], acc[i][3][4 * q + r]);
                *reinterpret_cast<float4*>(dst + (size_t)row * a.Kp + nn) = v;
            }
}

// dW (cout, cin, k, k) = sum over the splits, fixed order
__global__ void conv_dw_reduce_kernel(const float* __restrict__ partial, int splits, int cout, int cin, int cin_p, int k, int Kp,
                                      float* __restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int kk2 = k * k;
    if (i >= cout * cin * kk2) return;
    const int tap = i % kk2, ci = (i / kk2) % cin, co = i / (kk2 * cin);
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += partial[((size_t)sp * cout + co) * Kp + tap * cin_p + ci];
    dw[i] = s;
}

// ------------------------------------------------------------------------------------------------ pool / pyramid, backward
// max_pool2d(3, stride 2, pad 1) backward as a gather: input position (iy, ix) collects the gradient of every window whose
// FIRST maximum in scan order it is (ATen keeps the first maximum: `val > maxval`).  d_in = result (+ add, optional).
__global__ void maxpool_bwd_kernel(const float* __restrict__ in, const float* __restrict__ g, const float* __restrict__ add,
                                   float* __restrict__ d_in, int n, int hin, int win, int c, int hout, int wout) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int cq = c / 4;
    if (i >= (long long)n * hin * win * cq) return;
    const int q = (int)(i % cq);
    long long p = i / cq;
    const int ix = (int)(p % win);
    p /= win;
    const int iy = (int)(p % hin), img = (int)(p / hin);
    const float* base = in + (size_t)img * hin * win * c + 4 * q;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int oy_lo = iy > 0 ? (iy) / 2 : 0, oy_hi = (iy + 1) / 2;   // windows oy with 2 oy - 1 <= iy <= 2 oy + 1
    const int ox_lo = ix > 0 ? (ix) / 2 : 0, ox_hi = (ix + 1) / 2;
    for (int oy = oy_lo; oy <= oy_hi && oy < hout; ++oy)
        for (int ox = ox_lo; ox <= ox_hi && ox < wout; ++ox) {
            if (iy < 2 * oy - 1 || iy > 2 * oy + 1 || ix < 2 * ox - 1 || ix > 2 * ox + 1) continue;
            float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int arg[4] = {-1, -1, -1, -1};
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) {
                    const int yy = oy * 2 - 1 + dy, xx = ox * 2 - 1 + dx;
                    if (yy < 0 || yy >= hin || xx < 0 || xx >= win) continue;
                    const float4 v = *reinterpret_cast<const float4*>(base + ((size_t)yy * win + xx) * c);
                    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (vv[e] > best[e]) {
                            best[e] = vv[e];
                            arg[e] = yy * win + xx;
                        }
                }
            const float4 gg = *reinterpret_cast<const float4*>(g + (((size_t)img * hout + oy) * wout + ox) * c + 4 * q);
            const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (arg[e] == iy * win + ix) acc[e] += gv[e];
        }
    float4 o = make_float4(acc[0], acc[1], acc[2], acc[3]);
    if (add) {
        const float4 t = *reinterpret_cast<const float4*>(add + i * 4);
        o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
    }
    *reinterpret_cast<float4*>(d_in + i * 4) = o;
}

// Backward of upsample_concat_kernel (bilinear, align_corners = True) for one pyramid level, as a gather: low-resolution
// position (y, x) collects w_y w_x d_lat[oy][ox] from the output pixels whose footprint holds it, with the weights the forward
// computed.  d_lat (n, h0, w0, ctot), channels [coff, coff + c); result (n, hin, win, c) (+ add, optional).
__global__ void upsample_bwd_kernel(const float* __restrict__ d_lat, const float* __restrict__ add, float* __restrict__ d_in, int n,
                                    int hin, int win, int c, int h0, int w0, int ctot, int coff) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int cq = c / 4;
    if (i >= (long long)n * hin * win * cq) return;
    const int q = (int)(i % cq);
    long long p = i / cq;
    const int x = (int)(p % win);
    p /= win;
    const int y = (int)(p % hin), img = (int)(p / hin);
    const float sy = h0 > 1 ? (float)(hin - 1) / (float)(h0 - 1) : 0.f;
    const float sx = w0 > 1 ? (float)(win - 1) / (float)(w0 - 1) : 0.f;
    // candidate output rows: sy * oy in (y - 1, y + 1)
    int oy_lo = sy > 0.f ? (int)floorf((float)(y - 1) / sy) : 0, oy_hi = sy > 0.f ? (int)ceilf((float)(y + 1) / sy) : h0 - 1;
    int ox_lo = sx > 0.f ? (int)floorf((float)(x - 1) / sx) : 0, ox_hi = sx > 0.f ? (int)ceilf((float)(x + 1) / sx) : w0 - 1;
    oy_lo = oy_lo < 0 ? 0 : oy_lo;
    ox_lo = ox_lo < 0 ? 0 : ox_lo;
    oy_hi = oy_hi > h0 - 1 ? h0 - 1 : oy_hi;
    ox_hi = ox_hi > w0 - 1 ? w0 - 1 : ox_hi;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        const float fy = sy * (float)oy;
        const int y0 = (int)fy, y1 = y0 + (y0 < hin - 1 ? 1 : 0);
        const float ly1 = fy - (float)y0, ly0 = 1.0f - ly1;
        const float wy = (y0 == y ? ly0 : 0.f) + (y1 == y ? ly1 : 0.f);
        if (wy == 0.f) continue;
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const float fx = sx * (float)ox;
            const int x0 = (int)fx, x1 = x0 + (x0 < win - 1 ? 1 : 0);
            const float lx1 = fx - (float)x0, lx0 = 1.0f - lx1;
            const float wx = (x0 == x ? lx0 : 0.f) + (x1 == x ? lx1 : 0.f);
            if (wx == 0.f) continue;
            const float4 g = *reinterpret_cast<const float4*>(d_lat + (((size_t)img * h0 + oy) * w0 + ox) * ctot + coff + 4 * q);
            const float w = wy * wx;
            acc.x += w * g.x; acc.y += w * g.y; acc.z += w * g.z; acc.w += w * g.w;
        }
    }
    if (add) {
        const float4 t = *reinterpret_cast<const float4*>(add + i * 4);
        acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
    *reinterpret_cast<float4*>(d_in + i * 4) = acc;
}

// dst = a + b (float4 elements); b may be null
__global__ void add2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dst, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<const float4*>(a)[i];
    if (b) {
        const float4 t = reinterpret_cast<const float4*>(b)[i];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    reinterpret_cast<float4*>(dst)[i] = v;
}

// ------------------------------------------------------------------------------------------------ host side
// One convolution + batch norm of the trunk, with everything the backward needs
struct TrunkUnit {
    const TrunkConv* c = nullptr; // its entry of trunk_table()
    std::string conv, bn;         // state_dict prefixes ("encoder.model.layer1.0.conv1", "...bn1")
    ConvLayer fwd, bwd;           // the convolution on the packed live weights, scale 1 / shift 0; the transposed convolution of
                                  // its input gradient (flipped, transposed filters; bwd.w null where that is never needed)
    int hin, win, hout, wout;
    const float* x = nullptr;     // input activation (n, hin, win, cin_p)
    const float* resid = nullptr; // residual added before the relu (or null)
    bool relu = true;
    float *y = nullptr, *out = nullptr, *mean = nullptr, *invstd = nullptr;
};
// a packed operand's size in 16-byte elements
static int pack_count(const ConvLayer& L) { return (L.cout / 32) * L.J * 64; }

// every job of a device-side table in one launch; max_count = the largest job's count
static void launch_trunk_pack(const TrunkPackJob* jobs_dev, int n_jobs, int max_count, hipStream_t st) {
    int bx = (max_count + 255) / 256;
    if (bx > 128) bx = 128;
    hipLaunchKernelGGL(trunk_pack_kernel, dim3(bx, n_jobs), dim3(256), 0, st, jobs_dev);
}

// the transposed convolution of a unit's input gradient (conv_pack_src_t images): stride 1 over the (dilated) output gradient
static ConvLayer transposed_geometry(const TrunkConv& c) {
    ConvLayer L;
    L.cin = L.cin_p = c.cout;
    L.cout = c.cin;
    L.k = c.k;
    L.stride = 1;
    L.pad = c.k - 1 - c.pad;
    L.J = c.k * c.k * c.cout / 8;
    return L;
}
// a stride-2 convolution's gradient is read as a dilated input
static int transposed_dil_shift(const ConvLayer& fwd) { return fwd.stride == 2 ? 1 : 0; }
static TrunkPackJob pack_job(const ConvLayer& fwd, const ConvLayer& L, int kind, const float* src, float* dst) {
    return {src, dst, kind, fwd.cout, fwd.cin, fwd.cin_p, fwd.k, L.J, pack_count(L)};
}

struct TrunkTrain {
    DevBuf work, packs, jobs, part, dwpart, ones;
    std::vector<TrunkUnit> units;
    int n = 0, height = 0, width = 0;
    bool pool = true;
    Pyramid d = {};
    float* img4 = nullptr;
    float* pooled = nullptr;
    const float* level_out[4] = {nullptr, nullptr, nullptr, nullptr};
    // gradient scratch (carved from `work`)
    static constexpr int NSCR = 8;
    float* scr[NSCR] = {};
    float* d_level[4] = {nullptr, nullptr, nullptr, nullptr};
    float* lat_nhwc = nullptr;
    // weight gradients run on a side stream beside the chain of input gradients (which is the critical path); an event per
    // scratch buffer says when the side stream's last reader of it is done
    Stream side;
    Event ev_ready, ev_join, ev_buf[NSCR];
    // pack-job table: host copy (the source of the stream-ordered upload), and events after the last upload / pack launch
    std::vector<TrunkPackJob> host_jobs;
    Event ev_upload, ev_pack;
    bool pend[NSCR] = {};
    bool have_forward = false;
    bool bn_eval = false;    // batch norm on the running statistics (modules in eval() mode under autograd)
    int n_jobs = 0;
};

void trunk_release(TrunkTrain* t) { delete t; }   // pny_model_destroy, its only caller, has drained the device

static void dw_split(const ConvLayer& L, long long npix, int* splits, long long* chunk);
static size_t dw_partial_floats(const ConvLayer& L, long long npix);

static int find_param(pny_model* m, const std::string& name, const float** out) {
    auto it = m->params_dev.find(name);
    if (it == m->params_dev.end()) return fail(PNY_ERR_STATE, "trunk training: no device pointer bound for '" + name + "' (pny_model_bind_param)");
    *out = it->second;
    return 0;
}
static float* find_grad(pny_model* m, const std::string& name) {
    auto it = m->grads.find(name);
    return it == m->grads.end() ? nullptr : it->second;
}

// The work buffer (image, per unit y / out / mean / invstd, pooled level, gradient scratch, level gradients, latent) and the
// packed operands, laid out from `work` / `packs`; null: sizes only.  Sizes in floats.
static void trunk_layout(TrunkTrain& T, float* work, float* packs, size_t* work_fl, size_t* packs_fl) {
    const size_t n = T.n;
    Carver c{work}, pk{packs};
    T.img4 = c.take(n * T.height * T.width * 4);
    size_t max_act = n * T.d.h[0] * T.d.w[0] * TRUNK_CH[0];
    for (TrunkUnit& u : T.units) {
        const size_t act = n * u.hout * u.wout * u.fwd.cout;
        u.y = c.take(act);
        u.out = c.take(act);
        u.mean = c.take(u.fwd.cout);
        u.invstd = c.take(u.fwd.cout);
        max_act = std::max(max_act, act);
        u.fwd.w = pk.take((size_t)pack_count(u.fwd) * 4);
        u.bwd.w = u.fwd.cin >= 32 ? pk.take((size_t)pack_count(u.bwd) * 4) : nullptr;   // conv1's input gradient (the images) is never needed
    }
    T.pooled = c.take(n * T.d.h[1] * T.d.w[1] * TRUNK_CH[0]);
    for (float*& p : T.scr) p = c.take(max_act);
    for (int lv = 0; lv < 4; ++lv) T.d_level[lv] = c.take(n * T.d.h[lv] * T.d.w[lv] * TRUNK_CH[lv]);
    T.lat_nhwc = c.take(n * T.d.h[0] * T.d.w[0] * TRUNK_LATENT);
    *work_fl = c.off;
    *packs_fl = pk.off;
}

// lays out units, activations and packs for n images of height x width; (re)allocates when the shape changed
static int trunk_plan(pny_model* m, TrunkTrain& T, int n, int height, int width) {
    const bool pool = m->desc.enc_use_first_pool != 0;
    if (T.n == n && T.height == height && T.width == width && T.pool == pool && !T.units.empty()) return 0;
    T.units.clear();
    T.n = n;
    T.height = height;
    T.width = width;
    T.pool = pool;
    T.d = pyramid(height, width, pool);
    int hin = height, win = width;
    for (const TrunkConv& c : trunk_table()) {
        TrunkUnit u;
        u.c = &c;
        u.conv = "encoder.model." + c.conv;
        u.bn = "encoder.model." + c.bn;
        u.fwd = conv_geometry(c);
        u.bwd = transposed_geometry(c);
        u.hin = hin;
        u.win = win;
        u.hout = conv_out(hin, c.k, c.stride, c.pad);
        u.wout = conv_out(win, c.k, c.stride, c.pad);
        T.units.push_back(u);
        // the next unit's input: a block's downsample and conv1 read the same activation; layer1 reads the (pooled) stem
        if (c.role == TrunkRole::stem) hin = T.d.h[1], win = T.d.w[1];
        else if (c.role != TrunkRole::downsample) hin = u.hout, win = u.wout;
    }
    size_t work_fl, packs_fl;
    trunk_layout(T, nullptr, nullptr, &work_fl, &packs_fl);
    int rc;
    if ((rc = T.work.reserve(work_fl * sizeof(float))) || (rc = T.packs.reserve(packs_fl * sizeof(float)))) return rc;
    trunk_layout(T, T.work.f(), T.packs.f(), &work_fl, &packs_fl);
    // ones / zeros for the raw convolution (scale 1, shift 0)
    if ((rc = T.ones.reserve(512 * sizeof(float)))) return rc;
    {
        std::vector<float> v(512, 0.f);
        for (int i = 0; i < 256; ++i) v[i] = 1.0f;
        PNY_HIP(hipMemcpy(T.ones.p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        for (TrunkUnit& u : T.units) {
            u.fwd.scale = u.bwd.scale = T.ones.f();
            u.fwd.shift = u.bwd.shift = T.ones.f() + 256;
        }
    }
    if ((rc = T.part.reserve(BN_PART_FLOATS * sizeof(float)))) return rc;
    {   // the largest weight-gradient partial buffer of any unit (never reallocated while a side-stream launch may read it)
        size_t mx = 0;
        for (const TrunkUnit& u : T.units) {
            mx = std::max(mx, dw_partial_floats(u.fwd, (long long)n * u.hout * u.wout));
        }
        if ((rc = T.dwpart.reserve(mx * sizeof(float)))) return rc;
    }
    T.have_forward = false;
    T.n_jobs = 0;   // the job table depends on the parameter pointers: rebuilt at the next forward
    return 0;
}

// pny_model_bind_param on a trunk parameter: the pack-job table holds the device pointers of the conv weights it resolved, so a
// parameter that moved to new storage (load_state_dict(assign=True), p.data = ...) must be resolved again at the next forward
void trunk_params_rebound(TrunkTrain* t) {
    if (t) t->n_jobs = 0;
}

static int trunk_upload_jobs(pny_model* m, TrunkTrain& T, hipStream_t st) {
    std::vector<TrunkPackJob> jobs;
    int rc;
    // stream-ordered (no device-wide wait): a table uploaded before may still be read by the pack launch of an earlier forward
    // on another stream, and the previous upload may still be reading host_jobs (rare: after a re-bind or a new shape)
    if (!T.ev_upload) {
        if ((rc = T.ev_upload.ensure(hipEventDisableTiming, "hipEventCreate(trunk job upload)"))) return rc;
        if ((rc = T.ev_pack.ensure(hipEventDisableTiming, "hipEventCreate(trunk pack)"))) return rc;
    } else {
        PNY_HIP(hipEventSynchronize(T.ev_upload));     // the previous upload has read host_jobs
        PNY_HIP(hipStreamWaitEvent(st, T.ev_pack, 0));  // ... and the last pack launch (any stream) the old table
    }
    for (TrunkUnit& u : T.units) {
        const float* w = nullptr;
        if ((rc = find_param(m, u.conv + ".weight", &w))) return rc;
        jobs.push_back(pack_job(u.fwd, u.fwd, 0, w, u.fwd.w));
        if (u.bwd.w) jobs.push_back(pack_job(u.fwd, u.bwd, 1, w, u.bwd.w));
    }
    if ((rc = T.jobs.reserve(jobs.size() * sizeof(TrunkPackJob)))) return rc;
    T.host_jobs = jobs;
    PNY_HIP(hipMemcpyAsync(T.jobs.p, T.host_jobs.data(), jobs.size() * sizeof(TrunkPackJob), hipMemcpyHostToDevice, st));
    PNY_HIP(hipEventRecord(T.ev_upload, st));
    T.n_jobs = (int)jobs.size();
    return 0;
}

static void bn_grid(long long P, int* B, long long* chunk) {
    long long b = (P + 255) / 256;
    if (b > BN_MAXB) b = BN_MAXB;
    if (b < 1) b = 1;
    *chunk = (P + b - 1) / b;
    *B = (int)((P + *chunk - 1) / *chunk);
}

// Batch norm over the P pixels of a channel-last (P, C) tensor, C in {64, 128, 256}: the statistics launch and the apply launch
static void launch_bn_forward(const float* y, long long P, int C, const float* gamma, const float* beta, const float* resid, int relu,
                              float* out, float* mean, float* invstd, float* run_mean, float* run_var, float momentum, int use_running,
                              float* part, hipStream_t st) {
    int B;
    long long chunk;
    bn_grid(P, &B, &chunk);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(B), dim3(BN_THREADS), 0, st, y, P, C, chunk, part);
    const long long total = P * (C / 4);
    long long grid = (total + BN_THREADS - 1) / BN_THREADS;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)grid), dim3(BN_THREADS), 0, st, y, part, B, P, C, gamma, beta, resid, relu, out, mean,
                       invstd, run_mean, run_var, momentum, 1e-5f, use_running);
}

// ... and its backward: d_out (through the relu mask `mask`, or null) -> dy, optional g_out / d_gamma / d_beta
static void launch_bn_backward(const float* d_out, const float* mask, const float* y, const float* mean, const float* invstd,
                               const float* gamma, long long P, int C, float* dy, float* g_out, float* d_gamma, float* d_beta,
                               int use_running, float* part, hipStream_t st) {
    int B;
    long long chunk;
    bn_grid(P, &B, &chunk);
    hipLaunchKernelGGL(bn_bwd_stats_kernel, dim3(B), dim3(BN_THREADS), 0, st, d_out, mask, y, mean, invstd, P, C, chunk, part);
    const long long total = P * (C / 4);
    long long grid = (total + BN_THREADS - 1) / BN_THREADS;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)grid), dim3(BN_THREADS), 0, st, d_out, mask, y, mean, invstd, gamma, part, B, P, C, dy,
                       g_out, d_gamma, d_beta, use_running);
}

static int unit_forward(pny_model* m, TrunkTrain& T, TrunkUnit& u, float momentum, hipStream_t st) {
    if (!run_conv_ex(u.fwd, u.x, T.n, u.hin, u.win, u.hout, u.wout, 0, nullptr, 0, u.y, st)) return fail(PNY_ERR_HIP, "trunk training: convolution launch failed");
    const long long P = (long long)T.n * u.hout * u.wout;
    const float *gamma, *beta, *rm, *rv;
    int rc;
    if ((rc = find_param(m, u.bn + ".weight", &gamma)) || (rc = find_param(m, u.bn + ".bias", &beta)) ||
        (rc = find_param(m, u.bn + ".running_mean", &rm)) || (rc = find_param(m, u.bn + ".running_var", &rv)))
        return rc;
    launch_bn_forward(u.y, P, u.fwd.cout, gamma, beta, u.resid, u.relu ? 1 : 0, u.out, u.mean, u.invstd, const_cast<float*>(rm),
                      const_cast<float*>(rv), momentum, T.bn_eval ? 1 : 0, T.part.f(), st);
    PNY_HIP(hipGetLastError());
    return 0;
}

// forward over n images (n, 3, H, W) NCHW -> latent (n, 512, hl, wl) NCHW; keeps the activations for trunk_train_backward
int trunk_train_forward(pny_model* m, const float* images, int n, int height, int width, float momentum, int bn_eval,
                        float* latent_nchw, hipStream_t st) {
    if (!m->trunk) m->trunk = new TrunkTrain();
    TrunkTrain& T = *m->trunk;
    T.bn_eval = bn_eval != 0;
    int rc;
    if ((rc = trunk_plan(m, T, n, height, width))) return rc;
    if (T.n_jobs == 0 && (rc = trunk_upload_jobs(m, T, st))) return rc;
    T.have_forward = false;
    // weights of this step: one launch rebuilds every packed operand from the live parameters
    {
        int mx = 0;
        for (const TrunkUnit& u : T.units) mx = std::max(mx, std::max(pack_count(u.fwd), u.bwd.w ? pack_count(u.bwd) : 0));
        launch_trunk_pack(reinterpret_cast<const TrunkPackJob*>(T.jobs.p), T.n_jobs, mx, st);
        PNY_HIP(hipEventRecord(T.ev_pack, st));
    }
    launch_image_to_nhwc4(images, T.img4, n, height, width, st);
    const float *x = T.img4, *idt = nullptr, *a1 = nullptr;   // the block's input, its identity branch, conv1's output
    for (TrunkUnit& u : T.units) {
        const TrunkRole role = u.c->role;
        u.x = role == TrunkRole::conv2 ? a1 : x;
        u.resid = role == TrunkRole::conv2 ? idt : nullptr;
        u.relu = role != TrunkRole::downsample;   // downsample branch: bn(conv1x1(x)), no relu
        if ((rc = unit_forward(m, T, u, momentum, st))) return rc;
        switch (role) {
            case TrunkRole::stem:
                x = u.out;
                if (T.pool) {
                    launch_first_pool(u.out, T.pooled, n, T.d, st);
                    x = T.pooled;
                }
                idt = x;
                break;
            case TrunkRole::downsample: idt = u.out; break;
            case TrunkRole::conv1: a1 = u.out; break;
            case TrunkRole::conv2: x = idt = u.out; break;
        }
        if (u.c->level_end) T.level_out[u.c->level] = u.out;
    }
    launch_pyramid_to_latent(T.level_out, T.lat_nhwc, n, T.d, st);
    launch_nhwc_to_nchw(T.lat_nhwc, latent_nchw, n, TRUNK_LATENT, T.d.h[0] * T.d.w[0], st);
    PNY_HIP(hipGetLastError());
    T.have_forward = true;
    return 0;
}

// pixel slices of a unit's weight-gradient GEMM: ~4 waves per CU in all, at least 128 pixels per slice
static void dw_split(const ConvLayer& L, long long npix, int* splits, long long* chunk) {
    const int Kp = L.k * L.k * L.cin_p;
    const long long base = (long long)(L.cout / 64) * ((Kp + 127) / 128);
    long long sp = (1024 + base - 1) / base;
    const long long max_splits = std::max(1ll, npix / 128);
    if (sp > max_splits) sp = max_splits;
    if (sp < 1) sp = 1;
    *chunk = ((npix + sp - 1) / sp + 3) / 4 * 4;   // the pixel loop walks 4 pixels per iteration
    *splits = (int)((npix + *chunk - 1) / *chunk);
}

// floats of the partials buffer of a unit's weight gradient over npix output pixels
static size_t dw_partial_floats(const ConvLayer& L, long long npix) {
    int sp;
    long long ch;
    dw_split(L, npix, &sp, &ch);
    return (size_t)sp * L.cout * L.k * L.k * L.cin_p;
}

// dw (cout, cin, k, k) of convolution L from dy (n, hout, wout, cout) and its input x (n, hin, win, cin_p): the split-K GEMM
// and the reduction of its partials.  False (nothing launched) when `partial` is too small.  Reports the pixel slicing.
static bool launch_conv_dw(const ConvLayer& L, const float* dy, const float* x, int n, int hin, int win, int hout, int wout, float* partial,
                           size_t partial_bytes, float* dw, hipStream_t st, int* splits, long long* chunk) {
    DwcArgs a;
    a.dy = dy;
    a.x = x;
    a.n = n;
    a.hin = hin;
    a.win = win;
    a.cin_p = L.cin_p;
    a.hout = hout;
    a.wout = wout;
    a.cout = L.cout;
    a.k = L.k;
    a.stride = L.stride;
    a.pad = L.pad;
    a.Kp = L.k * L.k * L.cin_p;
    a.ntiles = (a.Kp + 127) / 128;
    a.npix = (long long)n * hout * wout;
    const long long base = (long long)(L.cout / 64) * a.ntiles;
    dw_split(L, a.npix, &a.splits, &a.chunk);
    if (splits) *splits = a.splits;
    if (chunk) *chunk = a.chunk;
    if ((size_t)a.splits * L.cout * a.Kp * sizeof(float) > partial_bytes) return false;
    a.partial = partial;
    const long long items = base * a.splits;
    hipLaunchKernelGGL(conv_dw_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, a);
    const int tot = L.cout * L.cin * L.k * L.k;
    hipLaunchKernelGGL(conv_dw_reduce_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, partial, a.splits, L.cout, L.cin, L.cin_p, L.k, a.Kp, dw);
    return true;
}

static int unit_weight_grad(pny_model* m, TrunkTrain& T, const TrunkUnit& u, const float* dy, hipStream_t main_st) {
    float* dw = find_grad(m, u.conv + ".weight");
    if (!dw) return 0;
    // on the side stream, behind the kernel that wrote dy; the buffer dy lives in is marked busy until this is done
    hipStream_t st = main_st;
    if (T.side) {
        PNY_HIP(hipEventRecord(T.ev_ready, main_st));
        PNY_HIP(hipStreamWaitEvent(T.side, T.ev_ready, 0));
        st = T.side;
    }
    if (!launch_conv_dw(u.fwd, dy, u.x, T.n, u.hin, u.win, u.hout, u.wout, T.dwpart.f(), T.dwpart.bytes, dw, st, nullptr, nullptr))
        return fail(PNY_ERR_STATE, "trunk backward: weight-gradient partials larger than planned");
    PNY_HIP(hipGetLastError());
    if (T.side)
        for (int i = 0; i < TrunkTrain::NSCR; ++i)
            if (T.scr[i] == dy) {
                PNY_HIP(hipEventRecord(T.ev_buf[i], T.side));
                T.pend[i] = true;
            }
    return 0;
}

// d_out -> [dy of the unit's convolution output in dy_buf] (+ masked gradient in g_buf), d gamma / d beta, weight gradient;
// then, if dx_buf, the input gradient dx = conv_T(dy) + dx_add
static int unit_backward(pny_model* m, TrunkTrain& T, TrunkUnit& u, const float* d_out, float* dy_buf, float* g_buf, float* dx_buf,
                         const float* dx_add, hipStream_t st) {
    const long long P = (long long)T.n * u.hout * u.wout;
    const float* gamma;
    int rc;
    if ((rc = find_param(m, u.bn + ".weight", &gamma))) return rc;
    launch_bn_backward(d_out, u.relu ? u.out : nullptr, u.y, u.mean, u.invstd, gamma, P, u.fwd.cout, dy_buf, g_buf, find_grad(m, u.bn + ".weight"),
                       find_grad(m, u.bn + ".bias"), T.bn_eval ? 1 : 0, T.part.f(), st);
    PNY_HIP(hipGetLastError());
    if ((rc = unit_weight_grad(m, T, u, dy_buf, st))) return rc;
    if (dx_buf && !run_conv_ex(u.bwd, dy_buf, T.n, u.hout, u.wout, u.hin, u.win, transposed_dil_shift(u.fwd), dx_add, 0, dx_buf, st))
        return fail(PNY_ERR_HIP, "trunk training: transposed convolution launch failed");
    return 0;
}

// gradient of max_pool2d(3, stride 2, pad 1): g (n, hout, wout, c) -> d_in (n, hin, win, c) (+ add, optional)
static void launch_maxpool_bwd(const float* in, const float* g, const float* add, float* d_in, int n, int hin, int win, int c, hipStream_t st) {
    const long long np = (long long)n * hin * win * (c / 4);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, in, g, add, d_in, n, hin, win, c,
                       conv_out(hin, 3, 2, 1), conv_out(win, 3, 2, 1));
}

// gradient of launch_upsample_level: channels of level lv in d_lat (n, h0, w0, 512) -> d_in (n, hin, win, TRUNK_CH[lv]) (+ add)
static void launch_upsample_bwd(const float* d_lat, const float* add, float* d_in, int n, int hin, int win, int lv, int h0, int w0,
                                hipStream_t st) {
    const long long np = (long long)n * hin * win * (TRUNK_CH[lv] / 4);
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, d_lat, add, d_in, n, hin, win, TRUNK_CH[lv], h0, w0,
                       TRUNK_LATENT, TRUNK_COFF[lv]);
}

// d loss / d latent (n, 512, hl, wl) NCHW -> gradients of every bound encoder parameter
int trunk_train_backward(pny_model* m, const float* d_latent_nchw, hipStream_t st) {
    if (!m->trunk || !m->trunk->have_forward) return fail(PNY_ERR_STATE, "pny_trunk_train_backward: no training forward to differentiate");
    TrunkTrain& T = *m->trunk;
    const int n = T.n;
    int rc;
    // pyramid: level gradients from the latent's channel groups
    float* d_lat = T.lat_nhwc;   // (the forward's channel-last latent is no longer needed)
    const Pyramid& d = T.d;
    launch_nchw_to_nhwc(d_latent_nchw, d_lat, n, TRUNK_LATENT, d.h[0] * d.w[0], st);
    for (int lv = 0; lv < 4; ++lv) launch_upsample_bwd(d_lat, nullptr, T.d_level[lv], n, d.h[lv], d.w[lv], lv, d.h[0], d.w[0], st);
    // residual layers, last to first.  g_x = gradient w.r.t. the current block's output.  Scratch: a pool of NSCR buffers of
    // the largest activation; at most four are live at any point.
    if (!T.side && !getenv("PNYOLO_TRUNK_NO_SIDE_STREAM")) {
        if ((rc = T.side.ensure(hipStreamNonBlocking, "hipStreamCreate(trunk side stream)"))) return rc;
        if ((rc = T.ev_ready.ensure(hipEventDisableTiming, "hipEventCreate(trunk side stream)"))) return rc;
        if ((rc = T.ev_join.ensure(hipEventDisableTiming, "hipEventCreate(trunk side stream)"))) return rc;
        for (Event& e : T.ev_buf)
            if ((rc = e.ensure(hipEventDisableTiming, "hipEventCreate(trunk side stream)"))) return rc;
    }
    for (bool& b : T.pend) b = false;
    bool used[TrunkTrain::NSCR] = {};
    auto grab = [&]() -> float* {
        // prefer a buffer no weight-gradient launch on the side stream still reads
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < TrunkTrain::NSCR; ++i)
                if (!used[i] && (pass == 1 || !T.pend[i])) {
                    used[i] = true;
                    if (T.pend[i]) {
                        (void)hipStreamWaitEvent(st, T.ev_buf[i], 0);
                        T.pend[i] = false;
                    }
                    return T.scr[i];
                }
        return nullptr;
    };
    auto drop = [&](const float* ptr) {
        for (int i = 0; i < TrunkTrain::NSCR; ++i)
            if (T.scr[i] == ptr) used[i] = false;
    };
    const float* g_x = T.d_level[T.units.back().c->level];
    size_t ui = T.units.size();
    while (ui > 1) {   // block by block down to the stem
        TrunkUnit& u2 = T.units[--ui];
        TrunkUnit& u1 = T.units[--ui];
        TrunkUnit* ud = T.units[ui - 1].c->role == TrunkRole::downsample ? &T.units[--ui] : nullptr;
        // a level's output also fed the pyramid (levels 2 and 1; the last level's gradient is the pyramid's alone, level 0 goes through the pool)
        if (u2.c->level_end && &u2 != &T.units.back()) {
            const int lv = u2.c->level;
            float* sum = grab();
            if (!sum) return fail(PNY_ERR_STATE, "trunk backward: scratch pool exhausted");
            const long long n4 = (long long)n * d.h[lv] * d.w[lv] * TRUNK_CH[lv] / 4;
            hipLaunchKernelGGL(add2_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, g_x, (const float*)T.d_level[lv], sum, n4);
            drop(g_x);
            g_x = sum;
        }
        // conv2 / bn2: upstream g_x through relu(out); g = the masked gradient = gradient of the identity branch
        float *dy2 = grab(), *g = grab(), *d_a1 = grab();
        if (!dy2 || !g || !d_a1) return fail(PNY_ERR_STATE, "trunk backward: scratch pool exhausted");
        if ((rc = unit_backward(m, T, u2, g_x, dy2, g, d_a1, nullptr, st))) return rc;
        drop(g_x);
        drop(dy2);
        // conv1 / bn1: upstream d_a1 through relu(a1); without a downsample branch the identity gradient g joins here
        float *dy1 = grab(), *dx = grab();
        if (!dy1 || !dx) return fail(PNY_ERR_STATE, "trunk backward: scratch pool exhausted");
        if ((rc = unit_backward(m, T, u1, d_a1, dy1, nullptr, dx, ud ? nullptr : g, st))) return rc;
        drop(d_a1);
        drop(dy1);
        if (ud) {   // downsample branch: upstream g (no relu behind its batch norm); its input gradient is added to dx
            float *dyd = grab(), *dx2 = grab();
            if (!dyd || !dx2) return fail(PNY_ERR_STATE, "trunk backward: scratch pool exhausted");
            if ((rc = unit_backward(m, T, *ud, g, dyd, nullptr, dx2, dx, st))) return rc;
            drop(dyd);
            drop(dx);
            dx = dx2;
        }
        drop(g);
        g_x = dx;
    }
    // level 0: through the max-pool (or directly), plus its pyramid share
    float* d_l0 = grab();
    TrunkUnit& u0 = T.units[0];
    if (T.pool) {
        launch_maxpool_bwd(u0.out, g_x, T.d_level[0], d_l0, n, d.h[0], d.w[0], TRUNK_CH[0], st);   // d.h[1], d.w[1]: conv_out(., 3, 2, 1)
    } else {
        const long long n4 = (long long)n * d.h[0] * d.w[0] * 16;
        hipLaunchKernelGGL(add2_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, g_x, (const float*)T.d_level[0], d_l0, n4);
    }
    drop(g_x);
    float* dy0 = grab();
    if (!d_l0 || !dy0) return fail(PNY_ERR_STATE, "trunk backward: scratch pool exhausted");
    if ((rc = unit_backward(m, T, u0, d_l0, dy0, nullptr, nullptr, nullptr, st))) return rc;
    if (T.side) {   // the caller's stream continues only behind the last weight gradient
        PNY_HIP(hipEventRecord(T.ev_join, T.side));
        PNY_HIP(hipStreamWaitEvent(st, T.ev_join, 0));
    }
    PNY_HIP(hipGetLastError());
    T.have_forward = false;
    return 0;
}

}  // namespace pny

extern "C" {

int pny_trunk_train_forward(pny_model* m, const float* images_dev, int n_images, int height, int width, float momentum, int bn_eval,
                            float* latent_nchw_dev, pny_stream stream) {
    if (!m || !images_dev || !latent_nchw_dev) return fail(PNY_ERR_ARG, "pny_trunk_train_forward: null argument");
    if (m->desc.d_latent != 512) return fail(PNY_ERR_ARG, "pny_trunk_train_forward: the ResNet-34 trunk yields 512 channels; model d_latent differs");
    if (n_images < 1 || height < 32 || width < 32) return fail(PNY_ERR_ARG, "pny_trunk_train_forward: bad shape");
    PNY_HIP(hipSetDevice(m->desc.device));
    return trunk_train_forward(m, images_dev, n_images, height, width, momentum, bn_eval, latent_nchw_dev, (hipStream_t)stream);
}

int pny_trunk_train_backward(pny_model* m, const float* d_latent_nchw_dev, pny_stream stream) {
    if (!m || !d_latent_nchw_dev) return fail(PNY_ERR_ARG, "pny_trunk_train_backward: null argument");
    PNY_HIP(hipSetDevice(m->desc.device));
    return trunk_train_backward(m, d_latent_nchw_dev, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ stage entry points
// One trunk stage per call on caller-chosen inputs (tests/test_gpu_trunk_stages.py), through the launchers the trunk itself
// uses.  No model handle: scratch is allocated per call and the call returns once the stream has drained.
namespace {
bool bn_channels(int C) { return C == 64 || C == 128 || C == 256; }
bool fits_int(long long a, long long b, long long c) { return a * b <= 0x7fffffffll && a * b * c <= 0x7fffffffll; }
const TrunkConv* stage_unit(int unit) {
    const std::vector<TrunkConv>& t = trunk_table();
    return unit >= 0 && unit < (int)t.size() ? &t[unit] : nullptr;
}
}  // namespace

int pny_trunk_unit(int unit, int* cin, int* cout, int* k, int* stride, int* pad) {
    const TrunkConv* c = stage_unit(unit);
    if (!c) return fail(PNY_ERR_ARG, "pny_trunk_unit: unit index out of range");
    if (cin) *cin = c->cin;
    if (cout) *cout = c->cout;
    if (k) *k = c->k;
    if (stride) *stride = c->stride;
    if (pad) *pad = c->pad;
    return PNY_OK;
}

int pny_trunk_conv(int unit, int transposed, const float* weight_dev, const float* in_dev, int n, int hin, int win, int hout, int wout,
                   const float* scale_dev, const float* shift_dev, const float* resid_dev, int relu, float* out_dev, int* variant,
                   pny_stream stream) {
    const TrunkConv* c = stage_unit(unit);
    if (!c) return fail(PNY_ERR_ARG, "pny_trunk_conv: unit index out of range");
    if (!weight_dev || !in_dev || !scale_dev || !shift_dev || !out_dev) return fail(PNY_ERR_ARG, "pny_trunk_conv: null argument");
    if (n < 1 || hin < 1 || win < 1 || hout < 1 || wout < 1 || !fits_int(n, hin, win) || !fits_int(n, hout, wout))
        return fail(PNY_ERR_ARG, "pny_trunk_conv: bad shape");
    if (transposed && c->cin < 32) return fail(PNY_ERR_ARG, "pny_trunk_conv: the stem has no transposed form (its input gradient is never computed)");
    // the convolution's own input and output sizes: (hin, win) -> (hout, wout) forward, the other way round transposed
    const int fh = transposed ? hout : hin, fw = transposed ? wout : win, oh = transposed ? hin : hout, ow = transposed ? win : wout;
    if (fh + 2 * c->pad < c->k || fw + 2 * c->pad < c->k || conv_out(fh, c->k, c->stride, c->pad) != oh || conv_out(fw, c->k, c->stride, c->pad) != ow)
        return fail(PNY_ERR_ARG, "pny_trunk_conv: sizes do not belong to this unit's convolution");
    hipStream_t st = (hipStream_t)stream;
    const ConvLayer fwd = conv_geometry(*c);
    ConvLayer L = transposed ? transposed_geometry(*c) : fwd;
    DevBuf scr;
    const size_t job_fl = 64;   // the one-job table in front of the packed operand
    static_assert(sizeof(TrunkPackJob) <= job_fl * sizeof(float), "job table slot");
    if (int rc = scr.reserve((job_fl + (size_t)pack_count(L) * 4) * sizeof(float), "hipMalloc(trunk stage scratch)")) return rc;
    L.w = reinterpret_cast<float*>(scr.p) + job_fl;
    L.scale = const_cast<float*>(scale_dev);
    L.shift = const_cast<float*>(shift_dev);
    const TrunkPackJob job = pack_job(fwd, L, transposed ? 1 : 0, weight_dev, L.w);
    PNY_HIP(hipMemcpy(scr.p, &job, sizeof(job), hipMemcpyHostToDevice));
    launch_trunk_pack(reinterpret_cast<const TrunkPackJob*>(scr.p), 1, job.count, st);
    PNY_HIP(hipGetLastError());
    if (!run_conv_ex(L, in_dev, n, hin, win, hout, wout, transposed ? transposed_dil_shift(fwd) : 0, resid_dev, relu ? 1 : 0, out_dev, st, variant))
        return fail(PNY_ERR_HIP, "pny_trunk_conv: convolution launch failed");
    PNY_HIP(hipStreamSynchronize(st));
    return PNY_OK;
}

int pny_trunk_conv_dw(int unit, const float* dy_dev, const float* x_dev, int n, int hin, int win, float* dw_dev, int* splits, int64_t* chunk,
                      pny_stream stream) {
    const TrunkConv* c = stage_unit(unit);
    if (!c) return fail(PNY_ERR_ARG, "pny_trunk_conv_dw: unit index out of range");
    if (!dy_dev || !x_dev || !dw_dev) return fail(PNY_ERR_ARG, "pny_trunk_conv_dw: null argument");
    if (n < 1 || hin < 1 || win < 1 || !fits_int(n, hin, win) || hin + 2 * c->pad < c->k || win + 2 * c->pad < c->k)
        return fail(PNY_ERR_ARG, "pny_trunk_conv_dw: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const ConvLayer L = conv_geometry(*c);
    const int hout = conv_out(hin, c->k, c->stride, c->pad), wout = conv_out(win, c->k, c->stride, c->pad);
    DevBuf scr;
    const size_t bytes = dw_partial_floats(L, (long long)n * hout * wout) * sizeof(float);
    if (int rc = scr.reserve(bytes, "hipMalloc(trunk stage scratch)")) return rc;
    int sp = 0;
    long long ch = 0;
    if (!launch_conv_dw(L, dy_dev, x_dev, n, hin, win, hout, wout, reinterpret_cast<float*>(scr.p), bytes, dw_dev, st, &sp, &ch))
        return fail(PNY_ERR_STATE, "pny_trunk_conv_dw: weight-gradient partials larger than planned");
    PNY_HIP(hipGetLastError());
    PNY_HIP(hipStreamSynchronize(st));
    if (splits) *splits = sp;
    if (chunk) *chunk = ch;
    return PNY_OK;
}

int pny_trunk_bn_forward(const float* y_dev, int64_t P, int C, const float* gamma_dev, const float* beta_dev, const float* resid_dev, int relu,
                         float* running_mean_dev, float* running_var_dev, float momentum, int use_running, float* out_dev, float* mean_dev,
                         float* invstd_dev, pny_stream stream) {
    if (!y_dev || !gamma_dev || !beta_dev || !out_dev || !mean_dev || !invstd_dev) return fail(PNY_ERR_ARG, "pny_trunk_bn_forward: null argument");
    if (!running_mean_dev != !running_var_dev || (use_running && !running_mean_dev))
        return fail(PNY_ERR_ARG, "pny_trunk_bn_forward: running_mean and running_var go together, and use_running needs them");
    if (!bn_channels(C) || P < 1 || P > 0x7fffffffll / C) return fail(PNY_ERR_ARG, "pny_trunk_bn_forward: C must be 64, 128 or 256 and P >= 1");
    hipStream_t st = (hipStream_t)stream;
    DevBuf scr;
    if (int rc = scr.reserve(BN_PART_FLOATS * sizeof(float), "hipMalloc(trunk stage scratch)")) return rc;
    launch_bn_forward(y_dev, P, C, gamma_dev, beta_dev, resid_dev, relu ? 1 : 0, out_dev, mean_dev, invstd_dev, running_mean_dev, running_var_dev,
                      momentum, use_running ? 1 : 0, reinterpret_cast<float*>(scr.p), st);
    PNY_HIP(hipGetLastError());
    PNY_HIP(hipStreamSynchronize(st));
    return PNY_OK;
}

int pny_trunk_bn_backward(const float* d_out_dev, const float* out_dev, const float* y_dev, const float* mean_dev, const float* invstd_dev,
                          const float* gamma_dev, int64_t P, int C, int use_running, float* dy_dev, float* g_out_dev, float* d_gamma_dev,
                          float* d_beta_dev, pny_stream stream) {
    if (!d_out_dev || !y_dev || !mean_dev || !invstd_dev || !gamma_dev || !dy_dev) return fail(PNY_ERR_ARG, "pny_trunk_bn_backward: null argument");
    if (!bn_channels(C) || P < 1 || P > 0x7fffffffll / C) return fail(PNY_ERR_ARG, "pny_trunk_bn_backward: C must be 64, 128 or 256 and P >= 1");
    hipStream_t st = (hipStream_t)stream;
    DevBuf scr;
    if (int rc = scr.reserve(BN_PART_FLOATS * sizeof(float), "hipMalloc(trunk stage scratch)")) return rc;
    launch_bn_backward(d_out_dev, out_dev, y_dev, mean_dev, invstd_dev, gamma_dev, P, C, dy_dev, g_out_dev, d_gamma_dev, d_beta_dev,
                       use_running ? 1 : 0, reinterpret_cast<float*>(scr.p), st);
    PNY_HIP(hipGetLastError());
    PNY_HIP(hipStreamSynchronize(st));
    return PNY_OK;
}

int pny_trunk_maxpool(const float* in_dev, int n, int hin, int win, int C, float* out_dev, pny_stream stream) {
    if (!in_dev || !out_dev) return fail(PNY_ERR_ARG, "pny_trunk_maxpool: null argument");
    if (!bn_channels(C) || n < 1 || hin < 1 || win < 1 || !fits_int(n, hin, (long long)win * C))
        return fail(PNY_ERR_ARG, "pny_trunk_maxpool: C must be 64, 128 or 256 and the sizes >= 1");
    launch_maxpool(in_dev, out_dev, n, hin, win, C, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_trunk_maxpool_backward(const float* in_dev, const float* g_dev, const float* add_dev, int n, int hin, int win, int C, float* d_in_dev,
                               pny_stream stream) {
    if (!in_dev || !g_dev || !d_in_dev) return fail(PNY_ERR_ARG, "pny_trunk_maxpool_backward: null argument");
    if (!bn_channels(C) || n < 1 || hin < 1 || win < 1 || !fits_int(n, hin, (long long)win * C))
        return fail(PNY_ERR_ARG, "pny_trunk_maxpool_backward: C must be 64, 128 or 256 and the sizes >= 1");
    launch_maxpool_bwd(in_dev, g_dev, add_dev, d_in_dev, n, hin, win, C, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_trunk_upsample(const float* in_dev, int n, int hin, int win, int level, int h0, int w0, float* latent_dev, pny_stream stream) {
    if (!in_dev || !latent_dev) return fail(PNY_ERR_ARG, "pny_trunk_upsample: null argument");
    if (level < 0 || level > 3 || n < 1 || hin < 1 || win < 1 || h0 < 1 || w0 < 1 || !fits_int(n, hin, (long long)win * TRUNK_LATENT) ||
        !fits_int(n, h0, (long long)w0 * TRUNK_LATENT))
        return fail(PNY_ERR_ARG, "pny_trunk_upsample: level must be 0 .. 3 and the sizes >= 1");
    launch_upsample_level(in_dev, latent_dev, n, hin, win, level, h0, w0, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_trunk_upsample_backward(const float* d_latent_dev, const float* add_dev, int n, int hin, int win, int level, int h0, int w0,
                                float* d_in_dev, pny_stream stream) {
    if (!d_latent_dev || !d_in_dev) return fail(PNY_ERR_ARG, "pny_trunk_upsample_backward: null argument");
    if (level < 0 || level > 3 || n < 1 || hin < 1 || win < 1 || h0 < 1 || w0 < 1 || !fits_int(n, hin, (long long)win * TRUNK_LATENT) ||
        !fits_int(n, h0, (long long)w0 * TRUNK_LATENT))
        return fail(PNY_ERR_ARG, "pny_trunk_upsample_backward: level must be 0 .. 3 and the sizes >= 1");
    launch_upsample_bwd(d_latent_dev, add_dev, d_in_dev, n, hin, win, level, h0, w0, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
