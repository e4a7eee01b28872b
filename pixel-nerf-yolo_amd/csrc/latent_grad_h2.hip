// The latent gradient (latent_grad.hip latent_grad_kernel) on split-f16 matrix products (x1 w1 + x2 w1 + x1 w2 on
// v_mfma_f32_32x32x16_f16, fp32 accumulation: the arithmetic of mlp_h2.hip / pixel_linear_h2_kernel), for scenes whose backward
// runs the f16x2 kernels: the GEMM is 8 launches and ~0.4 TFLOP of a training step with the encoder unfrozen.  Gradients have
// no fixed magnitude, so the B operand is multiplied by the power of two that puts the launch's max |dY| (tracked by the chain
// kernel, BwdArgs::dy_absmax) at 2^13 .. 2^14 before it is split, and the accumulators by its inverse on the way out (exact),
// as pny_dw_gemm_h2_kernel (dw_gemm_h2.hip) does.
//
// -DPNY_H2_PLANES=1 (latent_grad_h1.hip) is the latent gradient of PNY_PRECISION_F16_TRAIN, latent_grad_h1_kernel: ONE f16
// plane per operand -- the fp32 lin_z^T image rounded to f16 in registers, the scaled dY rounded to f16 in LDS, one MFMA per
// accumulator tile and 16 k instead of three.  The tiles, two-tile workgroups, inverse scale on the tap weights and
// float-atomic scatter are the same (reproducible to fp32 rounding, not bit for bit, like the other latent-gradient kernels).
// -DPNY_LG_FIXED (latent_grad_h2_det.hip, latent_grad_h1_det.hip) is the deterministic mode's build: the epilogue adds 64-bit
// fixed-point integers instead (latent_grad_fx.h).
#include "mlp_bwd_core.h"
#include "latent_grad_fx.h"

#ifndef PNY_H2_PLANES
#define PNY_H2_PLANES 2
#endif
#if PNY_H2_PLANES == 1 && defined(PNY_LG_FIXED)
#define PNY_LG_KERNEL latent_grad_h1_det_kernel
#define PNY_LG_LAUNCH launch_latent_grad_h1_det
#elif PNY_H2_PLANES == 1
#define PNY_LG_KERNEL latent_grad_h1_kernel
#define PNY_LG_LAUNCH launch_latent_grad_h1
#elif defined(PNY_LG_FIXED)
#define PNY_LG_KERNEL latent_grad_h2_det_kernel
#define PNY_LG_LAUNCH launch_latent_grad_h2_det
#else
#define PNY_LG_KERNEL latent_grad_h2_kernel
#define PNY_LG_LAUNCH launch_latent_grad_h2
#endif

namespace pny {

namespace {
constexpr int LG_KC = 32, LG_NW = 4;   // as latent_grad.hip
typedef _Float16 lgh8 __attribute__((ext_vector_type(8)));
#if PNY_H2_PLANES == 1
// two fp32 values to one f16 pair (round to nearest even)
__device__ __forceinline__ unsigned lg_cvt2(float a, float b) {
    unsigned p;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p) : "v"(a), "v"(b));
    return p;
}
#else
__device__ __forceinline__ void lg_split2(float a, float b, unsigned& p0, unsigned& p1) {
    float ra, rb;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p0) : "v"(a), "v"(b));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(p0), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(p0), "v"(b));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p1) : "v"(ra), "v"(rb));
}
#endif
}  // namespace

// TPW = 64-sample tiles per workgroup: the weights (1.5 MB of fp32 per 256 output channels at three view blocks) are what
// the kernel moves -- a workgroup with ONE tile reads them for 64 samples, 4 608 workgroups of a fine pass pull 6.9 GB through
// the L1s -- so a workgroup takes TWO consecutive tiles of its view through every weight chunk (128 accumulator registers per
// wave, 33 KB of staging): half the weight bytes per sample.  TPW = 1 is kept for launches with a single tile.
template <int TPW>
__global__ __launch_bounds__(64 * LG_NW) void PNY_LG_KERNEL(const MlpArgs a, const float* __restrict__ dy_stash, const StashLayout lay,
                                                            const float* __restrict__ w_cat, PNY_LG_OUT* __restrict__ grad, int nvb,
                                                            const unsigned* __restrict__ dy_absmax PNY_LG_FX_ARG) {
    PNY_LG_FX_LOAD
    constexpr int TS = 64 * TPW, MT = 2 * TPW;      // samples and 32-sample m-tiles of the workgroup
    __shared__ uint2 bp[2][PNY_H2_PLANES][LG_KC / 4][TS + 1];   // [buffer][plane][k / 4][sample]
    __shared__ __attribute__((aligned(16))) float tr[LG_NW][32][68];
    __shared__ int tap_off[TS][4];
    __shared__ float tap_w[TS][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = lane & 31, hh = lane >> 5;
    const int nblocks = a.L / 256;
    const int nb = blockIdx.x % nblocks;
    const long long tv = blockIdx.x / nblocks;
    const int v = (int)(tv % a.NS);
    const long long tile0 = (tv / a.NS) * TPW;
    const int K = nvb * HID, J = K / 8;
    float scale, inv_scale;
    pow2_scale(*dy_absmax, 13, &scale, &inv_scale);
    // tile t of the workgroup (the last workgroup of a view may hold a single live tile: the dead one re-reads the live
    // tile's stash and scatters with weight 0)
    long long tile_of[TPW];
    int vabs_of[TPW];   // index into the scene's view list (grouped scenes: two tiles may belong to two objects)
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        tile_of[t] = tile0 + t < a.n_tiles ? tile0 + t : tile0;
        vabs_of[t] = tile_view_base(a, tile_of[t] * 64) + v;
    }
    if (tid < TS) {
        const int t = tid >> 6;
        long long s = tile_of[t] * 64 + (tid & 63);
        int offs[4];
        float wgt[4];
        const bool live = (tile0 + t < a.n_tiles) && s < a.n_points;
        if (s >= a.n_points) s = a.n_points - 1;
        sample_taps(a, vabs_of[t], s, offs, wgt);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tap_off[tid][k] = offs[k];
            tap_w[tid][k] = live ? wgt[k] * inv_scale : 0.0f;   // the inverse scale rides on the tap weight
        }
    }
    const float* dy_rec[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) dy_rec[t] = lay.dy_record(dy_stash, tile_of[t]);
    auto stage_load = [&](int c, float4 (&sv)[TPW][2]) {
        const int b = c / (HID / LG_KC), kg0 = (c % (HID / LG_KC)) * (LG_KC / 4);
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const float4* src = reinterpret_cast<const float4*>(dy_rec[t] + lay.dy_dh(v, b)) + (size_t)kg0 * 64;
            sv[t][0] = src[tid];
            sv[t][1] = src[tid + 256];
        }
    };
    auto stage_store = [&](int buf, const float4 (&sv)[TPW][2]) {
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#if PNY_H2_PLANES == 1
                bp[buf][0][4 * h + (tid >> 6)][64 * t + (tid & 63)] =
                    make_uint2(lg_cvt2(sv[t][h].x * scale, sv[t][h].y * scale), lg_cvt2(sv[t][h].z * scale, sv[t][h].w * scale));
#else
                uint2 q0, q1;
                lg_split2(sv[t][h].x * scale, sv[t][h].y * scale, q0.x, q1.x);
                lg_split2(sv[t][h].z * scale, sv[t][h].w * scale, q0.y, q1.y);
                bp[buf][0][4 * h + (tid >> 6)][64 * t + (tid & 63)] = q0;
                bp[buf][1][4 * h + (tid >> 6)][64 * t + (tid & 63)] = q1;
#endif
            }
    };
    f32x16 acc[2][MT];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][mt][r] = 0.f;
    const int nt0 = nb * 8 + wave * 2;
    const float4* wp = reinterpret_cast<const float4*>(w_cat) + (size_t)nt0 * J * 64 + lane;
    const int nchunks = K / LG_KC;
    float4 sv[TPW][2];
    stage_load(0, sv);
    stage_store(0, sv);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) stage_load(c + 1, sv);
        // (fetching the fragments of chunk c + 1 while chunk c multiplies was measured: 32 more registers, 1.17 against 1.13 ms
        // per launch -- the exposed L2 latency at the head of a chunk is covered by the other workgroup of the CU)
        float4 wa[LG_KC / 8][2];
#pragma unroll
        for (int j = 0; j < LG_KC / 8; ++j)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) wa[j][nt] = wp[((size_t)nt * J + (size_t)c * (LG_KC / 8) + j) * 64];
#pragma unroll
        for (int st_ = 0; st_ < LG_KC / 16; ++st_) {
            // a 16-k step: the lane's own two float4 of the fp32 weight image (k = 16 s + 4 hh + 0..3 and 16 s + 8 + 4 hh + 0..3:
            // which 8 k a fragment holds is free as long as both operands agree), split (or rounded to one plane) in registers
#if PNY_H2_PLANES == 1
            lgh8 a1[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                a1[nt] = __builtin_bit_cast(lgh8, make_uint4(lg_cvt2(wa[2 * st_][nt].x, wa[2 * st_][nt].y),
                                                             lg_cvt2(wa[2 * st_][nt].z, wa[2 * st_][nt].w),
                                                             lg_cvt2(wa[2 * st_ + 1][nt].x, wa[2 * st_ + 1][nt].y),
                                                             lg_cvt2(wa[2 * st_ + 1][nt].z, wa[2 * st_ + 1][nt].w)));
#else
            lgh8 a1[2], a2[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                uint4 u1, u2;
                lg_split2(wa[2 * st_][nt].x, wa[2 * st_][nt].y, u1.x, u2.x);
                lg_split2(wa[2 * st_][nt].z, wa[2 * st_][nt].w, u1.y, u2.y);
                lg_split2(wa[2 * st_ + 1][nt].x, wa[2 * st_ + 1][nt].y, u1.z, u2.z);
                lg_split2(wa[2 * st_ + 1][nt].z, wa[2 * st_ + 1][nt].w, u1.w, u2.w);
                a1[nt] = __builtin_bit_cast(lgh8, u1);
                a2[nt] = __builtin_bit_cast(lgh8, u2);
            }
#endif
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const uint2 l1 = bp[buf][0][4 * st_ + hh][32 * mt + m0], h1 = bp[buf][0][4 * st_ + 2 + hh][32 * mt + m0];
                const lgh8 b1 = __builtin_bit_cast(lgh8, make_uint4(l1.x, l1.y, h1.x, h1.y));
#if PNY_H2_PLANES == 2
                const uint2 l2 = bp[buf][1][4 * st_ + hh][32 * mt + m0], h2 = bp[buf][1][4 * st_ + 2 + hh][32 * mt + m0];
                const lgh8 b2 = __builtin_bit_cast(lgh8, make_uint4(l2.x, l2.y, h2.x, h2.y));
#endif
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[nt], b1, acc[nt][mt], 0, 0, 0);
#if PNY_H2_PLANES == 2
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2[nt], b1, acc[nt][mt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[nt], b2, acc[nt][mt], 0, 0, 0);
#endif
            }
        }
        if (c + 1 < nchunks) {
            stage_store(buf ^ 1, sv);
            __syncthreads();
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        PNY_LG_OUT* gv = grad + (size_t)vabs_of[mt >> 1] * a.Hl * a.Wl * a.L + 32 * nt0 + lane;
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 t;
                t.x = acc[nt][mt][4 * q + 0];
                t.y = acc[nt][mt][4 * q + 1];
                t.z = acc[nt][mt][4 * q + 2];
                t.w = acc[nt][mt][4 * q + 3];
                *reinterpret_cast<float4*>(&tr[wave][m0][32 * nt + 8 * q + 4 * hh]) = t;
            }
        __syncthreads();
        for (int m = 0; m < 32; ++m) {
            const float val = tr[wave][m][lane];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float wk = tap_w[32 * mt + m][k];
                if (wk != 0.0f) PNY_LG_ADD(gv + tap_off[32 * mt + m][k], wk * val);
            }
        }
    }
}

// launch_latent_grad's share (latent_grad.hip) for this plane count (PNY_LG_FIXED: launch_latent_grad_det's, latent_grad_det.hip)
void PNY_LG_LAUNCH(const MlpArgs& a, const float* dy_stash, const StashLayout& lay, const float* w_cat, PNY_LG_OUT* grad, int nvb,
                   hipStream_t st, const unsigned* dy_absmax PNY_LG_FX_ARG) {
    if (a.n_tiles >= 2) {
        const long long pairs = (long long)((a.n_tiles + 1) / 2) * a.NS * (a.L / 256);
        hipLaunchKernelGGL(PNY_LG_KERNEL<2>, dim3((unsigned)pairs), dim3(64 * LG_NW), 0, st, a, dy_stash, lay, w_cat, grad, nvb, dy_absmax PNY_LG_FX_PASS);
    } else {
        const long long blocks = (long long)a.n_tiles * a.NS * (a.L / 256);
        hipLaunchKernelGGL(PNY_LG_KERNEL<1>, dim3((unsigned)blocks), dim3(64 * LG_NW), 0, st, a, dy_stash, lay, w_cat, grad, nvb, dy_absmax PNY_LG_FX_PASS);
    }
}

}  // namespace pny
