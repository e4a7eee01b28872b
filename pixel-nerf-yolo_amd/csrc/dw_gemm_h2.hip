// The weight-gradient GEMM of pny_dw_gemm_kernel (mlp_bwd.hip) on the f16 matrix cores with split fp32 operands (the arithmetic
// of mlp_h2.hip: x = x1 + x2 in two f16 planes, x1 y1 + x2 y1 + x1 y2 on v_mfma_f32_32x32x16_f16 with fp32 accumulation; 5.3x
// the matrix rate of the fp32 MFMA).  Clipped tiles (lin_in's 64 columns, lin_out's 64 rows) run a predicated instantiation, as
// in the fp32 kernel.
//   * The contraction runs over SAMPLES, and an f16 fragment holds 8 consecutive k of one row: a staging thread loads, for one
//     feature quad, the 8 samples {c, c + 4, ..., c + 28} of a 32-sample half (lanes c = 0..3 adjacent: 64-byte segments),
//     i.e. an 8 x 4 block in registers, and writes per feature ONE 16-byte vector per plane -- the transpose happens in
//     registers.  Which 8 samples share a fragment is irrelevant as long as both operands agree (k is a dummy index).
//   * LDS image per operand and plane: [c = 0..3][feature 0..255 (+1 pad)] x 16 bytes; a fragment read is 32 consecutive
//     features of one c: 512 contiguous bytes.  Two buffers of (A, X) x 2 planes = 128.5 KiB, one barrier per half.
//   * Gradients span many orders of magnitude and f16 does not: dY is multiplied by a power of two that puts the launch's
//     max |dY| (tracked by the chain kernel, BwdArgs::dy_absmax) at 2^13..2^14, and the accumulators are multiplied by its
//     inverse on the way out -- exact.  Elements down to 2^-27 of the maximum keep all 22 bits, smaller ones an absolute
//     2^-38 of the maximum.
//   * Bias gradients (column sums of dY) are taken by the staging threads from the fp32 values.
//
// -DPNY_H2_PLANES=1 (dw_gemm_h1.hip) is the weight-gradient GEMM of PNY_PRECISION_F16_TRAIN, pny_dw_gemm_h1_kernel: both
// operands rounded to ONE f16 plane (dY after the same power-of-two scale, so elements down to 2^-27 of the maximum stay
// normal f16; X the fp32 stash as it is), one MFMA per product and 16 samples instead of three, fp32 accumulation.  The work
// items, split-K partial tiles (train_api.hip build_items), fp32 bias sums and deterministic reduction (pny_dw_reduce_kernel)
// are the same; the LDS images have one plane: two buffers = 64.25 KiB.
#include "mlp_bwd_core.h"

#ifndef PNY_H2_PLANES
#define PNY_H2_PLANES 2
#endif
#if PNY_H2_PLANES == 1
#define PNY_DWG_KERNEL pny_dw_gemm_h1_kernel
#define PNY_DWG_LAUNCH launch_dw_gemm_h1
#else
#define PNY_DWG_KERNEL pny_dw_gemm_h2_kernel
#define PNY_DWG_LAUNCH launch_dw_gemm_h2
#endif

namespace pny {

namespace {
typedef _Float16 dwh8 __attribute__((ext_vector_type(8)));
constexpr int DWH_TILE = 256;                                         // output tile (as mlp_bwd.hip DW_TILE)
constexpr int DWH_CS = 257;                                           // 16-byte entries per c row (256 features + 1 pad)
constexpr int DWH_PLANE = 4 * DWH_CS;                                 // entries per plane
constexpr int DWH_BUF = 2 * PNY_H2_PLANES * DWH_PLANE;                // entries per buffer: (A, X) x planes
constexpr size_t DWH_LDS_BYTES = (size_t)2 * DWH_BUF * 16;            // 131584 (two planes), 65792 (one)

#if PNY_H2_PLANES == 1
// two fp32 values to one f16 pair (round to nearest even)
__device__ __forceinline__ unsigned dwh_cvt2(float a, float b) {
    unsigned p;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p) : "v"(a), "v"(b));
    return p;
}
#else
__device__ __forceinline__ void dwh_split2(float a, float b, unsigned& p0, unsigned& p1) {
    float ra, rb;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p0) : "v"(a), "v"(b));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(p0), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(p0), "v"(b));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p1) : "v"(ra), "v"(rb));
}
#endif
}  // namespace

template <bool FULL>   // FULL: complete 256 x 256 tiles, predicate-free; otherwise rows / columns beyond the job are zero-filled and skipped
__global__ __launch_bounds__(512, 2) void PNY_DWG_KERNEL(const DwJob* __restrict__ jobs, const DwItem* __restrict__ items,
                                                         const float* __restrict__ x_stash,
                                                         const float* __restrict__ dy_stash, long long x_tile,
                                                         long long dy_tile, float* __restrict__ partial,
                                                         float* __restrict__ bias_partial,
                                                         const unsigned* __restrict__ dy_absmax) {
    extern __shared__ __attribute__((aligned(16))) float dw_lds[];
    uint4* lds = reinterpret_cast<uint4*>(dw_lds);
    const DwItem it = items[blockIdx.x];
    const DwJob jb = jobs[it.job];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3, hh = lane >> 5, l31 = lane & 31;
    const int row0 = it.mt * DWH_TILE, col0 = it.nt * DWH_TILE;

    // scale = 2^(13 - floor(log2(max |dY|))), clamped to the normal range
    float scale, inv_scale;
    pow2_scale(*dy_absmax, 13, &scale, &inv_scale);

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // staging role of this thread: operand (waves 0..3: A = dY, waves 4..7: X), feature quad fq of the tile, sample group c
    const int op = wave >> 2;
    const int fq = (tid & 255) >> 2, c = tid & 3;
    const float sc = op == 0 ? scale : 1.0f;
    const bool want_bias = op == 0 && it.nt == 0;
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    float4 r[8];
    // clipped tiles: quads beyond the job's extent load nothing (zeros); quads beyond the last 32-wide MFMA tile that holds
    // live data are not even written
    const int extent = op == 0 ? jb.a_rows - row0 : jb.x_cols - col0;
    const bool q_load = FULL || 4 * fq < extent, q_write = FULL || 4 * fq < ((extent + 31) & ~31);
    bool live_a[4], live_x[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) live_a[i] = FULL || row0 + wr * 128 + 32 * i < jb.a_rows;
#pragma unroll
    for (int j = 0; j < 2; ++j) live_x[j] = FULL || col0 + wc * 64 + 32 * j < jb.x_cols;
    auto fetch = [&](int h) {
        const int tv = it.tv_lo + (h >> 1), half = h & 1;
        const int tile = tv / jb.n_views, v = tv - tile * jb.n_views;
        const float* rec = op == 0 ? stash_record(dy_stash, dy_tile, tile) + jb.a_off + (long long)v * jb.a_view
                                   : stash_record(x_stash, x_tile, tile) + jb.x_off + (long long)v * jb.x_view;
        const float4* g = reinterpret_cast<const float4*>(rec) + ((op == 0 ? row0 : col0) / 4 + fq) * 64 + 32 * half + c;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = q_load ? g[4 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto stage = [&](int b) {
        uint4* img = lds + b * DWH_BUF + op * (PNY_H2_PLANES * DWH_PLANE) + c * DWH_CS + 4 * fq;
        if (!q_write) return;
        if (want_bias) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {   // (asm: keeps the SLP vectoriser from packing these into v_pk_add_f32 beside the MFMAs)
                asm("v_add_f32 %0, %1, %0" : "+v"(bs[0]) : "v"(r[i].x));
                asm("v_add_f32 %0, %1, %0" : "+v"(bs[1]) : "v"(r[i].y));
                asm("v_add_f32 %0, %1, %0" : "+v"(bs[2]) : "v"(r[i].z));
                asm("v_add_f32 %0, %1, %0" : "+v"(bs[3]) : "v"(r[i].w));
            }
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (f == 0 ? r[i].x : f == 1 ? r[i].y : f == 2 ? r[i].z : r[i].w) * sc;
#if PNY_H2_PLANES == 1
            img[f] = make_uint4(dwh_cvt2(v[0], v[1]), dwh_cvt2(v[2], v[3]), dwh_cvt2(v[4], v[5]), dwh_cvt2(v[6], v[7]));
#else
            uint4 p0, p1;
            dwh_split2(v[0], v[1], p0.x, p1.x);
            dwh_split2(v[2], v[3], p0.y, p1.y);
            dwh_split2(v[4], v[5], p0.z, p1.z);
            dwh_split2(v[6], v[7], p0.w, p1.w);
            img[f] = p0;
            img[DWH_PLANE + f] = p1;
#endif
        }
    };
    const int n_half = 2 * (it.tv_hi - it.tv_lo);
    if (n_half > 0) {
        fetch(0);
        stage(0);
        if (n_half > 1) fetch(1);
        __syncthreads();
    }
    auto mm = [&](int cb) {   // the MFMAs of one half on buffer cb
        const uint4* pa = lds + cb * DWH_BUF + hh * DWH_CS + wr * 128 + l31;
        const uint4* px = lds + cb * DWH_BUF + PNY_H2_PLANES * DWH_PLANE + hh * DWH_CS + wc * 64 + l31;
#pragma unroll
        for (int st = 0; st < 2; ++st) {       // 16 samples per step: this lane's 8 are group c = 2 st + hh
#if PNY_H2_PLANES == 1
            dwh8 a1[4] = {}, x1[2] = {};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (FULL || live_a[i]) a1[i] = __builtin_bit_cast(dwh8, pa[2 * st * DWH_CS + 32 * i]);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (FULL || live_x[j]) x1[j] = __builtin_bit_cast(dwh8, px[2 * st * DWH_CS + 32 * j]);
#else
            dwh8 a1[4] = {}, a2[4] = {}, x1[2] = {}, x2[2] = {};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (FULL || live_a[i]) {
                    a1[i] = __builtin_bit_cast(dwh8, pa[2 * st * DWH_CS + 32 * i]);
                    a2[i] = __builtin_bit_cast(dwh8, pa[DWH_PLANE + 2 * st * DWH_CS + 32 * i]);
                }
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (FULL || live_x[j]) {
                    x1[j] = __builtin_bit_cast(dwh8, px[2 * st * DWH_CS + 32 * j]);
                    x2[j] = __builtin_bit_cast(dwh8, px[DWH_PLANE + 2 * st * DWH_CS + 32 * j]);
                }
#endif
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (FULL || (live_a[i] && live_x[j])) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[i], x1[j], acc[i][j], 0, 0, 0);
#if PNY_H2_PLANES == 2
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (FULL || (live_a[i] && live_x[j])) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2[i], x1[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (FULL || (live_a[i] && live_x[j])) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[i], x2[j], acc[i][j], 0, 0, 0);
#endif
        }
    };
    for (int h = 0; h < n_half; ++h) {
        const int cb = h & 1;
        if (h + 1 < n_half) {
            stage(cb ^ 1);                     // half h + 1: every wave left that buffer at the previous barrier
            if (h + 2 < n_half) fetch(h + 2);
        }
        mm(cb);
        __syncthreads();
    }
    float* P = partial + it.part_off;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!FULL && !(live_a[i] && live_x[j])) continue;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int row = row0 + wr * 128 + 32 * i + 8 * (rr >> 2) + 4 * hh + (rr & 3);
                const int col = col0 + wc * 64 + 32 * j + l31;
                if (FULL || (row < jb.a_rows && col < jb.x_cols)) P[(long long)row * jb.x_cols + col] = acc[i][j][rr] * inv_scale;
            }
        }
    if (want_bias) {   // the four lanes c = 0..3 of a feature quad hold the sums of their own samples
        float* B = bias_partial + it.bias_off;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            float t = bs[f];
            t += __shfl_xor(t, 1, 64);
            t += __shfl_xor(t, 2, 64);
            if (c == 0 && (FULL || row0 + 4 * fq + f < jb.a_rows)) B[row0 + 4 * fq + f] = t;
        }
    }
}

// launch_dw_gemm's share (mlp_bwd.hip) for this plane count: n_part clipped items first on `sp`, n_full complete tiles on `st`
void PNY_DWG_LAUNCH(const DwJob* jobs_dev, const DwItem* items_dev, int n_part, int n_full, const float* x_stash,
                    const float* dy_stash, long long x_tile, long long dy_tile, float* partial, float* bias_partial, hipStream_t st,
                    hipStream_t sp, const unsigned* dy_absmax) {
    static LdsLimit lds;
    (void)lds.raise(DWH_LDS_BYTES, PNY_DWG_KERNEL<true>, PNY_DWG_KERNEL<false>);
    if (n_part > 0)
        hipLaunchKernelGGL(PNY_DWG_KERNEL<false>, dim3(n_part), dim3(512), DWH_LDS_BYTES, sp, jobs_dev, items_dev, x_stash, dy_stash,
                           x_tile, dy_tile, partial, bias_partial, dy_absmax);
    if (n_full > 0)
        hipLaunchKernelGGL(PNY_DWG_KERNEL<true>, dim3(n_full), dim3(512), DWH_LDS_BYTES, st, jobs_dev, items_dev + n_part, x_stash,
                           dy_stash, x_tile, dy_tile, partial, bias_partial, dy_absmax);
}

}  // namespace pny
