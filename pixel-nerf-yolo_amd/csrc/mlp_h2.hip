// The fused conditioned-MLP kernel on the f16 matrix cores with SPLIT fp32 operands (gfx950, MI355X).
//
// fp32 = two f16 planes: x1 = f16(x) (round to nearest), x2 = f16(x - x1): 22 significant bits, and because f16 denormals are
// honoured the second plane keeps an ABSOLUTE precision of 2^-25 for |x| < 0.25 -- measured on the ResnetFC's magnitudes
// (tools/ubench/split_f16_check.hip, K = 512): max |error| against fp64 of
//     x1 w1 + x1 w2 + x2 w1   (three v_mfma_f32_32x32x16_f16 per 16 k, fp32 accumulation)          1.69e-6
//     v_mfma_f32_32x32x2_f32 (the exact-fp32 path of mlp.hip)                                       1.79e-6
// i.e. the same error as the fp32 matrix path, at 3 x 32 cycles per 16 k instead of 8 x 64: 5.3x the matrix rate.
// The 1e-4 parity bar is held by the same golden vectors (tests run this kernel under PNYOLO_MLP_PRECISION=f16x2).
//
// Same structure as pny_mlp_kernel<Cfg<2,2>, ZP = true> (mlp.hip): 8 waves, 64 samples x 512 features per workgroup, wave w owns
// features [64 w, 64 w + 64) (2 x 2 accumulator tiles of 32 x 32), the residual stream in the accumulators, persistent over
// tiles, weights as one stream per wave through a static-slot register ring across layer boundaries, projected-latent
// variant only (lin_z applied per latent pixel once per scene).  What changes:
//   * the LDS activation buffer holds the two f16 planes of relu(.), [k/8][plane][sample] x 16 bytes (same 128 KiB); a B
//     fragment of a 16-k step is one ds_read_b128 per plane; the epilogue splits in registers and writes 8 bytes per plane
//     and accumulator quad;
//   * weights are packed per 16-k step as [n-tile][plane][lane] x 16 bytes (4 bytes per weight, as before);
//   * the block entry is WAVE-OWNED (h2wave_entry; every non-stashing instantiation: pny_mlp_h2_kernel<false>,
//     pny_mlp_h2s_kernel, pny_mlp_h1_kernel<false>): the accumulator layout gives a lane four consecutive features of one
//     sample, one float4 of the projected map, so wave w gathers ITS OWN features -- the 256 contiguous bytes per latent pixel
//     that its rows hold -- for all samples of the tile, an accumulator tile (32 features x 32 samples) at a time, two in
//     flight.  A wave load still covers 8 consecutive samples x one 128-byte line.  The blend is staged in fp32 in the
//     tile's own plane bytes (feature quad j of sample s in the quad's slot at column s ^ j: 16 bytes per lane and free of
//     bank conflicts on both sides), read back in accumulator layout and turned into planes by the same wave: bias, projection,
//     relu, range guard and split run per tile inside the gather's software pipeline, while the next tile's loads are in
//     flight, and between the barrier behind the previous GEMM and the one in front of fc_0 there is no workgroup barrier.
//     The first tile of the next block is fetched underneath the fc_1 GEMM (in the registers of the then-dead `net`
//     accumulators).  A lane serves four samples per tile: tap offsets and weights are re-read from the LDS tap table,
//     and the loads go through a buffer resource of the view's map with 32-bit byte offsets (render_api.hip wants_projection keeps
//     a view's map under 4 GiB).
//     The STASH instantiations (training forwards) keep the SHARED entry: the projected channels of a block arrive in 4
//     chunks of 128 through two register buffers, wave w fetching samples 8 w .. 8 w + 7 for all 128 channels of a chunk
//     (first chunk of the next block underneath the fc_1 GEMM), staged in fp32 in the bytes the consumer lane later overwrites
//     (the first two floats of a feature quad in the quad's plane-0 slot, the other two in its plane-1 slot), a workgroup
//     barrier, then h2epilogue<true>.  With the wave-owned entry pny_mlp_h2_kernel<true> spills 198 VGPRs instead of 185, and
//     these kernels also gather the raw latent in the shared lane mapping.  Same blends, same sums in the same order: the
//     two entries give the same bits;
//   * biases are applied lazily in the epilogue that follows (b_in + b_z0 and b_fc1[b-1] + b_z[b] at the next block entry,
//     b_fc0 in the relu(net) epilogue, the last b_fc1 before lin_out) from a table in the remaining LDS (22 KiB for 5 blocks;
//     152 of the CU's 160 KiB in use): no bias registers, no global loads between a barrier and a GEMM.  (mean over views
//     of (h_v + b) = mean(h_v) + b, so the last per-view bias may follow the mean.)
//   * lin_out runs on the matrix cores as well (every two-plane instantiation; h2linout_product / h2linout_reduce below):
//     W_out is one more split-f16 image (pack.hip PACK_H2O, d_out rows padded with zero rows to one or two n-tiles), wave w
//     multiplies the k-steps of its own features with the planes it has just written in the last epilogue -- wave-level
//     ordering, no workgroup barrier -- into one fp32 partial per 64-k chunk, the partials go to the wave's own plane rows,
//     and behind ONE barrier they are added in chunk order, + b_out, output head, store (16 bytes per sample at d_out = 4).
//     24 MFMAs per wave and tile at d_out <= 32, where 256 of the 512 threads ran 64 x 512 scalar fp32 FMAs each on converted
//     planes before.  Both shapes add the same products in the same order (a wave of the 32-sample shape keeps its two chunks
//     apart), so they still agree bit for bit, and a result still does not depend on the batch.  The single-plane kernel keeps
//     the fp32 dot products on w_out as stored: its tests sit close to their bars (profiles/view_mean_fc1.md);
//   * stash / slab traffic goes through raw buffer resources (one VGPR of lane offset instead of per-quad 64-bit pointers);
//   * the VIEW-MEAN order (the non-stashing two-plane instantiations, pny_mlp_h2_kernel<false> and pny_mlp_h2s_kernel): the
//     last per-view block ends `h_v += fc_1(R_v)`, R_v =
//     relu(net_v + b_fc0), directly followed by the mean over views, and fc_1 is linear, so
//         mean_v(h_v + fc_1(R_v)) = mean_v(h_v) + fc_1(mean_v R_v):
//     that block's fc_1 GEMM runs ONCE per sample instead of once per view (20 instead of 22 full GEMMs per 3-view tile).
//     Every view but the last stops behind the block's fc_0 GEMM: in registers net = relu(net + b_fc0), the running sums of
//     the earlier views are added to net and to h from two lane-private slabs (the h slab and, behind the h slabs of the
//     whole grid, a second one of the same layout for R) and stored back; nothing goes to the planes, no barrier, and the
//     fc_0 GEMM leaves the weight ring primed for the next view's lin_in.  The last view writes the planes of net / NS (the
//     epilogues' split and f16-range guard), scales h by 1 / NS and runs the one fc_1 GEMM.  One path: a single view takes
//     it with 1 / NS = 1, which is exact.  One fp32 sum per sample is reordered (the sqrt(NS) averaging of that one layer's
//     rounding error is lost); a result still does not depend on the batch a point is rendered in.
//     -DPNY_H2_PER_VIEW_FC1 (diagnostic builds only, tools/h2_variant_build.sh) keeps the per-view order for an A/B.
// STASH = true is the training forward (the backward's operand stash written from prologue and epilogues); it keeps the
// per-view order: the backward and the stash layout consume relu(net_v) of every view.  The single-plane kernel below keeps
// it too: its no-grad kernel is also the training forward of an F16_TRAIN scene whose stash has no room, and with the view-mean
// order there tests/test_gpu_f16_train.py test_recompute_in_chunks_deterministic measures 2.94e-3 against its 2.6e-3 bar
// (1.28e-3 in the per-view order).
// This file is compiled with -fno-slp-vectorize (csrc/Makefile).  Phase timing: -DPNY_H2_STAMP
// (tools/h2_variant_build.sh).
//
// -DPNY_H2_PLANES=1 (mlp_h1.hip) is the single-plane kernel of PNY_PRECISION_F16: x = f16(x), w = f16(w), one
// v_mfma_f32_32x32x16_f16 per accumulator tile and 16 k (fp32 accumulation), weights packed per 16-k step as
// [n-tile][lane] x 16 bytes (2 bytes per weight; model_api.hip build_h1_images).  The LDS layout stays the one above: relu(.) goes to
// plane slot 0 only, and slot 1 keeps its one job of staging half of the block entry's fp32 projection -- the projection
// is added in fp32 exactly as in the two-plane kernel, at the same 152 KiB of LDS.  Its STASH instantiation is the training
// forward of PNY_PRECISION_F16_TRAIN: the stash layout is unchanged and holds this kernel's own fp32 values.
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <vector>

#include "mlp_bwd_core.h"
#include "mlp_h2_core.h"

// The same source is the SPLIT shape's translation unit (mlp_h2s.hip: -DPNY_H2_SPLIT with PNY_H2_NT = 4, PNY_H2_MT = 1;
// mlp_h2_core.h): 4 waves, 32-sample tiles, 65 KiB of LDS and two workgroups per CU; render only (no STASH instantiation: the
// backward's stash is laid out on 64-sample tiles), biases read from global memory instead of an LDS table.
#if PNY_H2_PLANES == 1
#define PNY_H2_KERNEL pny_mlp_h1_kernel
#elif defined(PNY_H2_SPLIT)
#define PNY_H2_KERNEL pny_mlp_h2s_kernel
#else
#define PNY_H2_KERNEL pny_mlp_h2_kernel
#endif

namespace pny {

// Diagnostic build only (-DPNY_H2_STAMP): s_memtime brackets around the phases of a tile, summed per wave and printed by
// launch_mlp_h2.  No stamp executes in the product build.
#ifdef PNY_H2_STAMP
enum { HS_TOTAL = 0, HS_GEMM, HS_GATHER_WAIT, HS_GATHER, HS_EPI_WAIT, HS_EPI, HS_PROLOGUE, HS_LINOUT, HS_SLAB, HS_REAL, HS_N };
__device__ unsigned long long* g_h2_stamp_buf;
__device__ __forceinline__ unsigned long long h2now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define HS_T0() hs_t_ = h2now()
#define HS_LAP(cat)                         \
    {                                       \
        const unsigned long long n_ = h2now(); \
        hs_acc[cat] += n_ - hs_t_;          \
        hs_t_ = n_;                         \
    }
#else
#define HS_T0()
#define HS_LAP(cat)
#endif

// The 8-byte slot of feature quad (row, half) = (feature / 8, (feature / 4) & 1) of sample m in plane p is at byte
//     (2 row + p) * ROW_BYTES + 16 m + 8 half.

// GEMM epilogue, and with ADDZ the second half of the SHARED block entry (STASH instantiations; the others enter a block through
// h2wave_entry below): acc += bias (+ the staged fp32 projection, ADDZ), then the planes of relu(acc) go to the
// slots of the lane's own feature quads -- the bytes the staged projection was read from, so no other lane's data is touched.
// `bias`: a 512-float vector of the workgroup's LDS bias table.
// Stores into the tile's record of the X stash go through a raw buffer resource with 32-bit offsets (64-bit pointers per
// accumulator quad cost 32 address registers per epilogue).  The whole offset travels in the VGPR, the scalar offset stays
// the constant 0: a buffer store of more than 64 bits needs ONE wait state before a VALU write of its data registers, LLVM's
// hazard recogniser inserts it only when soffset is not a register, and gfx950 needs it with an SGPR soffset too -- with the
// slot offset in an SGPR the compiler put the next write of the first data register directly behind 8 of these stores (the
// x_in and z operands) and ~20 % of them carried the NEW value in dword 0 (lin_in / lin_z weight gradients off by 1-9 %, in
// exactly the `.x` columns).  One `s_nop 0` behind the store cures that form (profiles/r03_anomalies.md B;
// tools/check_store_hazard.py guards the built library against the pattern).
__device__ __forceinline__ void stash_store(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, float a, float b, float c, float d) {
    const f32x4 v = {a, b, c, d};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc, voff + soff, 0, 0);
}

// put_planes (mlp_h2_core.h) with the running maximum of the f16-range guard (include/pnyolo.h pny_model_range_status): a
// value >= 65520 rounds to an f16 infinity.  SIGNED: the values may be negative (lin_in's inputs); relu outputs are compared
// as they are (two v_max3_f32 per quad).
template <bool SIGNED = false>
__device__ __forceinline__ void h2put_planes(char* slot, float r0, float r1, float r2, float r3, float& rmax) {
    if constexpr (SIGNED)
        rmax = fmaxf(fmaxf(rmax, fmaxf(fabsf(r0), fabsf(r1))), fmaxf(fabsf(r2), fabsf(r3)));
    else
        rmax = fmaxf(fmaxf(rmax, fmaxf(r0, r1)), fmaxf(r2, r3));
    put_planes(slot, r0, r1, r2, r3);
}
// ... and the guard's tail: one branch per call site, the maximum local to the call (a register kept across the GEMM loops
// costs spills there: 60 -> 169 spilled VGPRs when it was a kernel-wide running maximum)
__device__ __forceinline__ void range_check(float rmax, unsigned* range_flag) {
    if (__builtin_expect(!(rmax < 65520.0f), 0)) range_report(range_flag, 1u);
}

// STASH (training forward): relu(acc + ...) is also written in fp32 to `stash` in the [feature/4][sample] float4 tile layout of
// the backward's operand stash (stash.h; the same values the fp32 STASH kernel of mlp.hip writes).
template <bool ADDZ, bool STASH = false>
__device__ __forceinline__ void h2epilogue(f32x16 (&acc)[h2::NT][h2::MT], const float* bias, char* planes, int wave, int lane, unsigned* range_flag,
                                           __amdgpu_buffer_rsrc_t stash = __amdgpu_buffer_rsrc_t(), unsigned stash_off = 0) {
    using namespace h2;
    const unsigned stash_lane = (unsigned)(((8 * NT * wave + (lane >> 5)) * TM + (lane & 31)) * 16);
    const int m0 = lane & 31, hh = lane >> 5;
    const float* bl = bias + 32 * NT * wave + 4 * hh;
    float rmax = 0.f;   // f16-range guard: the largest value this call hands to the planes
    // accumulator quad (nt, q) of this lane = features 32 NT wave + 32 nt + 8 q + 4 hh + 0..3: row 4 NT wave + 4 nt + q, half hh
    char* base = planes + (4 * NT * wave) * (2 * ROW_BYTES) + m0 * 16 + 8 * hh;
    // the LDS reads of a (nt, mt) tile -- bias quads, staged projection -- are issued together ahead of its arithmetic
    // (left to itself the compiler reads, waits and converts quad by quad: 16 exposed LDS latencies per epilogue)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float4 b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const float4*>(bl + 32 * nt + 8 * q);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            float2 za[4], zb[4];
            if (ADDZ) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const char* s0 = base + (4 * nt + q) * (2 * ROW_BYTES) + 32 * mt * 16;
                    za[q] = *reinterpret_cast<const float2*>(s0);
                    zb[q] = *reinterpret_cast<const float2*>(s0 + ROW_BYTES);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                char* s0 = base + (4 * nt + q) * (2 * ROW_BYTES) + 32 * mt * 16;
                float x0 = acc[nt][mt][4 * q + 0] + b[q].x, x1 = acc[nt][mt][4 * q + 1] + b[q].y;
                float x2 = acc[nt][mt][4 * q + 2] + b[q].z, x3 = acc[nt][mt][4 * q + 3] + b[q].w;
                if (ADDZ) {
                    x0 += za[q].x;
                    x1 += za[q].y;
                    x2 += zb[q].x;
                    x3 += zb[q].y;
                }
                acc[nt][mt][4 * q + 0] = x0;
                acc[nt][mt][4 * q + 1] = x1;
                acc[nt][mt][4 * q + 2] = x2;
                acc[nt][mt][4 * q + 3] = x3;
                const float r0 = relu1(x0), r1 = relu1(x1), r2 = relu1(x2), r3 = relu1(x3);
                if constexpr (STASH) stash_store(stash, stash_lane, stash_off + (unsigned)(((8 * nt + 2 * q) * TM + 32 * mt) * 16), r0, r1, r2, r3);
                h2put_planes(s0, r0, r1, r2, r3, rmax);
            }
        }
    }
    range_check(rmax, range_flag);
}

// Cross-view running sum slab of the workgroup (layout of mlp_core.h slab_store / slab_load: register quad q of tile
// position p of lane l at float4 index (4 p + q) * 64 + l of the wave's part), addressed through a buffer resource: the lane's
// offset in one VGPR instead of 16 hoisted (and spilled) 64-bit addresses.  Non-temporal (aux = 2), like the fp32 kernels'.
struct SlabRef {
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned lane_off;
};
__device__ __forceinline__ void h2slab_store(const f32x16 (&h)[h2::NT][h2::MT], const SlabRef& sl) {
    using namespace h2;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = {h[nt][mt][4 * q + 0], h[nt][mt][4 * q + 1], h[nt][mt][4 * q + 2], h[nt][mt][4 * q + 3]};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), sl.rsrc,
                                                       sl.lane_off + (unsigned)(((nt * MT + mt) * 4 + q) * 64 * 16), 0, 2);
            }
}
__device__ __forceinline__ void h2slab_load(f32x16 (&t)[h2::NT][h2::MT], const SlabRef& sl) {
    using namespace h2;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(sl.rsrc, sl.lane_off, (unsigned)(((nt * MT + mt) * 4 + q) * 64 * 16), 2);
                const f32x4 v = __builtin_bit_cast(f32x4, u);
                t[nt][mt][4 * q + 0] = v.x;
                t[nt][mt][4 * q + 1] = v.y;
                t[nt][mt][4 * q + 2] = v.z;
                t[nt][mt][4 * q + 3] = v.w;
            }
}

// The last per-view block in the view-mean order (header comment): behind its fc_0 GEMM, in registers,
//     net = relu(net + b_fc0) (+ the running sum of the earlier views' relu: `add`),   h += the earlier views' h (`add`),
// and both running sums go back to the lane's slabs for the next view (`store`).  Nothing touches the planes, so no barrier.
// The slabs arrive an accumulator tile at a time through a few buffers of 16 registers (SlabPipe), never the 64 registers of a
// whole slab.
// `add` and `store` are run-time flags of ONE body on purpose: as four instantiations that join in front of the next phase
// the kernel spilled 126 VGPRs instead of 33.
// piece 2 t = tile t of the relu slab, piece 2 t + 1 = tile t of the h slab; SD buffers of 16 registers: SD - 1 pieces are in
// flight while one is summed.  Measured on the C2 frame (profiles/view_mean_fc1.md): depth 2 38.16, 3 37.98, 4 37.89 ms per
// launch at the same spill count, 5 spills more; issuing the first pieces underneath the fc_0 GEMM (h2gemm's `side` hook)
// returned nothing on top (37.83 with two pieces, 38.6 with three).
#ifndef PNY_H2_SLAB_DEPTH
#define PNY_H2_SLAB_DEPTH 4
#endif
struct SlabPipe {
    static constexpr int SD = PNY_H2_SLAB_DEPTH;
    static_assert(SD >= 2, "slab pipeline");
    f32x4 buf[SD][4];
};
__device__ __forceinline__ void h2slab_issue(SlabPipe& sp, int p, const SlabRef& sh, const SlabRef& sr) {
    const SlabRef& s = (p & 1) ? sh : sr;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        sp.buf[p % SlabPipe::SD][q] =
            __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, s.lane_off, (unsigned)(((p >> 1) * 4 + q) * 64 * 16), 2));
}
__device__ __forceinline__ void h2view_sum(f32x16 (&net)[h2::NT][h2::MT], f32x16 (&h)[h2::NT][h2::MT], const float* bias, const SlabRef& sh,
                                           const SlabRef& sr, bool add, bool store, int wave, int lane) {
    using namespace h2;
    SlabPipe sp;
    const float* bl = bias + 32 * NT * wave + 4 * (lane >> 5);
    constexpr int NP = 2 * NT * MT, SD = SlabPipe::SD;
    if (add) {
#pragma unroll
        for (int p = 0; p + 1 < SD; ++p) h2slab_issue(sp, p, sh, sr);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int nt = (p >> 1) / MT, mt = (p >> 1) % MT;
        if (add) {
            if (p + SD - 1 < NP) h2slab_issue(sp, p + SD - 1, sh, sr);
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x16& t = (p & 1) ? h[nt][mt] : net[nt][mt];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(p & 1)) {
                const float4 b = *reinterpret_cast<const float4*>(bl + 32 * nt + 8 * q);
                t[4 * q + 0] = relu1(t[4 * q + 0] + b.x);
                t[4 * q + 1] = relu1(t[4 * q + 1] + b.y);
                t[4 * q + 2] = relu1(t[4 * q + 2] + b.z);
                t[4 * q + 3] = relu1(t[4 * q + 3] + b.w);
            }
            if (add) {
#pragma unroll
                for (int i = 0; i < 4; ++i) t[4 * q + i] = t[4 * q + i] + sp.buf[p % SD][q][i];
            }
            if (store) {
                const SlabRef& s = (p & 1) ? sh : sr;
                const f32x4 v = {t[4 * q + 0], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), s.rsrc, s.lane_off + (unsigned)(((p >> 1) * 4 + q) * 64 * 16), 0, 2);
            }
        }
        if (add) __builtin_amdgcn_sched_barrier(0);
    }
}

// ... and on the last view the planes of the mean, net * rns (rns = 1 / NS; 1 for a single view: today's bits), go to the
// lane's own feature-quad slots like an epilogue's, with the same f16-range guard; then h becomes the mean as well.
__device__ __forceinline__ void h2mean_planes(const f32x16 (&net)[h2::NT][h2::MT], f32x16 (&h)[h2::NT][h2::MT], float rns, char* planes, int wave,
                                              int lane, unsigned* range_flag) {
    using namespace h2;
    float rmax = 0.f;
    char* base = planes + (4 * NT * wave) * (2 * ROW_BYTES) + (lane & 31) * 16 + 8 * (lane >> 5);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                char* s0 = base + (4 * nt + q) * (2 * ROW_BYTES) + 32 * mt * 16;
                const float r0 = net[nt][mt][4 * q + 0] * rns, r1 = net[nt][mt][4 * q + 1] * rns;
                const float r2 = net[nt][mt][4 * q + 2] * rns, r3 = net[nt][mt][4 * q + 3] * rns;
                h2put_planes(s0, r0, r1, r2, r3, rmax);
#pragma unroll
                for (int i = 0; i < 4; ++i) h[nt][mt][4 * q + i] = h[nt][mt][4 * q + i] * rns;
            }
    range_check(rmax, range_flag);
}

// The shared block entry's gather_commit (mlp_core.h; STASH instantiations only): wave w blends samples 8 w .. 8 w + 7 of chunk
// c, feature quads [32 c, 32 c + 32), and writes the first two floats of a quad to the 8 bytes its consumer lane owns in the
// quad's plane-0 slot, the other two to those in its plane-1 slot (rows of OTHER waves: a workgroup barrier follows)
template <int B>
__device__ __forceinline__ void h2gather_commit(const GatherTaps<h2::C, 2>& g, char* planes, int chunk, int wave, int lane) {
    using namespace h2;
    constexpr int NMB = GatherTaps<C>::NMB, QSTEP = GatherTaps<C>::QSTEP;
    const int m = (wave % NMB) * 8 + (lane & 7);
    // quad 32 chunk + 8 qb + (lane >> 3): row 16 chunk + 4 qb + (lane >> 4), half (lane >> 3) & 1
    char* base = planes + (16 * chunk + (lane >> 4)) * (2 * ROW_BYTES) + m * 16 + 8 * ((lane >> 3) & 1);
#pragma unroll
    for (int i = 0; i < GatherTaps<C>::QPW; ++i) {
        const int qb = wave / NMB + i * QSTEP;
        const float4 r = tap_blend(g.x[B][i], g.w);
        char* s0 = base + (4 * qb) * (2 * ROW_BYTES);
        *reinterpret_cast<float2*>(s0) = make_float2(r.x, r.y);
        *reinterpret_cast<float2*>(s0 + ROW_BYTES) = make_float2(r.z, r.w);
    }
}

// ---- The wave-owned block entry (the non-stashing instantiations; header comment) ----------------------------------------------
// Wave w gathers ITS OWN features of the block's projected channels -- the 32 NT consecutive floats per latent pixel that its
// rows hold -- for all TM samples, one accumulator tile (nt, mt) = 32 features x 32 samples at a time ("sub-chunk" t =
// nt MT + mt: 16 float4 tap loads per lane, two sub-chunks in flight).  A wave load covers 8 consecutive samples x one
// 128-byte line: lane l reads feature quad jq = l & 7 of sample 8 pass + (l >> 3).  The lane serves four samples per
// sub-chunk, so tap offsets and weights are re-read from the LDS tap table per sub-chunk (8 lanes per record: a broadcast),
// and the loads go through a buffer resource of the view's map with 32-bit offsets (the wave's channel offset in an SGPR).
struct WaveGather {
    f32x4 x[2][4][4];   // [buffer][pass][tap]
};
template <int B, int T>
__device__ __forceinline__ void h2wave_issue(WaveGather& wg, __amdgpu_buffer_rsrc_t zr, const float4* tap_tab, unsigned c0, int lane) {
    using namespace h2;
    constexpr int nt = T / MT, mt = T % MT;
    asm volatile("" : "+v"(lane));   // (addresses recomputed at every call, not hoisted and spilled: h2wave_entry)
    const float4* tt = tap_tab + 2 * (32 * mt + (lane >> 3));
    const unsigned ql = 16u * (unsigned)(lane & 7);
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const float4 o = tt[16 * pass];
        const unsigned off[4] = {(unsigned)__float_as_int(o.x), (unsigned)__float_as_int(o.y), (unsigned)__float_as_int(o.z), (unsigned)__float_as_int(o.w)};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            wg.x[B][pass][k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(zr, off[k] * 4u + ql, c0 + 128u * nt, 0));
    }
}
// Blend sub-chunk T and stage it in fp32 in the tile's OWN plane bytes (4 rows x 2 slots x 512 bytes = the 4 KiB of 32 x 32
// floats), private to the wave: feature quad j of sample s (both tile-local) at
//     slot (row j >> 1, plane slot j & 1), byte 16 (s ^ j)
// -- the slot whose two halves the quad's consumer lanes overwrite with planes.  The XOR makes both sides conflict-free at
// 16 bytes per lane: the 8 lanes of a store group (one sample, j = 0..7) hit 8 different 16-byte columns, and a read group
// (16 samples, one j) a permutation of 16 contiguous ones.  Then, in accumulator layout (lane = sample m0, half hh; quad q =
// staged quad j = 2 q + hh): acc += bias, += projection (that order), relu, range guard, split, planes -- h2epilogue<true>'s
// arithmetic per quad.  Wave-level ordering only (the LDS serves a wave's instructions in order): the wavefront-scope fences
// keep the compiler from moving the read-back over the staging stores or the plane stores over the read-back.  Quad q's
// planes overwrite slots 2 q and 2 q + 1 only, whose staged values every lane has read by then.
template <int B, int T>
__device__ __forceinline__ void h2wave_commit(const WaveGather& wg, f32x16 (&acc)[h2::NT][h2::MT], const float4* tap_tab, const float* bias,
                                              char* planes, int wave, int lane, float& rmax) {
    using namespace h2;
    constexpr int nt = T / MT, mt = T % MT;
    const int jq = lane & 7, sl = lane >> 3, m0 = lane & 31, hh = lane >> 5;
    char* tb = planes + (4 * NT * wave + 4 * nt) * (2 * ROW_BYTES) + 32 * mt * 16;
    char* wr = tb + jq * ROW_BYTES + 16 * (sl ^ jq);
    const float4* tw = tap_tab + 2 * (32 * mt + sl) + 1;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const float4 w4 = tw[16 * pass];
        const float w[4] = {w4.x, w4.y, w4.z, w4.w};
        float4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = make_float4(wg.x[B][pass][k][0], wg.x[B][pass][k][1], wg.x[B][pass][k][2], wg.x[B][pass][k][3]);
        *reinterpret_cast<float4*>(wr + 128 * pass) = tap_blend(x, w);   // sample 8 pass + sl: column (8 pass + sl) ^ jq
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float* bl = bias + 32 * NT * wave + 32 * nt + 4 * hh;
    // quad q + 1's bias and staged projection are read before quad q's planes are written (other slots)
    auto rd_b = [&](int q) { return *reinterpret_cast<const float4*>(bl + 8 * q); };
    auto rd_z = [&](int q) { return *reinterpret_cast<const float4*>(tb + (2 * q + hh) * ROW_BYTES + 16 * (m0 ^ (2 * q + hh))); };
    float4 b = rd_b(0), z = rd_z(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 bq = b, zq = z;
        if (q + 1 < 4) b = rd_b(q + 1), z = rd_z(q + 1);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        char* s0 = tb + q * (2 * ROW_BYTES) + m0 * 16 + 8 * hh;
        float x0 = acc[nt][mt][4 * q + 0] + bq.x, x1 = acc[nt][mt][4 * q + 1] + bq.y;
        float x2 = acc[nt][mt][4 * q + 2] + bq.z, x3 = acc[nt][mt][4 * q + 3] + bq.w;
        x0 += zq.x;
        x1 += zq.y;
        x2 += zq.z;
        x3 += zq.w;
        acc[nt][mt][4 * q + 0] = x0;
        acc[nt][mt][4 * q + 1] = x1;
        acc[nt][mt][4 * q + 2] = x2;
        acc[nt][mt][4 * q + 3] = x3;
        const float r0 = relu1(x0), r1 = relu1(x1), r2 = relu1(x2), r3 = relu1(x3);
        h2put_planes(s0, r0, r1, r2, r3, rmax);
    }
}
// The whole entry of a per-view block behind barrier A: sub-chunk 0 is in buffer 0 already (fetched before lin_in or
// underneath the previous fc_1 GEMM); the loads of sub-chunk t + 1 are issued before sub-chunk t is blended, staged and
// turned into planes, so that vector work runs while they are in flight.
__device__ __forceinline__ void h2wave_entry(WaveGather& wg, f32x16 (&acc)[h2::NT][h2::MT], __amdgpu_buffer_rsrc_t zr, const float4* tap_tab, unsigned c0,
                                             const float* bias, char* planes, int wave, int lane, unsigned* range_flag) {
    static_assert(h2::NT * h2::MT == 4, "four sub-chunks");
    // the entry's lane-dependent addresses are recomputed here (a dozen VALU instructions) instead of being hoisted out of the
    // tile loop and kept, i.e. spilled, across the GEMMs
    asm volatile("" : "+v"(lane));
    float rmax = 0.f;
    h2wave_issue<1, 1>(wg, zr, tap_tab, c0, lane);
    __builtin_amdgcn_sched_barrier(0);
    h2wave_commit<0, 0>(wg, acc, tap_tab, bias, planes, wave, lane, rmax);
    h2wave_issue<0, 2>(wg, zr, tap_tab, c0, lane);
    __builtin_amdgcn_sched_barrier(0);
    h2wave_commit<1, 1>(wg, acc, tap_tab, bias, planes, wave, lane, rmax);
    h2wave_issue<1, 3>(wg, zr, tap_tab, c0, lane);
    __builtin_amdgcn_sched_barrier(0);
    h2wave_commit<0, 2>(wg, acc, tap_tab, bias, planes, wave, lane, rmax);
    h2wave_commit<1, 3>(wg, acc, tap_tab, bias, planes, wave, lane, rmax);
    range_check(rmax, range_flag);
}

// ---- lin_out as a split-K product on the matrix cores (the two-plane instantiations; header comment) ------------------------------
// out^T = W_out relu(h_top)^T, W_out as a split-f16 image of its own (pack.hip PACK_H2O: one n-tile of 32 output rows, two
// for d_out > 32, the rows past d_out zero).  Wave w multiplies the k-steps of ITS OWN features with the planes its own
// lanes have just written in h2epilogue -- wave-level ordering as in h2wave_commit, no workgroup barrier between epilogue
// and product -- into ONE partial per 64-k chunk (the 64-sample shape: the wave's 64 features are chunk w; the 32-sample
// shape: two chunks, 2 w and 2 w + 1, in separate accumulators), so that both shapes add the same products in the same order.
// Per k-step the products come in h2gemm's order: x1 w1, x2 w1, x1 w2.  The partials go to the wave's own plane rows, which
// are free once the B fragments are in registers (all of them are read first: with two n-tiles the first one's partials
// already cover rows the second would still read): chunk c of the wave at c * TM * QO * 16 bytes of the wave's 16 KiB, output
// quad qd (outputs 4 qd .. 4 qd + 3; QO = ceil(d_out / 4) of them) of sample m at (m QO + qd) * 16 -- for d_out = 4 the 32
// lanes of an m-tile write 512 contiguous bytes.  Behind one workgroup barrier h2linout_reduce adds the 8 chunks in chunk
// order in fp32.
#if PNY_H2_PLANES == 2
struct LinOutW {
    h8 f[2 * h2::NT][2];   // [k-step of the wave][plane] of one n-tile of the lin_out image
};
// fragment (step j, n-tile nto, plane p) of the image at byte `img_off` of the weight blob: this lane's W_out[32 nto + (l & 31)][16 j + 8 (l >> 5) + 0..7]
__device__ __forceinline__ void h2linout_issue(LinOutW& lw, const WStream& ws, unsigned img_off, int nto_n, int nto, int wave) {
    using namespace h2;
    // (the 4 NT scalar offsets are formed here, per call: hoisted out of the tile loop they are SGPRs spilled across the GEMMs)
    unsigned base = img_off + (unsigned)(((2 * NT * wave * nto_n + nto) * 2) * 64) * 16u, step = (unsigned)(nto_n * 2 * 64) * 16u;
    asm volatile("" : "+s"(base), "+s"(step));
#pragma unroll
    for (int ks = 0; ks < 2 * NT; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p)
            lw.f[ks][p] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(ws.rsrc, ws.lane_off, base + ks * step + (unsigned)(p * 64) * 16u, 0));
}
constexpr int LINOUT_WAVE_BYTES = 4 * h2::NT * 2 * h2::ROW_BYTES;   // the plane rows of one wave: 16 KiB in both shapes
static_assert((h2::NT / 2) * h2::TM * 16 * 16 <= LINOUT_WAVE_BYTES, "a wave's partials (64 outputs) fit its own rows");
__device__ __forceinline__ void h2linout_product(LinOutW& lw, const WStream& ws, unsigned img_off, int d_out, char* planes, int wave, int lane) {
    using namespace h2;
    constexpr int NCH = NT / 2;   // 64-k chunks of the wave
    asm volatile("" : "+v"(lane));   // (addresses recomputed here, not hoisted over the GEMMs and spilled: h2wave_entry)
    const int m0 = lane & 31, hh = lane >> 5;
    const int qo = (d_out + 3) >> 2, nto_n = d_out > 32 ? 2 : 1;
    char* region = planes + wave * LINOUT_WAVE_BYTES;
    // the planes come from other lanes of this wave (h2epilogue); the LDS serves a wave's instructions in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    h8 B[NCH][MT][4][2];   // k-step 4 c + ks of the wave = rows 2 (4 c + ks) + hh of its rows
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    B[c][mt][ks][p] = *reinterpret_cast<const h8*>(region + (2 * (4 * c + ks) + hh) * (2 * ROW_BYTES) + p * ROW_BYTES + (32 * mt + m0) * 16);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the partial stores below stay behind these reads
    for (int nto = 0; nto < nto_n; ++nto) {
        if (nto > 0) h2linout_issue(lw, ws, img_off, nto_n, nto, wave);   // (n-tile 0 was fetched ahead of the epilogue)
        f32x16 acc[NCH][MT];
        h2zero<NCH, MT>(acc);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[c][mt] = h2mfma(lw.f[4 * c + ks][0], B[c][mt][ks][0], acc[c][mt]);
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[c][mt] = h2mfma(lw.f[4 * c + ks][0], B[c][mt][ks][1], acc[c][mt]);
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[c][mt] = h2mfma(lw.f[4 * c + ks][1], B[c][mt][ks][0], acc[c][mt]);
        }
        // accumulator quad q of this lane = outputs 32 nto + 8 q + 4 hh + 0..3 of sample 32 mt + m0: output quad 8 nto + 2 q + hh
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int qd = 8 * nto + 2 * q + hh;
                    if (qd < qo)
                        *reinterpret_cast<f32x4*>(region + c * (TM * qo * 16) + ((32 * mt + m0) * qo + qd) * 16) =
                            f32x4{acc[c][mt][4 * q + 0], acc[c][mt][4 * q + 1], acc[c][mt][4 * q + 2], acc[c][mt][4 * q + 3]};
                }
    }
}
// ... and behind the workgroup barrier: the chunks' partials summed in chunk order 0 .. 7, + b_out, the output head, the store
// (one thread per sample and output quad; d_out = 4: one 16-byte store per sample)
__device__ __forceinline__ void h2linout_reduce(const MlpArgs& a, long long tile, const char* planes, int tid) {
    using namespace h2;
    constexpr int NCH = NT / 2, NCHUNK = (THREADS / 64) * NCH;
    static_assert(NCHUNK * 64 == HID, "eight chunks of 64 k");
    asm volatile("" : "+v"(tid));   // (as in h2linout_product)
    const int qo = (a.d_out + 3) >> 2;
    const bool vec = a.d_out == 4 && (reinterpret_cast<size_t>(a.out) & 15) == 0;
    for (int idx = tid; idx < qo * TM; idx += THREADS) {
        const int qd = idx / TM, m = idx % TM;
        const char* src = planes + (m * qo + qd) * 16;
        f32x4 part[NCHUNK];
#pragma unroll
        for (int g = 0; g < NCHUNK; ++g) part[g] = *reinterpret_cast<const f32x4*>(src + (g / NCH) * LINOUT_WAVE_BYTES + (g % NCH) * (TM * qo * 16));
        float sum[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sum[i] = part[0][i];
#pragma unroll
            for (int g = 1; g < NCHUNK; ++g) sum[i] = sum[i] + part[g][i];
        }
        const long long s = tile * TM + m;
        if (s >= a.n_points) continue;
        if (vec) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sum[i] = output_head(sum[i] + a.w.b_out[i], i, a.yolo);
            *reinterpret_cast<float4*>(a.out + s * 4) = make_float4(sum[0], sum[1], sum[2], sum[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int o = 4 * qd + i;
                if (o < a.d_out) a.out[s * a.d_out + o] = output_head(sum[i] + a.w.b_out[o], o, a.yolo);
            }
        }
    }
}
#endif

// per (view, tile) prologue: the lin_in B operand (positional code, view dirs) as f16 planes in rows 0..7 of each plane, and
// the tap table; the arithmetic is prologue<C>()'s (mlp_core.h).  STASH: the operand also goes to the stash in fp32
// ([feature/4][sample]), and a second table holds the same taps addressing the latent itself (pixel x L).
template <bool STASH>
__device__ __forceinline__ void h2prologue(const MlpArgs& a, int v, long long tile, char* planes, float4* tap_tab, int tid, unsigned* range_flag,
                                           __amdgpu_buffer_rsrc_t stash = __amdgpu_buffer_rsrc_t(), unsigned stash_xin = 0, float4* tap_raw = nullptr) {
    using namespace h2;
    constexpr int NPART = THREADS / TM;
    const int m = tid % TM, part = tid / TM;
    long long s = tile * TM + m;
    if (s >= a.n_points) s = a.n_points - 1;
    float p[3], d[3];
    load_point(a, s, p, d);
    const Cam cam = a.cams[tile_view_base(a, tile * TM) + v];
    float xr[3], xc[3], vd[3];
    camera_point(cam, p, d, xr, xc, vd);
    float rmax = 0.f;   // f16-range guard: lin_in's inputs (coordinates, view directions) go through the same split
    for (int g = part; g < D_IN_PAD / 4; g += NPART) {
        const float e0 = input_entry(4 * g + 0, xr, vd, a.freq_factor, a.num_freqs), e1 = input_entry(4 * g + 1, xr, vd, a.freq_factor, a.num_freqs);
        const float e2 = input_entry(4 * g + 2, xr, vd, a.freq_factor, a.num_freqs), e3 = input_entry(4 * g + 3, xr, vd, a.freq_factor, a.num_freqs);
        if constexpr (STASH) stash_store(stash, (unsigned)((g * TM + m) * 16), stash_xin, e0, e1, e2, e3);
        h2put_planes<true>(planes + (g >> 1) * (2 * ROW_BYTES) + m * 16 + 8 * (g & 1), e0, e1, e2, e3, rmax);
    }
    range_check(rmax, range_flag);
    if (part == NPART - 1) {
        int pix[4], offs[4];
        float wgt[4];
        pixel_taps(a, cam, xc, 1, pix, wgt);
#pragma unroll
        for (int k = 0; k < 4; ++k) offs[k] = pix[k] * a.tap_stride;
        tap_record(tap_tab, m, offs, wgt);
        if constexpr (STASH) {
#pragma unroll
            for (int k = 0; k < 4; ++k) offs[k] = pix[k] * a.L;
            tap_record(tap_raw, m, offs, wgt);
        }
    }
}

// STASH = the training forward (pny_scene_stash_next_render): the same kernel also writes every operand the backward needs to
// the tile's record of the X stash in fp32 -- the positional-code inputs, the interpolated latent z (an extra gather of the
// raw latent per view: the weight gradient of lin_z needs it, the forward itself only the projected maps), relu(h_in) and
// relu(net) of every block, relu(h_top) -- in the layout the fp32 STASH kernel of mlp.hip writes.
template <bool STASH>
__global__ __launch_bounds__(h2::THREADS, 2) void PNY_H2_KERNEL(const MlpArgs a) {
    using namespace h2;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* planes = smem_raw;
    float4* tap_tab = reinterpret_cast<float4*>(smem_raw + ACT_BYTES);
    float* bias_tab = reinterpret_cast<float*>(smem_raw + ACT_BYTES + TAP_BYTES);   // [b_in, b_fc0[0], b_fc1[0], b_fc0[1], ...][512]
    float4* tap_raw = reinterpret_cast<float4*>(smem_raw + lds_bytes(a.n_blocks));   // STASH only: taps addressing the raw latent
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const SlabRef slab = {__builtin_amdgcn_make_buffer_rsrc(a.scratch + (size_t)blockIdx.x * (TM * HID), 0, TM * HID * 4, 0x00020000),
                          (unsigned)((wave * (NT * MT * 16 * 64) + 4 * lane) * 4)};
    // The view-mean order (header comment) of the non-stashing two-plane instantiations; -DPNY_H2_PER_VIEW_FC1 (diagnostic
    // builds only, tools/h2_variant_build.sh) keeps the per-view order for an A/B.  Its second slab, the running sum of
    // relu(net), lies behind the h slabs of the whole grid.
#if defined(PNY_H2_PER_VIEW_FC1) || PNY_H2_PLANES == 1
    constexpr bool VIEW_MEAN = false;
#else
    constexpr bool VIEW_MEAN = !STASH;
#endif
    // The block entry: wave-owned (h2wave_entry) in every non-stashing instantiation -- pny_mlp_h2_kernel<false>,
    // pny_mlp_h2s_kernel, pny_mlp_h1_kernel<false>; the STASH instantiations (training forwards) keep the shared entry
    // (h2gather_commit, the "projection visible" barrier, h2epilogue<true>): they also gather the raw latent in the shared
    // lane mapping and are far over the register budget already.
    constexpr bool WAVE_ENTRY = !STASH;
    const SlabRef slab_r = {__builtin_amdgcn_make_buffer_rsrc(a.scratch + ((size_t)gridDim.x + blockIdx.x) * (TM * HID), 0, TM * HID * 4, 0x00020000),
                            slab.lane_off};
    const int nb = a.n_blocks;
    const int nvb = a.combine_layer < nb ? a.combine_layer : nb;   // >= 1 (the host only selects this kernel with a projection)
    const WStream ws = wstream(a, lane);
    const H2Seg s_in = h2seg(ws, a.h2_in, D_IN_PAD / 16, wave);
    auto fc0seg = [&](int b) { return h2seg(ws, a.h2_fc0[b], HID / 16, wave); };
    auto fc1seg = [&](int b) { return h2seg(ws, a.h2_fc1[b], HID / 16, wave); };
    // bias applied at the entry of block b (b = n_blocks: before lin_out): b_in, or the previous block's b_fc1 -- the
    // packing (pack.hip PACK_ADD2) has folded the block's lin_z bias into either
    auto entry_bias = [&](int b) -> const float* {
        if constexpr (LDS_BIAS) return bias_tab + (b == 0 ? 0 : 2 * b) * HID;
        return b == 0 ? a.w.b_in : a.w.b_fc1[b - 1];   // (folded with the block's lin_z bias, pack.hip PACK_ADD2)
    };
    auto fc0_bias = [&](int b) -> const float* {
        if constexpr (LDS_BIAS) return bias_tab + (1 + 2 * b) * HID;
        return a.w.b_fc0[b];
    };
    H2Ring ring;
    h2ring_fill(ring, ws, s_in);
#ifdef PNY_H2_STAMP
    unsigned long long hs_acc[HS_N], hs_t_ = 0;
    for (int i = 0; i < HS_N; ++i) hs_acc[i] = 0;
    const unsigned long long hs_start = h2now();
    const unsigned long long hs_real0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
#endif
    if constexpr (LDS_BIAS) {
        for (int i = tid; i < (1 + 2 * nb) * HID; i += THREADS) {
            const int vec = i / HID, f = i % HID;
            const float* src = vec == 0 ? a.w.b_in : ((vec & 1) ? a.w.b_fc0[(vec - 1) >> 1] : a.w.b_fc1[(vec - 2) >> 1]);
            bias_tab[i] = src[f];
        }
    }

    const TileWalk tw = tile_walk(a.n_tiles);   // XCD-aware order (mlp_core.h)
    for (long long tile = tw.first; tile < tw.last; tile += tw.step) {
        f32x16 h[NT][MT];
        f32x16 net[NT][MT];
        GatherTaps<C, 2> g;   // shared entry: taps of the current view; two chunks of projected channels in flight
        WaveGather wg;        // wave-owned entry: two sub-chunks in flight
        __amdgpu_buffer_rsrc_t zr = __amdgpu_buffer_rsrc_t();   // the current view's projected map
        const unsigned wave_c0 = (unsigned)(32 * NT * wave) * 4u;   // byte offset of the wave's first feature inside a block's 512 channels
        auto prefetch = [&](int c0) {   // first piece of the projection of the block at channel c0 into buffer 0
            if constexpr (WAVE_ENTRY)
                h2wave_issue<0, 0>(wg, zr, tap_tab, (unsigned)c0 * 4u + wave_c0, lane);
            else
                gather_issue<C, 0>(g, c0, wave);
        };
        // one residual block from "planes hold relu(h_in)" on: net = fc_0(.), h += fc_1(relu(net + b_fc0)).  `next_c0` >= 0:
        // the first chunk of the NEXT block's projection (channel offset next_c0) is fetched into gather buffer 0
        // underneath the fc_1 GEMM -- `net` is dead there, its registers hold the chunk.
        // this tile's record of the X stash as a buffer resource; byte offsets spelled out in stash.h's order (its accessors cost scratch here)
        __amdgpu_buffer_rsrc_t xr = __amdgpu_buffer_rsrc_t();
        if constexpr (STASH)
            xr = stash_rsrc(a.lay.x_record(a.stash_x, tile), a.lay.x_tile);
        auto block_tail = [&](int blk, const H2Seg& after, bool slab_in, int next_c0, unsigned stash_net) {
            HS_T0();
            h2zero<NT, MT>(net);
            __syncthreads();
            HS_LAP(HS_EPI_WAIT);
            h2gemm(net, ring, ws, fc0seg(blk), fc1seg(blk), planes, lane);
            HS_LAP(HS_GEMM);
            __syncthreads();
            HS_LAP(HS_EPI_WAIT);
            h2epilogue<false, STASH>(net, fc0_bias(blk), planes, wave, lane, a.range_flag, xr, stash_net);
            // three exclusive continuations (the running sum of the other views and the prefetched chunk both want the
            // registers of `net`: written as one if / else chain so that the allocator never has to provide for both)
            if (!VIEW_MEAN && slab_in) {   // (per-view order only: the view-mean order sums in mean_tail)
                h2slab_load(net, slab);
                HS_LAP(HS_EPI);
                __syncthreads();
                HS_LAP(HS_EPI_WAIT);
                h2gemm(h, ring, ws, fc1seg(blk), after, planes, lane);
                HS_LAP(HS_GEMM);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) h[nt][mt][r] = net[nt][mt][r] + h[nt][mt][r];
            } else if (next_c0 >= 0) {
                HS_LAP(HS_EPI);
                __syncthreads();
                HS_LAP(HS_EPI_WAIT);
                h2gemm(h, ring, ws, fc1seg(blk), after, planes, lane, [&]() { prefetch(next_c0); });
                HS_LAP(HS_GEMM);
            } else {
                HS_LAP(HS_EPI);
                __syncthreads();
                HS_LAP(HS_EPI_WAIT);
                h2gemm(h, ring, ws, fc1seg(blk), after, planes, lane);
                HS_LAP(HS_GEMM);
            }
        };
        for (int v = 0; v < a.NS; ++v) {
            // grouped scene: the tile's object sees views vb .. vb + NS - 1 (recomputed per view: a value kept across the
            // GEMM loops costs SGPR spills)
            const int vb = tile_view_base(a, tile * TM);
            const H2Seg after_view = v + 1 < a.NS ? s_in : (nvb < nb ? fc0seg(nvb) : s_in);
            const unsigned x_view = STASH ? stash_bytes((unsigned)v * (unsigned)a.lay.x_view) : 0u;
            auto act_slot = [&](int i) { return x_view + stash_bytes((unsigned)a.lay.o_act + (unsigned)i * (unsigned)STASH_SLOT); };
            HS_T0();
            __syncthreads();
            h2prologue<STASH>(a, v, tile, planes, tap_tab, tid, a.range_flag, xr, x_view + stash_bytes((unsigned)a.lay.o_in), tap_raw);
            h2zero<NT, MT>(h);
            __syncthreads();
            if constexpr (STASH) {
                // z = the interpolated latent of this view (reference encoder.py:101), the B operand of lin_z's weight
                // gradient: gathered from the latent itself, 128 channels at a time, two chunks in flight, written straight
                // to the stash (a lane holds 4 channels of one sample = one float4 of the [channel/4][sample] tile)
                const unsigned xz = x_view + stash_bytes((unsigned)a.lay.o_z);
                gather_setup<C>(g, a.latent + (size_t)(vb + v) * a.Hl * a.Wl * a.L, tap_raw, wave, lane);
                const int nch = a.L / GCH;
                const unsigned zlane = (unsigned)(((lane >> 3) * TM + (wave % 8) * 8 + (lane & 7)) * 16);
                auto put = [&](const float4(&x)[4][4], int c) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float4 r = tap_blend(x[i], g.w);
                        stash_store(xr, zlane, xz + (unsigned)((32 * c + 8 * i) * TM * 16), r.x, r.y, r.z, r.w);
                    }
                };
                gather_issue<C, 0>(g, 0, wave);
                for (int c = 0; c < nch; c += 2) {
                    if (c + 1 < nch) gather_issue<C, 1>(g, (c + 1) * GCH, wave);
                    __builtin_amdgcn_sched_barrier(0);
                    put(g.x[0], c);
                    if (c + 2 < nch) gather_issue<C, 0>(g, (c + 2) * GCH, wave);
                    __builtin_amdgcn_sched_barrier(0);
                    if (c + 1 < nch) put(g.x[1], c + 1);
                }
            }
            if constexpr (WAVE_ENTRY) {
                // (a view's map is under 4 GiB: render_api.hip wants_projection; a read past it would return zeros)
                const size_t zfloats = (size_t)a.Hl * a.Wl * a.zp_stride;
                zr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.zp) + (size_t)(vb + v) * zfloats, 0, (int)(unsigned)(zfloats * 4), 0x00020000);
            } else {
                gather_setup<C>(g, a.zp + (size_t)(vb + v) * a.Hl * a.Wl * a.zp_stride, tap_tab, wave, lane);
            }
            prefetch(0);   // block 0, first piece
            HS_LAP(HS_PROLOGUE);
            h2gemm(h, ring, ws, s_in, fc0seg(0), planes, lane);
            HS_LAP(HS_GEMM);
            // one per-view block; the last one of a view is a call site of its own so that the compiler sees that the
            // gather buffers are dead across its fc_1 GEMM (where the other views' running sum takes those registers)
            auto block_entry = [&](int blk) {
                // h += interp(lin_z[blk](latent map)): the block's 512 projected channels in 4 chunks of 128, staged in
                // fp32 (see h2epilogue).  Chunk 0 is in buffer 0 already (issued before / underneath the previous GEMM);
                // from here two chunks are in flight: the loads of chunk c + 1 are issued before chunk c is blended.
                const int cb = blk * HID;
                HS_LAP(HS_GATHER);
                __syncthreads();  // every wave is done reading the planes (previous GEMM)
                HS_LAP(HS_GATHER_WAIT);
                if constexpr (WAVE_ENTRY) {
                    // wave-private from here to the fc_0 GEMM's barrier: gather, staging, bias + projection, relu, planes
                    h2wave_entry(wg, h, zr, tap_tab, (unsigned)cb * 4u + wave_c0, entry_bias(blk), planes, wave, lane, a.range_flag);
                    HS_LAP(HS_GATHER);
                    return;
                }
                gather_issue<C, 1>(g, cb + GCH, wave);
                __builtin_amdgcn_sched_barrier(0);
                h2gather_commit<0>(g, planes, 0, wave, lane);
                gather_issue<C, 0>(g, cb + 2 * GCH, wave);
                __builtin_amdgcn_sched_barrier(0);
                h2gather_commit<1>(g, planes, 1, wave, lane);
                gather_issue<C, 1>(g, cb + 3 * GCH, wave);
                __builtin_amdgcn_sched_barrier(0);
                h2gather_commit<0>(g, planes, 2, wave, lane);
                h2gather_commit<1>(g, planes, 3, wave, lane);
                HS_LAP(HS_GATHER);
                __syncthreads();  // projection visible
                HS_LAP(HS_GATHER_WAIT);
                h2epilogue<true, STASH>(h, entry_bias(blk), planes, wave, lane, a.range_flag, xr, act_slot(2 * blk));
                HS_LAP(HS_EPI);
            };
            auto view_block = [&](int blk, const H2Seg& after, bool slab_in, int next_c0) {
                block_entry(blk);
                block_tail(blk, after, slab_in, next_c0, act_slot(2 * blk + 1));
            };
            // The last per-view block in the view-mean order: fc_1 is linear, so mean_v(h_v + fc_1(R_v)) = mean_v(h_v) +
            // fc_1(mean_v R_v) with R_v = relu(net_v + b_fc0) -- every view but the last ends behind its fc_0 GEMM, with both
            // running sums in the slabs and the ring primed for the next view's lin_in; the last view runs the one fc_1 GEMM.
            auto mean_tail = [&](int blk) {
                const bool last = v + 1 == a.NS;
                HS_T0();
                h2zero<NT, MT>(net);
                __syncthreads();
                HS_LAP(HS_EPI_WAIT);
                h2gemm(net, ring, ws, fc0seg(blk), last ? fc1seg(blk) : s_in, planes, lane);
                HS_LAP(HS_GEMM);
                h2view_sum(net, h, fc0_bias(blk), slab, slab_r, v > 0, !last, wave, lane);
                if (!last) {
                    HS_LAP(HS_SLAB);
                    return;
                }
                HS_LAP(v > 0 ? HS_SLAB : HS_EPI);
                __syncthreads();   // every wave is done reading the planes (fc_0 GEMM)
                HS_LAP(HS_EPI_WAIT);
                h2mean_planes(net, h, 1.0f / (float)a.NS, planes, wave, lane, a.range_flag);
                HS_LAP(HS_EPI);
                __syncthreads();
                HS_LAP(HS_EPI_WAIT);
                h2gemm(h, ring, ws, fc1seg(blk), after_view, planes, lane);
                HS_LAP(HS_GEMM);
            };
#if defined(PNY_H2_NOPREFETCH)
            for (int blk = 0; blk + 1 < nvb; ++blk) {
                view_block(blk, fc0seg(blk + 1), false, -1);
                prefetch((blk + 1) * HID);
            }
#else
            for (int blk = 0; blk + 1 < nvb; ++blk) view_block(blk, fc0seg(blk + 1), false, (blk + 1) * HID);
#endif
            if constexpr (VIEW_MEAN) {
                block_entry(nvb - 1);
                mean_tail(nvb - 1);
            } else {
                view_block(nvb - 1, after_view, v > 0, -1);
            }
            if (!VIEW_MEAN && a.NS > 1) {
                HS_T0();
                if (v + 1 < a.NS) {
                    h2slab_store(h, slab);
                } else {
                    const float rns = 1.0f / (float)a.NS;   // (the fp32 kernel divides; one rounding more here, far inside the bar)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) h[nt][mt][r] = h[nt][mt][r] * rns;
                }
                HS_LAP(HS_SLAB);
            }
        }
        auto post_slot = [&](int i) { return stash_bytes((unsigned)a.lay.x_post + (unsigned)i * (unsigned)STASH_SLOT); };
        for (int blk = nvb; blk < nb; ++blk) {
            HS_T0();
            __syncthreads();
            HS_LAP(HS_EPI_WAIT);
            h2epilogue<false, STASH>(h, entry_bias(blk), planes, wave, lane, a.range_flag, xr, post_slot(2 * (blk - nvb)));
            HS_LAP(HS_EPI);
            block_tail(blk, blk + 1 < nb ? fc0seg(blk + 1) : s_in, false, -1, post_slot(2 * (blk - nvb) + 1));
        }
        // out = lin_out(relu(h + b_fc1[last])) (reference resnetfc.py:185) + output head (models.py:312-317)
        HS_T0();
#if PNY_H2_PLANES == 2
        // Two planes: lin_out is a split-K product on the matrix cores (h2linout_product).  The wave's fragments of the first
        // n-tile are fetched ahead of the barrier and the epilogue; between epilogue and product there is no workgroup barrier.
        // The reduction's readers are done before they reach the barrier in front of the next tile's h2prologue, which
        // overwrites rows 0..7.
        const unsigned out_off = (unsigned)(reinterpret_cast<const char*>(a.h2_out) - ws.base);
        LinOutW lw;
        h2linout_issue(lw, ws, out_off, a.d_out > 32 ? 2 : 1, 0, wave);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        h2epilogue<false, STASH>(h, entry_bias(nb), planes, wave, lane, a.range_flag, xr, post_slot(2 * (nb - nvb)));
        h2linout_product(lw, ws, out_off, a.d_out, planes, wave, lane);
        __syncthreads();
        h2linout_reduce(a, tile, planes, tid);
#else
        // One plane: fp32 dot products with w_out as stored, on the planes behind a workgroup barrier
        __syncthreads();
        h2epilogue<false, STASH>(h, entry_bias(nb), planes, wave, lane, a.range_flag, xr, post_slot(2 * (nb - nvb)));
        __syncthreads();
        for (int idx = tid; idx < a.d_out * TM; idx += THREADS) {
            const int o = idx / TM, m = idx % TM;
            const float4* wrow = reinterpret_cast<const float4*>(a.w.w_out + (size_t)o * HID);
            float sum = 0.f;
#pragma unroll 4
            for (int kg = 0; kg < HID / 8; ++kg) {
                const h8 x0 = *reinterpret_cast<const h8*>(planes + kg * (2 * ROW_BYTES) + m * 16);
                const float4 wa = wrow[2 * kg], wb = wrow[2 * kg + 1];
                sum += (float)x0[0] * wa.x;
                sum += (float)x0[1] * wa.y;
                sum += (float)x0[2] * wa.z;
                sum += (float)x0[3] * wa.w;
                sum += (float)x0[4] * wb.x;
                sum += (float)x0[5] * wb.y;
                sum += (float)x0[6] * wb.z;
                sum += (float)x0[7] * wb.w;
            }
            sum = output_head(sum + a.w.b_out[o], o, a.yolo);
            const long long s = tile * TM + m;
            if (s < a.n_points) a.out[s * a.d_out + o] = sum;
        }
#endif
        HS_LAP(HS_LINOUT);
    }
#ifdef PNY_H2_STAMP
    hs_acc[HS_TOTAL] = h2now() - hs_start;
    hs_acc[HS_REAL] = __builtin_amdgcn_s_memrealtime() - hs_real0;
    if (lane == 0)
        for (int i = 0; i < HS_N; ++i) g_h2_stamp_buf[((size_t)blockIdx.x * (THREADS / 64) + wave) * HS_N + i] = hs_acc[i];
#endif
}

#if !defined(PNY_H2_SPLIT) && PNY_H2_PLANES == 2
bool mlp_h2_supports(int n_blocks, int combine_layer) { return n_blocks <= h2::MAX_NB && combine_layer >= 1; }
#endif

template <bool STASH>
static void launch_mlp_h2_t(const MlpArgs& a, int grid, hipStream_t st) {
    const int extra = STASH ? h2::TAP_BYTES : 0;   // second tap table
    static LdsLimit lds;
    (void)lds.raise(h2::lds_bytes(h2::MAX_NB) + extra, PNY_H2_KERNEL<STASH>);
#ifdef PNY_H2_STAMP
    // debug buffer, raw and never freed on purpose: a static's destructor would run after the HIP runtime may have shut down
    static unsigned long long* dbuf = nullptr;
    constexpr int NWV = h2::THREADS / 64;
    const size_t nst = (size_t)grid * NWV * HS_N;
    if (!dbuf) {
        (void)hipMalloc((void**)&dbuf, (size_t)1024 * 8 * HS_N * sizeof(unsigned long long));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_h2_stamp_buf), &dbuf, sizeof(dbuf));
    }
    (void)hipMemsetAsync(dbuf, 0, nst * sizeof(unsigned long long), st);
#endif
    hipLaunchKernelGGL(PNY_H2_KERNEL<STASH>, dim3(grid), dim3(h2::THREADS), h2::lds_bytes(a.n_blocks) + extra, st, a);
#ifdef PNY_H2_STAMP
    {
        std::vector<unsigned long long> hst(nst);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(hst.data(), dbuf, nst * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        double sum[HS_N] = {0};
        for (size_t i = 0; i < nst; ++i) sum[i % HS_N] += (double)hst[i];
        static const char* names[HS_N] = {"total", "gemm", "gather-barrier-wait", "gather", "epilogue-barrier-wait", "epilogue", "prologue", "lin_out", "slab", "realtime"};
        fprintf(stderr, "[h2 stamp%s, %d x %d] tiles=%d grid=%d:", STASH ? ", stash" : "", h2::NT, h2::MT, a.n_tiles, grid);
        for (int i = 0; i < HS_N; ++i) fprintf(stderr, " %s=%.1f%%", names[i], 100.0 * sum[i] / sum[0]);
        fprintf(stderr, " (mean wave cycles %.4g; in-kernel clock %.3f GHz = wave cycles / s_memrealtime ticks x 100 MHz)\n",
                sum[0] / ((double)grid * NWV), sum[0] / sum[HS_REAL] * 0.1);
    }
#endif
}

#if PNY_H2_PLANES == 1 && defined(PNY_H1_STASH)
// training forward of PNY_PRECISION_F16_TRAIN (mlp_h1t.hip): as launch_mlp_h2_stash, with the single-plane images
void launch_mlp_h1_stash(const MlpArgs& a, int grid, hipStream_t st) { launch_mlp_h2_t<true>(a, grid, st); }
#elif PNY_H2_PLANES == 1
// single-plane images in a.h2_in / a.h2_fc0 / a.h2_fc1 and their buffer in a.w_base / a.w_bytes; 64-sample tiles
void launch_mlp_h1(const MlpArgs& a, int grid, hipStream_t st) { launch_mlp_h2_t<false>(a, grid, st); }
#elif defined(PNY_H2_SPLIT)
// 32-sample tiles, two workgroups per CU: a.n_tiles counts 32-sample tiles, grid <= 2 x CUs
void launch_mlp_h2s(const MlpArgs& a, int grid, hipStream_t st) { launch_mlp_h2_t<false>(a, grid, st); }
#else
void launch_mlp_h2(const MlpArgs& a, int grid, hipStream_t st) { launch_mlp_h2_t<false>(a, grid, st); }
// training forward: a.stash_x / a.lay set, a.zp AND a.latent valid (152 + 2 KiB of LDS for 5 blocks)
void launch_mlp_h2_stash(const MlpArgs& a, int grid, hipStream_t st) { launch_mlp_h2_t<true>(a, grid, st); }
#endif

}  // namespace pny
