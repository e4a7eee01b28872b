// The packed weight operands of the fused MLP and of the latent projection, and the ONE kernel that builds them from the
// state_dict tensors: pny_model_finalize runs it on uploaded copies, pny_model_refresh (after an optimizer step) on the
// live parameter tensors where PyTorch keeps them -- no state_dict round trip through the host (27 MB of repacking and a
// synchronous upload per step before).  This file is the description of the formats; model_api.hip only lays the images out
// and lists the jobs (pack_mlp), encoder.hip build_pixel_linear allocates the projection weights.  A job writes `count`
// 16-byte elements, element i as below; W is the (n_out x k_in) row-major tensor, K padded with zeros to k_pad.
//
// PACK_A   A-operand order of v_mfma_f32_32x32x2_f32 for H^T = W X^T (mlp.hip): k-iteration j (8 inputs), n-tile nt (32
//          output features), lane l, component r:  dst[((j*16 + nt)*64 + l)*4 + r] = W[32 nt + (l & 31)][8 j + 4 (l >> 5) + r].
//          k-iteration-major: the 16 KiB that ALL waves of a workgroup need for iteration j are contiguous, so the 16
//          per-wave streams of a CU walk the same pages together (measured +1 % over n-tile-major, where each stream strides
//          through its own 64 KiB region).
// PACK_AT  the same with W^T as the matrix, for the backward chain (dX^T = W^T dY^T, mlp_bwd.hip): W^T is (k_in x n_out),
//          its rows (the GEMM's outputs) are 512 and its K (= n_out) is padded to k_pad.
// PACK_NT  the same elements n-tile-major, [n-tile][k-iteration][lane]: the projection weights (encoder.hip, one job per
//          stacked lin_z block) -- the order of the trunk's convolution weights.
// PACK_NTT W^T n-tile-major as one block of a wider image: the stacked lin_z^T of the latent gradient (latent_grad.hip).
// PACK_H2  split-f16 image for mlp_h2.hip: w = w1 + w2, w1 = f16(w), w2 = f16(w - w1) (round to nearest); per 16-k step j
//          [n-tile][plane][lane] x 8 halves, lane l holding W[32 nt + (l & 31)][16 j + 8 (l >> 5) + 0..7].  4 bytes per weight.
// PACK_H2T the same of W^T (mlp_bwd_h2.hip).
// PACK_H2O the PACK_H2 image of lin_out (mlp_h2.hip's split-K product): n_out <= 64 rows padded with zero rows to 32, or to 64
//          for n_out > 32, so per 16-k step one or two n-tiles instead of 16 (the same branch of the kernel as PACK_H2).
// PACK_H1  plane 0 of a PACK_H2 / PACK_H2T image, 2 bytes per weight (mlp_h1.hip, mlp_bwd_h1.hip).
// PACK_COPY / PACK_ADD2  the tensor as stored / the sum of two (a lin_z bias folded into the bias before it); count floats.
#include "pny_common.h"

namespace pny {

__global__ __launch_bounds__(256) void repack_kernel(const PackJob* __restrict__ jobs, unsigned* range_flag) {
    bool out_of_range = false;   // a weight that has no f16 representation (or a NaN): PNY_RANGE_WEIGHT
    const PackJob jb = jobs[blockIdx.y];
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < jb.count; i += stride) {
        if (jb.kind == PACK_COPY) {
            jb.dst[i] = jb.src[i];
        } else if (jb.kind == PACK_ADD2) {
            jb.dst[i] = jb.src[i] + jb.src2[i];
        } else if (jb.kind == PACK_NTT) {  // transposed block of the stacked lin_z^T: dst already points at the
            const int l = (int)(i & 63);   // block's first k-iteration; n_out = d_latent, k_in = 512, k_pad = total K
            const int jl = (int)((i >> 6) % (jb.k_in / 8)), nt = (int)((i >> 6) / (jb.k_in / 8));
            const int c = 32 * nt + (l & 31), f = 8 * jl + 4 * (l >> 5);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = jb.src[(size_t)(f + r) * jb.n_out + c];
            reinterpret_cast<float4*>(jb.dst)[((size_t)nt * (jb.k_pad / 8) + jl) * 64 + l] = make_float4(v[0], v[1], v[2], v[3]);
        } else if (jb.kind == PACK_H2 || jb.kind == PACK_H2T || jb.kind == PACK_H2O) {   // [16-k step][n-tile][plane][lane] x 8 halves
            // n-tiles per step: the 16 of a 512-row matrix, or lin_out's one or two (PACK_H2O: rows past n_out are zero)
            const int ntn = jb.kind == PACK_H2O ? (jb.n_out > 32 ? 2 : 1) : 16;
            const int l = (int)(i & 63), p = (int)((i >> 6) & 1), nt = (int)((i >> 7) % ntn), j = (int)((i >> 7) / ntn);
            const int row = 32 * nt + (l & 31), col = 16 * j + 8 * (l >> 5);
            const bool row_ok = jb.kind != PACK_H2O || row < jb.n_out;
            typedef _Float16 h8 __attribute__((ext_vector_type(8)));
            h8 o;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                // PACK_H2T: the matrix is W^T, element (row, col + r) = W[col + r][row], W is (n_out x k_in)
                const float w = jb.kind == PACK_H2T ? ((col + r < jb.n_out) ? jb.src[(size_t)(col + r) * jb.k_in + row] : 0.f)
                                                    : ((row_ok && col + r < jb.k_in) ? jb.src[(size_t)row * jb.k_in + col + r] : 0.f);
                out_of_range |= !(fabsf(w) <= 65504.0f);
                const _Float16 w1 = (_Float16)w;
                o[r] = p == 0 ? w1 : (_Float16)(w - (float)w1);
            }
            reinterpret_cast<h8*>(jb.dst)[i] = o;
        } else if (jb.kind == PACK_H1) {   // plane 0 of a PACK_H2 image (src): [16-k step][n-tile 0..15][lane] x 8 halves
            reinterpret_cast<uint4*>(jb.dst)[i] = reinterpret_cast<const uint4*>(jb.src)[(i >> 6) * 128 + (i & 63)];
        } else {
            const int l = (int)(i & 63);
            const int J = jb.k_pad / 8;
            int j, nt;
            if (jb.kind == PACK_NT) {   // [n-tile][k-iteration][lane]
                j = (int)((i >> 6) % J);
                nt = (int)((i >> 6) / J);
            } else {                    // [k-iteration][n-tile 0..15][lane]
                nt = (int)((i >> 6) & 15);
                j = (int)(i >> 10);
            }
            const int row = 32 * nt + (l & 31), col = 8 * j + 4 * (l >> 5);
            float v[4];
            if (jb.kind == PACK_AT) {   // matrix = W^T: element (row, col + r) = W[col + r][row], W is (n_out x k_in)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (col + r < jb.n_out) ? jb.src[(size_t)(col + r) * jb.k_in + row] : 0.f;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (col + r < jb.k_in) ? jb.src[(size_t)row * jb.k_in + col + r] : 0.f;
            }
            reinterpret_cast<float4*>(jb.dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    if (out_of_range) range_report(range_flag, 4u);
}

void launch_repack(const PackJob* jobs_dev, int n_jobs, long long max_elems, hipStream_t st, unsigned* range_flag) {
    if (n_jobs <= 0) return;
    long long bx = (max_elems + 255) / 256;
    if (bx > 256) bx = 256;   // grid-stride beyond 64 K elements per job
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(repack_kernel, dim3((unsigned)bx, (unsigned)n_jobs), dim3(256), 0, st, jobs_dev, range_flag);
}

}  // namespace pny
