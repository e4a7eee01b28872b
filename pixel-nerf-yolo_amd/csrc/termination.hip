// Early ray termination on the device (conventions and arithmetic in pny_termination.h; entry points in occupancy_api.hip, the
// segment loop of pny_render in render_api.hip; the segment forms of classify / gather / expand are in occupancy.hip beside the
// kernels they restate).  Wave64.
//
// Launches
//   transmittance update  ONE: termination_update_kernel.  One wavefront per ray and step, one sample per lane, as
//                         composite_kernel reads a ray: the factor (1 - alpha + 1e-10f) per lane, their product by a butterfly
//                         of shuffles, segments longer than 64 samples chunk by chunk with the product carried.  Lane 0
//                         multiplies the ray's carried T and clears its alive byte.  Every ray has one writer, and a product
//                         over a butterfly is the same on every run, so the same input gives the same bits.  A wavefront
//                         strides over its rays and counts the alive ones in a register: the alive count is one integer atomic
//                         add per wavefront.
// TERM_THREADS = 256 threads on at most RECON_MAX_BLOCKS workgroups.
#include <hip/hip_runtime.h>

#include "pny_recon.h"
#include "pny_termination.h"

namespace pny {
namespace {

constexpr int TERM_THREADS = 256;
constexpr int TERM_WAVES = TERM_THREADS / 64;

__device__ __forceinline__ float wave_product(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x *= __shfl_xor(x, o, 64);
    return x;
}

__global__ __launch_bounds__(TERM_THREADS) void termination_update_kernel(TermUpdateArgs a) {
    const int lane = (int)threadIdx.x & 63;
    unsigned alive_here = 0;   // (lane 0 counts)
    for (int64_t ray = (int64_t)blockIdx.x * TERM_WAVES + (threadIdx.x >> 6); ray < a.n; ray += (int64_t)gridDim.x * TERM_WAVES) {
        const float far = a.rays[ray * 8 + 7];
        const float* zr = a.z + ray * a.K;
        const float4* sr = reinterpret_cast<const float4*>(a.samp) + ray * a.K;
        float prod = 1.0f;
        for (int k0 = a.k_begin; k0 < a.k_end; k0 += 64) {
            const int k = k0 + lane;
            float f = 1.0f;
            if (k < a.k_end) f = term_factor(sr[k].w, zr[k], k + 1 < a.K ? zr[k + 1] : far);
            prod *= wave_product(f);
        }
        if (lane == 0) {
            const float T = a.T[ray] * prod;
            const bool alive = term_alive(a.alive[ray] != 0, T, a.t_min);
            a.T[ray] = T;
            a.alive[ray] = alive ? 1 : 0;
            alive_here += alive ? 1u : 0u;
        }
    }
    if (a.alive_count && lane == 0 && alive_here) atomicAdd(a.alive_count, (unsigned long long)alive_here);
}

}  // namespace

void launch_termination_update(const TermUpdateArgs& a, hipStream_t st) {
    int64_t blocks = (a.n + TERM_WAVES - 1) / TERM_WAVES;
    if (blocks < 1) blocks = 1;
    if (blocks > (int64_t)RECON_MAX_BLOCKS) blocks = RECON_MAX_BLOCKS;
    hipLaunchKernelGGL(termination_update_kernel, dim3((unsigned)blocks), dim3(TERM_THREADS), 0, st, a);
}

}  // namespace pny
