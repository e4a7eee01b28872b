// Adam over every tensor of a parameter group in ONE launch (pny_optim_adam_step, optim_api.hip).
//
// Work: a device-resident table of chunks {tensor, element offset, count <= ADAM_CHUNK}, one workgroup per chunk.  Tensors range
// from 4 elements (a lin_out bias) to 2.4 M (a 512-channel 3 x 3 convolution); fixed-size chunks give every workgroup the same
// bounded amount of work whatever the tensor sizes are, and the hardware dispatcher balances them (a group is at most a few
// thousand chunks: 28 M parameters with the trunk trained = ~1800).
// Memory: purely bandwidth-bound, 4 streams in (parameter, gradient, both moments) and 3 out.  16-byte loads and stores
// wherever the chunk's four base pointers share their misalignment to 16 bytes (a scalar head of up to 3 elements brings all
// four to a boundary, a scalar tail takes count % 4); pointers that disagree take the scalar path for the whole chunk.
// No LDS, no atomics: every element is read and written by exactly one lane, so a step is bit-reproducible; the file is
// compiled with -ffp-contract=off (csrc/Makefile) and the operation order below is fixed (the two fmaf are explicit), so every build
// gives the same bits.
// Parameters and moments are fixed for the optimizer's life (AdamTensor); the gradient pointers change with every backward
// and are read from a host-pinned table that the launch owns until it has executed (optim_api.hip: ring of tables).
#include "pny_common.h"

namespace pny {

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamScalars& sc) {
    if (sc.weight_decay != 0.f) g = g + sc.weight_decay * p;
    // both moments with the product fused into the sum: one rounding fewer each.  exp_avg is then ATen's lerp_ bit for bit
    // (start + weight * (end - start), which the device compiler fuses), so its error against fp64 IS torch.optim.Adam's
    m = fmaf(g - m, sc.one_minus_beta1, m);
    v = fmaf(sc.one_minus_beta2 * g, g, v * sc.beta2);
    p = p - sc.step_size * m / (sqrtf(v) / sc.bc2_sqrt + sc.eps);
}

__device__ __forceinline__ void adam_scalar(float* p, const float* g, float* m, float* v, int i, const AdamScalars& sc) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update(pi, g[i], mi, vi, sc);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamTensor* __restrict__ tensors, const AdamChunk* __restrict__ chunks,
                                                         float* const* __restrict__ grads, int first, AdamScalars sc) {
    const AdamChunk c = chunks[blockIdx.x];
    const float* g_base = grads[c.tensor - first];
    if (!g_base) return;   // this tensor takes no step (no .grad, or it belongs to another launch of the group)
    const AdamTensor t = tensors[c.tensor];
    float* p = t.p + c.offset;
    float* m = t.m + c.offset;
    float* v = t.v + c.offset;
    const float* g = g_base + c.offset;
    const int n = c.count, tid = (int)threadIdx.x;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
    const bool same = ((unsigned)(reinterpret_cast<uintptr_t>(g) >> 2) & 3u) == mis &&
                      ((unsigned)(reinterpret_cast<uintptr_t>(m) >> 2) & 3u) == mis &&
                      ((unsigned)(reinterpret_cast<uintptr_t>(v) >> 2) & 3u) == mis;
    int head = n, body = 0;   // elements [0, head) scalar, [head, head + body) as float4, [head + body, n) scalar
    if (same) {
        head = (int)((4u - mis) & 3u);
        if (head > n) head = n;
        body = (n - head) & ~3;
    }
    for (int i = tid; i < head; i += 256) adam_scalar(p, g, m, v, i, sc);
#pragma unroll 4
    for (int i = head + 4 * tid; i < head + body; i += 4 * 256) {
        float4 pp = *reinterpret_cast<const float4*>(p + i);
        const float4 gg = *reinterpret_cast<const float4*>(g + i);
        float4 mm = *reinterpret_cast<const float4*>(m + i);
        float4 vv = *reinterpret_cast<const float4*>(v + i);
        adam_update(pp.x, gg.x, mm.x, vv.x, sc);
        adam_update(pp.y, gg.y, mm.y, vv.y, sc);
        adam_update(pp.z, gg.z, mm.z, vv.z, sc);
        adam_update(pp.w, gg.w, mm.w, vv.w, sc);
        *reinterpret_cast<float4*>(p + i) = pp;
        *reinterpret_cast<float4*>(m + i) = mm;
        *reinterpret_cast<float4*>(v + i) = vv;
    }
    for (int i = head + body + tid; i < n; i += 256) adam_scalar(p, g, m, v, i, sc);
}

void launch_adam(const AdamTensor* tensors_dev, const AdamChunk* chunks_dev, int n_chunks, float* const* grads, int first,
                 const AdamScalars& sc, hipStream_t st) {
    if (n_chunks <= 0) return;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, tensors_dev, chunks_dev, grads, first, sc);
}

}  // namespace pny
