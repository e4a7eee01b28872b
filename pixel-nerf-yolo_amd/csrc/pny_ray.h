// The ray of one pixel through a pinhole camera, device code shared by gen_rays_kernel, train_batch_kernel
// (render_kernels.hip) and resident_batch_kernel (resident.hip): one copy of the arithmetic, so a sampled training ray carries
// the bits of the same pixel of a full gen_rays call whichever kernel produced it.
//   cam16: [M 3x3 row-major (pixel-dir -> world), origin(3), fx, fy, cx, cy]
#pragma once
#include <hip/hip_runtime.h>

namespace pny {

// cam16 of a cam->world pose P (4 x 4 row-major) and its intrinsics
__device__ __forceinline__ void cam16_from_pose(const float* P, float fx, float fy, float cx, float cy, float* c) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) c[3 * r + q] = P[4 * r + q];
        c[9 + r] = P[4 * r + 3];
    }
    c[12] = fx, c[13] = fy, c[14] = cx, c[15] = cy;
}

// The unit direction of pixel (x, y) in camera space (reference util.py:115-145, 240-278): normalize((x-cx)/fx, -(y-cy)/fy, -1)
__device__ __forceinline__ void pinhole_dir(const float* c, int x, int y, float& d0, float& d1, float& d2) {
    d0 = ((float)x - c[14]) / c[12];
    d1 = -(((float)y - c[15]) / c[13]);
    d2 = -1.0f;
    const float nrm = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    d0 /= nrm;
    d1 /= nrm;
    d2 /= nrm;
}

// The row [origin, M d, near, far], written as two 16-byte words
__device__ __forceinline__ void store_ray(const float* c, float d0, float d1, float d2, float znear, float zfar,
                                          float* row) {
    float4* o = reinterpret_cast<float4*>(row);  // hipMalloc / torch allocations: rows are 32-byte aligned
    o[0] = make_float4(c[9], c[10], c[11], c[0] * d0 + c[1] * d1 + c[2] * d2);
    o[1] = make_float4(c[3] * d0 + c[4] * d1 + c[5] * d2, c[6] * d0 + c[7] * d1 + c[8] * d2, znear, zfar);
}

}  // namespace pny
