// Conventions and arithmetic of early ray termination in depth segments (termination.hip and the segment kernels of
// occupancy.hip; entry points in occupancy_api.hip; the segment loop of pny_render in render_api.hip).  A scene with the mode on
// (pny_scene_set_termination) stops evaluating the MLP along a ray once the ray has become opaque.  tests/termination_ref.py
// restates every line of this in numpy.
//
//   setting     a threshold t_min with 0 < t_min < 1 and a segment count S in 1 .. 16; t_min == 0 switches the mode off.  It is a
//               rendering option, not a property of the encoded object: nothing that changes the scene's latent or cameras
//               clears it (the occupancy grid IS cleared by those).
//   segments    a pass with K samples per ray has S' = min(S, K) segments; segment j holds the sample indices
//               [floor(j K / S'), floor((j + 1) K / S')).  The coarse pass has K = n_coarse, the fine pass K = n_coarse + n_fine
//               (its samples are sorted by depth).
//   T           the transmittance at a boundary b is the product of (1 - alpha_k + 1e-10f) over k < b, with
//               alpha_k = 1 - expf(-delta_k * fmaxf(sigma_k, 0)), delta_k = z_{k+1} - z_k and the last delta = far - z_last, all
//               fp32: composite_kernel's own arithmetic (render_kernels.hip).  sigma_k is the MASKED per-sample output: a sample
//               that was not evaluated has sigma = 0 and a factor of exactly 1.  The order of the multiplications is free.
//   alive       every ray is alive in segment 0; alive in segment j + 1 iff alive in segment j and !(T_b < t_min) at the
//               boundary b between them.  A NaN transmittance keeps the ray alive; a ray that dies stays dead.
//   kept        a sample is evaluated iff its ray is alive in its segment and, with a grid attached, occ_keep accepts it; with no
//               grid every cell counts as occupied.
//   contract    on the same rays and draws a terminated pny_render gives what the default render gives if the MLP's
//               (r, g, b, sigma) at every sample that was not kept were (0, 0, 0, 0) before the composite, in both passes (the
//               fine depths follow from the masked coarse weights).  Composite and fine sampling run unchanged.
//   host waits  ONE per issued segment: the kept count and the count of alive rays are read together into a pinned pair before
//               the compact rows are reserved.  A pass stops issuing segments once no ray is alive (the remaining columns are
//               zeroed by one 2-D memset).  With the mode off and a grid attached the path and its two waits are the grid's own.
//   memory      on top of a culled pass (pny_occupancy.h): 4 bytes (T) and 1 byte (alive) per ray; slot, tile sums and compact
//               rows are sized by the LARGEST segment, n * ceil(K / S') samples, and reused by every segment.
// It also compiles for the host (__host__ / __device__ defined away).
#pragma once
#include <math.h>
#include <stdint.h>

namespace pny {

constexpr int TERM_MAX_SEGMENTS = 16;

__host__ __device__ inline int term_segments(int K, int S) { return S < K ? S : K; }
// the first sample index of segment j of S' (j = S': K)
__host__ __device__ inline int term_bound(int K, int Sp, int j) { return (int)((int64_t)j * K / Sp); }

// (1 - alpha + 1e-10f) of one sample: composite_kernel's arithmetic
__host__ __device__ inline float term_factor(float sigma, float z, float znext) {
    const float delta = znext - z;
    const float alpha = 1.0f - expf(-delta * fmaxf(sigma, 0.f));
    return 1.0f - alpha + 1e-10f;
}

// the product of the factors of samples [k_begin, k_end) of one ray, in ascending order; z (K), samp (K, 4)
__host__ __device__ inline float term_product(const float* z, const float* samp, int K, int k_begin, int k_end, float far) {
    float p = 1.0f;
    for (int k = k_begin; k < k_end; ++k) p *= term_factor(samp[4 * k + 3], z[k], k + 1 < K ? z[k + 1] : far);
    return p;
}

__host__ __device__ inline bool term_alive(bool alive, float T, float t_min) { return alive && !(T < t_min); }

struct TermUpdateArgs {
    const float* rays;       // (n, 8): far is column 7
    const float* z;          // (n, K)
    const float* samp;       // (n, K, 4), 16-byte aligned
    int64_t n;
    int K, k_begin, k_end;
    float t_min;
    float* T;                // (n): carried
    uint8_t* alive;          // (n): carried
    unsigned long long* alive_count;   // null, or the count of rays alive after this call (zeroed before the launch)
};

}  // namespace pny
