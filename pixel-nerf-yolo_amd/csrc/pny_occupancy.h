// Conventions and arithmetic of the per-object occupancy grid (occupancy.hip; entry points in occupancy_api.hip): a bitfield over
// the cells of a sigma volume, and the test that sends a depth sample of a ray to its cell.  A scene with a grid attached
// (pny_scene_set_occupancy) evaluates the MLP at the kept samples only.  tests/occupancy_ref.py restates every line of this in
// numpy.
//
//   contract    a culled pny_render gives, on the same rays and draws, what the render without the grid gives if the MLP's
//               (r, g, b, sigma) at every rejected sample were (0, 0, 0, 0) before the composite, in both passes (the fine
//               pass's samples follow from the masked coarse weights).  Composite and fine sampling run unchanged.
//   host waits  TWO per culled pny_render, one per pass: the kept count is read into a pinned word before the compact rows are
//               reserved and the MLP is launched on exactly that many points.
//   cells       a volume of (X, Y, Z) grid points, x slowest, z fastest (pny_recon.h), has (X - 1, Y - 1, Z - 1) cells, the
//               marching-cubes cells.  Flat index f = (ix (Y - 1) + iy) (Z - 1) + iz; cell f is bit f & 31 of uint32 word
//               f >> 5; bits past the last cell are 0.
//   occupied    a corner is occupied when !(sigma <= thresh): a NaN is occupied.  With a second volume a corner is occupied when
//               it is in either (the max of the two, a NaN in either counting).  A cell is raw-occupied when any of its 8
//               corners is -- a trilinear interpolant never exceeds its corners -- and occupied when any cell within Chebyshev
//               distance `dilate` (0 .. 4) is raw-occupied: equivalently, when any grid point of the box
//               [i - dilate, i + dilate + 1] per axis, clipped to the volume, is an occupied corner.
//   sample      p_a = fmaf(z, d_a, o_a), the fused form written out so that host and device agree whatever a compiler contracts;
//               t_a = (p_a - lo_a) * inv_a with lo_a = (float)c1_a and inv_a = (float)((double)cells_a / (c2_a - c1_a)),
//               subtraction and multiplication rounded separately; inside iff 0 <= t_a < (float)cells_a on all three axes (a
//               NaN is outside); i_a = (int)t_a.  An outside sample is kept when outside_empty == 0, rejected when it is 1.
//   slot        the rank of a kept sample among the kept samples in ascending sample order, -1 for a rejected one.
//   memory      the bitfield is one bit per cell (256 KB at 128^3); a culled pass holds 4 bytes per sample (slot), 4 per 1024
//               samples (tile sums) and 40 bytes per KEPT sample (xyz, dirs and the MLP's output of the compact rows).
// It also compiles for the host (__host__ / __device__ defined away).
#pragma once
#include <math.h>
#include <stdint.h>

#include "pny_recon.h"

namespace pny {

constexpr int OCC_THREADS = RECON_THREADS;                 // every kernel of occupancy.hip: four waves
constexpr int OCC_TILE = MC_SCAN_TILE;                     // samples per workgroup of the classification and per scan level
constexpr int OCC_TILE_STEPS = OCC_TILE / OCC_THREADS;     // a thread ranks one sample per step
constexpr int OCC_MAX_DILATE = 4;
// two levels of tile sums, the second scanned by one workgroup: at most OCC_TILE^3 samples
constexpr int64_t OCC_MAX_SAMPLES = (int64_t)OCC_TILE * OCC_TILE * OCC_TILE;

__host__ __device__ inline int64_t occ_cells(int x, int y, int z) { return (int64_t)(x - 1) * (y - 1) * (z - 1); }
__host__ __device__ inline int64_t occ_words(int64_t cells) { return (cells + 31) >> 5; }

// !(sigma <= thresh): true for a NaN
__host__ __device__ inline bool occ_corner(float s, float thresh) { return !(s <= thresh); }

struct OccBuildArgs {
    const float* sigma;      // (X, Y, Z)
    const float* sigma2;     // the same shape, or null
    McDims d;
    float thresh;
    int dilate;
    uint32_t* bits;          // occ_words(cells) words
    unsigned long long* occupied;   // null, or the count of occupied cells (zeroed before the launch)
    uint32_t n_words;
};

// cell (ix, iy, iz) after dilation: any occupied corner in the clipped box of grid points around it
__host__ __device__ inline bool occ_cell(const OccBuildArgs& a, int ix, int iy, int iz) {
    const int x0 = ix - a.dilate < 0 ? 0 : ix - a.dilate, x1 = ix + a.dilate + 1 > a.d.x - 1 ? a.d.x - 1 : ix + a.dilate + 1;
    const int y0 = iy - a.dilate < 0 ? 0 : iy - a.dilate, y1 = iy + a.dilate + 1 > a.d.y - 1 ? a.d.y - 1 : iy + a.dilate + 1;
    const int z0 = iz - a.dilate < 0 ? 0 : iz - a.dilate, z1 = iz + a.dilate + 1 > a.d.z - 1 ? a.d.z - 1 : iz + a.dilate + 1;
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y) {
            const uint32_t row = ((uint32_t)x * (uint32_t)a.d.y + (uint32_t)y) * (uint32_t)a.d.z;
            for (int z = z0; z <= z1; ++z) {
                if (occ_corner(a.sigma[row + (uint32_t)z], a.thresh)) return true;
                if (a.sigma2 && occ_corner(a.sigma2[row + (uint32_t)z], a.thresh)) return true;
            }
        }
    return false;
}

// word w of the bitfield: cells 32 w .. 32 w + 31, the bits past the last cell 0
__host__ __device__ inline uint32_t occ_word(const OccBuildArgs& a, uint32_t w) {
    const uint32_t cy = (uint32_t)(a.d.y - 1), cz = (uint32_t)(a.d.z - 1);
    const uint32_t cells = (uint32_t)(a.d.x - 1) * cy * cz;
    uint32_t bits = 0;
    for (uint32_t b = 0; b < 32u; ++b) {
        const uint32_t f = w * 32u + b;
        if (f >= cells) break;
        const uint32_t r = f / cz;
        const int iz = (int)(f - r * cz), ix = (int)(r / cy);
        const int iy = (int)(r - (uint32_t)ix * cy);
        if (occ_cell(a, ix, iy, iz)) bits |= 1u << b;
    }
    return bits;
}

// the grid as the classification reads it
struct OccGrid {
    const uint32_t* bits;
    int cells[3];            // X - 1, Y - 1, Z - 1
    float lo[3], inv[3], hi[3];   // (float)c1, (float)((double)cells / (c2 - c1)), (float)cells
    int outside_empty;
};

inline void occ_grid_axes(OccGrid& g, const int32_t* dims, const double* c1, const double* c2) {
    for (int a = 0; a < 3; ++a) {
        g.cells[a] = dims[a] - 1;
        g.lo[a] = (float)c1[a];
        g.inv[a] = (float)((double)g.cells[a] / (c2[a] - c1[a]));
        g.hi[a] = (float)g.cells[a];
    }
}

// flat cell of the sample at depth z of the ray (o, d), or -1 outside the grid
__host__ __device__ inline int64_t occ_sample_cell(const OccGrid& g, const float* o, const float* d, float z) {
    int i[3];
    for (int a = 0; a < 3; ++a) {
        const float p = fmaf(z, d[a], o[a]);
        const float q = p - g.lo[a];
        const float t = q * g.inv[a];
        if (!(t >= 0.0f && t < g.hi[a])) return -1;
        i[a] = (int)t;
    }
    return ((int64_t)i[0] * g.cells[1] + i[1]) * g.cells[2] + i[2];
}

__host__ __device__ inline bool occ_keep(const OccGrid& g, const float* o, const float* d, float z) {
    const int64_t f = occ_sample_cell(g, o, d, z);
    if (f < 0) return g.outside_empty == 0;
    return (g.bits[f >> 5] >> (unsigned)(f & 31)) & 1u;
}

// Workspace of a classification of n samples: per tile of OCC_TILE samples the kept samples before it (sums1: n1 entries) and,
// where n1 > OCC_TILE, per tile of sums1 its sum (sums2: n2 <= OCC_TILE entries).  Every part starts on a 256-byte boundary.
struct OccLayout {
    int64_t n1, n2;          // n2 = 0: sums1 is scanned by one workgroup
    size_t sums1, sums2;     // uint32[n1], uint32[n2]
    size_t bytes;
};

inline OccLayout occ_layout(int64_t n_samples) {
    OccLayout l;
    l.n1 = (n_samples + OCC_TILE - 1) / OCC_TILE;
    l.n2 = l.n1 > OCC_TILE ? (l.n1 + OCC_TILE - 1) / OCC_TILE : 0;
    l.sums1 = 0;
    l.sums2 = mc_align((size_t)l.n1 * 4);
    l.bytes = l.sums2 + mc_align((size_t)l.n2 * 4);
    if (l.bytes == 0) l.bytes = 256;
    return l;
}

struct OccClassifyArgs {
    OccGrid g;
    const float* rays;       // (n, 8), rows 16-byte aligned
    const float* z;          // (n, K)
    uint32_t n_samples, K;
    int32_t* slot;           // (n, K)
    uint32_t* sums1;
};

// The classification of the columns [k_begin, k_begin + Ks) of the (n, K) depths (a depth segment: pny_termination.h).
// g.bits null: every cell occupied; alive null: every ray alive, else the rays with alive[ray] == 0 reject all of theirs.
struct OccSegmentArgs {
    OccGrid g;
    const float* rays;       // (n, 8), rows 16-byte aligned
    const float* z;          // (n, K)
    const uint8_t* alive;    // (n) or null
    uint32_t n_samples;      // n * Ks
    uint32_t K, k_begin, Ks;
    int32_t* slot;           // (n, Ks)
    uint32_t* sums1;
};

__host__ __device__ inline bool occ_keep_segment(const OccSegmentArgs& a, uint32_t ray, const float* o, const float* d, float z) {
    if (a.alive && a.alive[ray] == 0) return false;
    return a.g.bits ? occ_keep(a.g, o, d, z) : true;
}

}  // namespace pny
