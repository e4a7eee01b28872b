// Mesh extraction on the device (conventions and arithmetic in pny_recon.h; entry points in recon_api.hip): the grid front end
// of the reference's src/util/recon.py and marching cubes over a (X, Y, Z) fp32 sigma volume, giving an indexed, welded mesh
// whose bits do not depend on the run.  No atomics: every output element has one writer, and a vertex or triangle finds its
// place from an exclusive scan of per-point counts.
//
// Launches
//   pny_grid_points   ONE: grid_points_kernel, a thread per grid point of the slab, six stores.
//   pny_mc_count      TWO up to 1024 * 1024 points, FOUR above:
//       mc_count_kernel      a workgroup per tile of MC_SCAN_TILE = 1024 consecutive points, four per thread.  Per point the
//                            owned vertices (0..3, its +x, +y, +z edges) and the triangles of the cell whose low corner it is
//                            (0..5, MC_NUM_TRIS in LDS), packed into one word (a tile holds at most 3072 and 5120: 16 bits
//                            each) and scanned inside the tile: wave scan by shuffles, four wave sums through LDS.  Writes the
//                            per-point offsets inside the tile and the tile's sums.
//       mc_scan_sums_kernel  the same scan over the tile sums, vertices and triangles as two 32-bit scans; with more than 1024
//                            tiles it runs once per level (sums1 -> sums2, then sums2 by one workgroup), and
//       mc_add_kernel        adds the scanned sums2 back into sums1.
//     The level that one workgroup scans also writes the two totals.  Levels are separate launches: nothing is handed between
//     workgroups inside a launch.
//   pny_mc_emit       TWO: mc_vertices_kernel (a thread per point: its offset is voff[p] + sums1[p / 1024].v) and
//                     mc_triangles_kernel (a thread per cell, the case table in LDS; a triangle corner on table edge e is the
//                     vertex of e's owner: the owner's offset plus the rank of e's axis among the owner's cut edges, recomputed
//                     from the owner's sigma and its three neighbours').
// Every kernel runs RECON_THREADS = 256 threads on at most RECON_MAX_BLOCKS workgroups and strides over the rest.  All are bound
// by memory traffic: count and the emits read the volume (eight, four and eight cached loads per point), the offsets are 8
// bytes per point.
#include <hip/hip_runtime.h>

#include "pny_recon.h"

#define MC_TABLE_STORAGE __attribute__((aligned(16))) __constant__ const
#include "mc_table.h"

namespace pny {
namespace {

static_assert(RECON_THREADS == 256 && RECON_THREADS % 64 == 0, "four waves per workgroup");
static_assert(MC_ROW == 16, "a table row is one 16-byte load");
static_assert(3 * MC_SCAN_TILE < 65536 && MC_MAX_TRIS * MC_SCAN_TILE < 65536, "a tile's counts fit 16 bits each");

__global__ __launch_bounds__(RECON_THREADS) void grid_points_kernel(GridArgs a) {
    const int64_t n = a.i1 - a.i0;
    const int64_t yz = (int64_t)a.sy * a.sz;
    for (int64_t t = (int64_t)blockIdx.x * RECON_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * RECON_THREADS) {
        const int64_t i = a.i0 + t;
        const int ix = (int)(i / yz);
        const int r = (int)(i - (int64_t)ix * yz);
        const int iy = r / a.sz, iz = r - iy * a.sz;
        const float x = grid_coord(ix, a.sx, a.lo[0], a.step[0], a.hi[0]);
        const float y = grid_coord(iy, a.sy, a.lo[1], a.step[1], a.hi[1]);
        const float z = grid_coord(iz, a.sz, a.lo[2], a.step[2], a.hi[2]);
        float dx, dy, dz;
        grid_dir(x, y, z, dx, dy, dz);
        float* p = a.xyz + 3 * t;
        float* d = a.dirs + 3 * t;
        p[0] = x, p[1] = y, p[2] = z;
        d[0] = dx, d[1] = dy, d[2] = dz;
    }
}

// Exclusive scan of one word per thread over the workgroup; `total` is the workgroup's sum.  Two barriers.
__device__ __forceinline__ unsigned block_scan(unsigned x, unsigned* wave_sums, unsigned& total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    unsigned incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    unsigned base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RECON_THREADS / 64; ++w) {
        const unsigned s = wave_sums[w];
        base += w < wave ? s : 0u;
        all += s;
    }
    __syncthreads();       // wave_sums is free for the next call
    total = all;
    return base + incl - x;
}

struct Point {
    int x, y, z;
};

__device__ __forceinline__ Point point_of(unsigned p, const McDims& d) {
    Point q;
    const unsigned r = p / (unsigned)d.z;
    q.z = (int)(p - r * (unsigned)d.z);
    q.x = (int)(r / (unsigned)d.y);
    q.y = (int)(r - (unsigned)q.x * (unsigned)d.y);
    return q;
}

// which of point p's +x, +y, +z edges are cut: bit 0, 1, 2
__device__ __forceinline__ unsigned owned_cuts(const float* sigma, unsigned p, const Point& q, const McDims& d, float iso) {
    const bool in = mc_inside(sigma[p], iso);
    unsigned m = 0;
    if (q.x + 1 < d.x && mc_inside(sigma[p + (unsigned)d.y * (unsigned)d.z], iso) != in) m |= 1u;
    if (q.y + 1 < d.y && mc_inside(sigma[p + (unsigned)d.z], iso) != in) m |= 2u;
    if (q.z + 1 < d.z && mc_inside(sigma[p + 1u], iso) != in) m |= 4u;
    return m;
}

// case index of the cell whose low corner is p (the cell exists: every coordinate below its dimension - 1)
__device__ __forceinline__ unsigned cell_case(const float* sigma, unsigned p, const McDims& d, float iso) {
    const unsigned sx = (unsigned)d.y * (unsigned)d.z, sy = (unsigned)d.z;
    unsigned c = 0;
#pragma unroll
    for (unsigned k = 0; k < 8; ++k)
        c |= mc_inside(sigma[p + (k & 1u) * sx + ((k >> 1) & 1u) * sy + (k >> 2)], iso) ? (1u << k) : 0u;
    return c;
}

__device__ __forceinline__ bool has_cell(const Point& q, const McDims& d) { return q.x + 1 < d.x && q.y + 1 < d.y && q.z + 1 < d.z; }

__global__ __launch_bounds__(RECON_THREADS) void mc_count_kernel(McArgs a, unsigned n_tiles) {
    __shared__ unsigned char num_tris[256];
    __shared__ unsigned wave_sums[RECON_THREADS / 64];
    num_tris[threadIdx.x] = MC_NUM_TRIS[threadIdx.x];
    __syncthreads();
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const unsigned p0 = tile * (unsigned)MC_SCAN_TILE + threadIdx.x * (unsigned)MC_SCAN_ITEMS;
        unsigned c[MC_SCAN_ITEMS], mine = 0;
#pragma unroll
        for (int j = 0; j < MC_SCAN_ITEMS; ++j) {
            const unsigned p = p0 + (unsigned)j;
            c[j] = 0;
            if (p < a.n_points) {
                const Point q = point_of(p, a.d);
                c[j] = (unsigned)__popc(owned_cuts(a.sigma, p, q, a.d, a.iso));
                if (has_cell(q, a.d)) c[j] |= (unsigned)num_tris[cell_case(a.sigma, p, a.d, a.iso)] << 16;
            }
            mine += c[j];
        }
        unsigned total;
        unsigned before = block_scan(mine, wave_sums, total);
#pragma unroll
        for (int j = 0; j < MC_SCAN_ITEMS; ++j) {
            const unsigned p = p0 + (unsigned)j;
            if (p < a.n_points) a.voff[p] = before & 0xffffu, a.toff[p] = before >> 16;
            before += c[j];
        }
        if (threadIdx.x == 0) a.sums1[tile].v = total & 0xffffu, a.sums1[tile].t = total >> 16;
    }
}

// Exclusive scan of s[0 .. n) in place, tile by tile; next[tile] = the tile's sums (or null); counts = the sums of tile 0 as
// two int32 (or null: only the launch of one tile passes it).
__global__ __launch_bounds__(RECON_THREADS) void mc_scan_sums_kernel(McCount* s, unsigned n, McCount* next, int32_t* counts) {
    __shared__ unsigned wave_sums[RECON_THREADS / 64];
    const unsigned n_tiles = (n + MC_SCAN_TILE - 1) / MC_SCAN_TILE;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const unsigned i0 = tile * (unsigned)MC_SCAN_TILE + threadIdx.x * (unsigned)MC_SCAN_ITEMS;
        McCount c[MC_SCAN_ITEMS];
        unsigned mv = 0, mt = 0;
#pragma unroll
        for (int j = 0; j < MC_SCAN_ITEMS; ++j) {
            c[j].v = c[j].t = 0;
            if (i0 + (unsigned)j < n) c[j] = s[i0 + (unsigned)j];
            mv += c[j].v, mt += c[j].t;
        }
        unsigned tv, tt;
        unsigned bv = block_scan(mv, wave_sums, tv);
        unsigned bt = block_scan(mt, wave_sums, tt);
#pragma unroll
        for (int j = 0; j < MC_SCAN_ITEMS; ++j) {
            if (i0 + (unsigned)j < n) s[i0 + (unsigned)j].v = bv, s[i0 + (unsigned)j].t = bt;
            bv += c[j].v, bt += c[j].t;
        }
        if (threadIdx.x == 0) {
            if (next) next[tile].v = tv, next[tile].t = tt;
            if (counts && tile == 0) counts[0] = (int32_t)tv, counts[1] = (int32_t)tt;
        }
    }
}

// s[i] += up[i / MC_SCAN_TILE]
__global__ __launch_bounds__(RECON_THREADS) void mc_add_kernel(McCount* s, unsigned n, const McCount* up) {
    for (unsigned i = blockIdx.x * (unsigned)RECON_THREADS + threadIdx.x; i < n; i += gridDim.x * (unsigned)RECON_THREADS) {
        const McCount u = up[i / (unsigned)MC_SCAN_TILE];
        McCount c = s[i];
        c.v += u.v, c.t += u.t;
        s[i] = c;
    }
}

__global__ __launch_bounds__(RECON_THREADS) void mc_vertices_kernel(McArgs a) {
    const unsigned sx = (unsigned)a.d.y * (unsigned)a.d.z, sy = (unsigned)a.d.z;
    for (unsigned p = blockIdx.x * (unsigned)RECON_THREADS + threadIdx.x; p < a.n_points; p += gridDim.x * (unsigned)RECON_THREADS) {
        const Point q = point_of(p, a.d);
        const unsigned m = owned_cuts(a.sigma, p, q, a.d, a.iso);
        if (!m) continue;
        int64_t at = (int64_t)a.voff[p] + (int64_t)a.sums1[p / (unsigned)MC_SCAN_TILE].v;
        const float s0 = a.sigma[p];
        const float fx = (float)q.x, fy = (float)q.y, fz = (float)q.z;
        if ((m & 1u) && at < a.n_vertices) {
            float* v = a.vertices + 3 * at;
            v[0] = mc_cut(q.x, s0, a.sigma[p + sx], a.iso), v[1] = fy, v[2] = fz;
        }
        at += m & 1u;
        if ((m & 2u) && at < a.n_vertices) {
            float* v = a.vertices + 3 * at;
            v[0] = fx, v[1] = mc_cut(q.y, s0, a.sigma[p + sy], a.iso), v[2] = fz;
        }
        at += (m >> 1) & 1u;
        if ((m & 4u) && at < a.n_vertices) {
            float* v = a.vertices + 3 * at;
            v[0] = fx, v[1] = fy, v[2] = mc_cut(q.z, s0, a.sigma[p + 1u], a.iso);
        }
    }
}

__global__ __launch_bounds__(RECON_THREADS) void mc_triangles_kernel(McArgs a) {
    __shared__ uint4 rows[256];                     // MC_TRI_TABLE, a row per 16 bytes
    rows[threadIdx.x] = reinterpret_cast<const uint4*>(&MC_TRI_TABLE[0][0])[threadIdx.x];
    __syncthreads();
    const signed char* table = reinterpret_cast<const signed char*>(rows);
    const unsigned sx = (unsigned)a.d.y * (unsigned)a.d.z, sy = (unsigned)a.d.z;
    for (unsigned p = blockIdx.x * (unsigned)RECON_THREADS + threadIdx.x; p < a.n_points; p += gridDim.x * (unsigned)RECON_THREADS) {
        const Point q = point_of(p, a.d);
        if (!has_cell(q, a.d)) continue;
        const unsigned cs = cell_case(a.sigma, p, a.d, a.iso);
        const signed char* row = table + cs * MC_ROW;
        if (row[0] < 0) continue;
        const int64_t t0 = (int64_t)a.toff[p] + (int64_t)a.sums1[p / (unsigned)MC_SCAN_TILE].t;
        for (int k = 0; k < 3 * MC_MAX_TRIS && row[k] >= 0; ++k) {
            const int64_t at = 3 * t0 + k;
            if (at >= 3 * a.n_triangles) break;
            int dx, dy, dz, axis;
            mc_edge((int)row[k], dx, dy, dz, axis);
            const unsigned o = p + (unsigned)dx * sx + (unsigned)dy * sy + (unsigned)dz;
            Point oq;
            oq.x = q.x + dx, oq.y = q.y + dy, oq.z = q.z + dz;
            const unsigned m = owned_cuts(a.sigma, o, oq, a.d, a.iso);
            const unsigned rank = (unsigned)__popc(m & ((1u << axis) - 1u));
            a.triangles[at] = (int32_t)(a.voff[o] + a.sums1[o / (unsigned)MC_SCAN_TILE].v + rank);
        }
    }
}

inline unsigned capped(int64_t blocks) { return (unsigned)(blocks < (int64_t)RECON_MAX_BLOCKS ? blocks : (int64_t)RECON_MAX_BLOCKS); }

}  // namespace

void launch_grid_points(const GridArgs& a, hipStream_t st) {
    const int64_t n = a.i1 - a.i0;
    hipLaunchKernelGGL(grid_points_kernel, dim3(capped((n + RECON_THREADS - 1) / RECON_THREADS)), dim3(RECON_THREADS), 0, st, a);
}

// count + tile scan, then the scan of the sums level by level; counts = int32[2] {vertices, triangles}
void launch_mc_count(const McArgs& a, const McLayout& l, McCount* sums2, int32_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(mc_count_kernel, dim3(capped(l.n1)), dim3(RECON_THREADS), 0, st, a, (unsigned)l.n1);
    if (l.n2 == 0) {
        hipLaunchKernelGGL(mc_scan_sums_kernel, dim3(1), dim3(RECON_THREADS), 0, st, a.sums1, (unsigned)l.n1, (McCount*)nullptr, counts);
        return;
    }
    hipLaunchKernelGGL(mc_scan_sums_kernel, dim3(capped(l.n2)), dim3(RECON_THREADS), 0, st, a.sums1, (unsigned)l.n1, sums2, (int32_t*)nullptr);
    hipLaunchKernelGGL(mc_scan_sums_kernel, dim3(1), dim3(RECON_THREADS), 0, st, sums2, (unsigned)l.n2, (McCount*)nullptr, counts);
    hipLaunchKernelGGL(mc_add_kernel, dim3(capped((l.n1 + RECON_THREADS - 1) / RECON_THREADS)), dim3(RECON_THREADS), 0, st, a.sums1,
                       (unsigned)l.n1, (const McCount*)sums2);
}

void launch_mc_vertices(const McArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(mc_vertices_kernel, dim3(capped(((int64_t)a.n_points + RECON_THREADS - 1) / RECON_THREADS)), dim3(RECON_THREADS), 0,
                       st, a);
}

void launch_mc_triangles(const McArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(mc_triangles_kernel, dim3(capped(((int64_t)a.n_points + RECON_THREADS - 1) / RECON_THREADS)), dim3(RECON_THREADS),
                       0, st, a);
}

}  // namespace pny
