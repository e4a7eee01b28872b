// The occupancy grid on the device (conventions and arithmetic in pny_occupancy.h; entry points in occupancy_api.hip, the culled
// passes of pny_render in render_api.hip): the bitfield from one or two sigma volumes, and the classify / gather / expand kernels that
// let a render evaluate the MLP at the kept samples only.  Wave64 throughout.  No atomics on the bits and none in the ranking:
// every output element has one writer, so the same input gives the same bits on every run.
//
// Launches
//   occupancy build     ONE: occupancy_build_kernel, a thread per 32-bit word (32 cells, a direct window of grid points per
//                       cell: at 128^3 and dilate 1 that is 64 cached loads per cell), one vector store per word; the occupied
//                       count by one integer atomic add of each wave's popcounts.
//   occupancy classify  THREE up to 1024 * 1024 samples, FIVE above:
//       occupancy_classify_kernel  a workgroup per tile of OCC_TILE = 1024 consecutive samples, a thread per sample and step.
//                                  The ray row is two 16-byte loads, the cell's word one 32-bit load; the keep flag is ranked
//                                  inside the wave by ballot / mbcnt, the 16 wave counts of a tile through LDS.  Writes the rank
//                                  inside the tile (or -1) and the tile's sum.
//       occupancy_scan_sums_kernel the exclusive scan of the tile sums, recon.hip's scheme restated for one word per entry: tile
//                                  by tile, with more than 1024 tiles once per level (sums1 -> sums2, then sums2 by one
//                                  workgroup) and occupancy_add_sums_kernel adds the scanned sums2 back.  The level that one
//                                  workgroup scans writes the kept count.
//       occupancy_add_kernel       slot[s] += sums1[s / 1024] for the kept samples.
//   gather              ONE: occupancy_gather_kernel, a thread per sample: a kept one writes its point o + z d (the arithmetic of
//                       mlp_core.h load_point, not the fused form of the classification) and the ray's d to its compact row.
//   expand              ONE: occupancy_expand_kernel, a thread per sample: 16 bytes, the compact row's or zeros.  The reads
//                       ascend with the sample index, so they coalesce.
//   depth segments      the *_segment_kernel forms of classify, gather and expand read and write the columns [k_begin, k_end) of
//                       the (n, K) buffers (early ray termination: pny_termination.h); the sums are scanned by the same kernels.
// Every kernel runs OCC_THREADS = 256 threads on at most RECON_MAX_BLOCKS workgroups and strides over the rest.
#include <hip/hip_runtime.h>

#include "pny_occupancy.h"

namespace pny {
namespace {

static_assert(OCC_THREADS == 256 && OCC_THREADS % 64 == 0, "four waves per workgroup");
static_assert(OCC_TILE_STEPS == 4, "the classification ranks four samples per thread");
constexpr int OCC_WAVES = OCC_THREADS / 64;

__device__ __forceinline__ unsigned wave_sum(unsigned x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_build_kernel(OccBuildArgs a) {
    unsigned mine = 0;
    for (uint32_t w = blockIdx.x * (uint32_t)OCC_THREADS + threadIdx.x; w < a.n_words; w += gridDim.x * (uint32_t)OCC_THREADS) {
        const uint32_t bits = occ_word(a, w);
        a.bits[w] = bits;
        mine += (unsigned)__popc(bits);
    }
    if (a.occupied) {
        const unsigned total = wave_sum(mine);
        if ((threadIdx.x & 63) == 0 && total) atomicAdd(a.occupied, (unsigned long long)total);
    }
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_classify_kernel(OccClassifyArgs a, unsigned n_tiles) {
    __shared__ unsigned counts[OCC_TILE_STEPS * OCC_WAVES];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        bool keep[OCC_TILE_STEPS];
        unsigned rank[OCC_TILE_STEPS];
#pragma unroll
        for (int j = 0; j < OCC_TILE_STEPS; ++j) {
            const uint32_t s = tile * (uint32_t)OCC_TILE + (uint32_t)j * OCC_THREADS + threadIdx.x;
            keep[j] = false;
            if (s < a.n_samples) {
                const uint32_t ray = s / a.K;
                const float4* r = reinterpret_cast<const float4*>(a.rays + (size_t)ray * 8);
                const float4 r0 = r[0], r1 = r[1];
                const float o[3] = {r0.x, r0.y, r0.z}, d[3] = {r0.w, r1.x, r1.y};
                keep[j] = occ_keep(a.g, o, d, a.z[s]);
            }
            const unsigned long long b = __ballot(keep[j]);
            rank[j] = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
            if (lane == 0) counts[j * OCC_WAVES + wave] = (unsigned)__popcll(b);
        }
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < OCC_TILE_STEPS; ++j) {
            unsigned base = before;
#pragma unroll
            for (int w = 0; w < OCC_WAVES; ++w) {
                const unsigned c = counts[j * OCC_WAVES + w];
                base += w < wave ? c : 0u;
                before += c;
            }
            const uint32_t s = tile * (uint32_t)OCC_TILE + (uint32_t)j * OCC_THREADS + threadIdx.x;
            if (s < a.n_samples) a.slot[s] = keep[j] ? (int32_t)(base + rank[j]) : -1;
        }
        total = before;
        if (threadIdx.x == 0) a.sums1[tile] = total;
        __syncthreads();       // counts is free for the next tile
    }
}

// Exclusive scan of one word per thread over the workgroup; `total` is the workgroup's sum.  Two barriers.  (recon.hip block_scan)
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
    for (int w = 0; w < OCC_WAVES; ++w) {
        const unsigned s = wave_sums[w];
        base += w < wave ? s : 0u;
        all += s;
    }
    __syncthreads();
    total = all;
    return base + incl - x;
}

// Exclusive scan of s[0 .. n) in place, tile by tile; next[tile] = the tile's sum (or null); kept = the sum of tile 0 as an
// int64 (or null: only the launch of one tile passes it).
__global__ __launch_bounds__(OCC_THREADS) void occupancy_scan_sums_kernel(uint32_t* s, unsigned n, uint32_t* next, int64_t* kept) {
    __shared__ unsigned wave_sums[OCC_WAVES];
    const unsigned n_tiles = (n + OCC_TILE - 1) / OCC_TILE;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const unsigned i0 = tile * (unsigned)OCC_TILE + threadIdx.x * (unsigned)OCC_TILE_STEPS;
        unsigned c[OCC_TILE_STEPS], mine = 0;
#pragma unroll
        for (int j = 0; j < OCC_TILE_STEPS; ++j) {
            c[j] = i0 + (unsigned)j < n ? s[i0 + (unsigned)j] : 0u;
            mine += c[j];
        }
        unsigned total;
        unsigned before = block_scan(mine, wave_sums, total);
#pragma unroll
        for (int j = 0; j < OCC_TILE_STEPS; ++j) {
            if (i0 + (unsigned)j < n) s[i0 + (unsigned)j] = before;
            before += c[j];
        }
        if (threadIdx.x == 0) {
            if (next) next[tile] = total;
            if (kept && tile == 0) *kept = (int64_t)total;
        }
    }
}

// s[i] += up[i / OCC_TILE]
__global__ __launch_bounds__(OCC_THREADS) void occupancy_add_sums_kernel(uint32_t* s, unsigned n, const uint32_t* up) {
    for (unsigned i = blockIdx.x * (unsigned)OCC_THREADS + threadIdx.x; i < n; i += gridDim.x * (unsigned)OCC_THREADS)
        s[i] += up[i / (unsigned)OCC_TILE];
}

// slot[s] += sums1[s / OCC_TILE] where the sample is kept
__global__ __launch_bounds__(OCC_THREADS) void occupancy_add_kernel(int32_t* slot, unsigned n, const uint32_t* sums1) {
    for (unsigned s = blockIdx.x * (unsigned)OCC_THREADS + threadIdx.x; s < n; s += gridDim.x * (unsigned)OCC_THREADS) {
        const int32_t v = slot[s];
        if (v >= 0) slot[s] = v + (int32_t)sums1[s / (unsigned)OCC_TILE];
    }
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_gather_kernel(const int32_t* slot, const float* rays, const float* z, unsigned n,
                                                                       unsigned K, long long m, float* xyz, float* dirs) {
    for (unsigned s = blockIdx.x * (unsigned)OCC_THREADS + threadIdx.x; s < n; s += gridDim.x * (unsigned)OCC_THREADS) {
        const long long at = slot[s];
        if (at < 0 || at >= m) continue;
        const float4* r = reinterpret_cast<const float4*>(rays + (size_t)(s / K) * 8);
        const float4 r0 = r[0], r1 = r[1];
        const float zz = z[s];
        float* p = xyz + 3 * at;
        float* d = dirs + 3 * at;
        d[0] = r0.w, d[1] = r1.x, d[2] = r1.y;
        p[0] = r0.x + zz * r0.w;
        p[1] = r0.y + zz * r1.x;
        p[2] = r0.z + zz * r1.y;
    }
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_expand_kernel(const int32_t* slot, const float4* outc, unsigned n, long long m,
                                                                       float4* out) {
    for (unsigned s = blockIdx.x * (unsigned)OCC_THREADS + threadIdx.x; s < n; s += gridDim.x * (unsigned)OCC_THREADS) {
        const long long at = slot[s];
        out[s] = (at >= 0 && at < m) ? outc[at] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ---------------------------------------------------------------------------------- depth segments (pny_termination.h)
// The same three kernels on the columns [k_begin, k_begin + Ks) of the (n, K) buffers.  Sample s of a segment is column s % Ks
// of ray s / Ks; slot is (n, Ks), ranked in ascending s, which is ascending sample order inside the segment.
__global__ __launch_bounds__(OCC_THREADS) void occupancy_classify_segment_kernel(OccSegmentArgs a, unsigned n_tiles) {
    __shared__ unsigned counts[OCC_TILE_STEPS * OCC_WAVES];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        bool keep[OCC_TILE_STEPS];
        unsigned rank[OCC_TILE_STEPS];
#pragma unroll
        for (int j = 0; j < OCC_TILE_STEPS; ++j) {
            const uint32_t s = tile * (uint32_t)OCC_TILE + (uint32_t)j * OCC_THREADS + threadIdx.x;
            keep[j] = false;
            if (s < a.n_samples) {
                const uint32_t ray = s / a.Ks, col = s - ray * a.Ks;
                const float4* r = reinterpret_cast<const float4*>(a.rays + (size_t)ray * 8);
                const float4 r0 = r[0], r1 = r[1];
                const float o[3] = {r0.x, r0.y, r0.z}, d[3] = {r0.w, r1.x, r1.y};
                keep[j] = occ_keep_segment(a, ray, o, d, a.z[(size_t)ray * a.K + a.k_begin + col]);
            }
            const unsigned long long b = __ballot(keep[j]);
            rank[j] = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
            if (lane == 0) counts[j * OCC_WAVES + wave] = (unsigned)__popcll(b);
        }
        __syncthreads();
        unsigned before = 0;
#pragma unroll
        for (int j = 0; j < OCC_TILE_STEPS; ++j) {
            unsigned base = before;
#pragma unroll
            for (int w = 0; w < OCC_WAVES; ++w) {
                const unsigned c = counts[j * OCC_WAVES + w];
                base += w < wave ? c : 0u;
                before += c;
            }
            const uint32_t s = tile * (uint32_t)OCC_TILE + (uint32_t)j * OCC_THREADS + threadIdx.x;
            if (s < a.n_samples) a.slot[s] = keep[j] ? (int32_t)(base + rank[j]) : -1;
        }
        if (threadIdx.x == 0) a.sums1[tile] = before;
        __syncthreads();       // counts is free for the next tile
    }
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_gather_segment_kernel(const int32_t* slot, const float* rays, const float* z,
                                                                               unsigned n, unsigned K, unsigned k_begin, unsigned Ks,
                                                                               long long m, float* xyz, float* dirs) {
    for (unsigned s = blockIdx.x * (unsigned)OCC_THREADS + threadIdx.x; s < n; s += gridDim.x * (unsigned)OCC_THREADS) {
        const long long at = slot[s];
        if (at < 0 || at >= m) continue;
        const unsigned ray = s / Ks, col = s - ray * Ks;
        const float4* r = reinterpret_cast<const float4*>(rays + (size_t)ray * 8);
        const float4 r0 = r[0], r1 = r[1];
        const float zz = z[(size_t)ray * K + k_begin + col];
        float* p = xyz + 3 * at;
        float* d = dirs + 3 * at;
        d[0] = r0.w, d[1] = r1.x, d[2] = r1.y;
        p[0] = r0.x + zz * r0.w;
        p[1] = r0.y + zz * r1.x;
        p[2] = r0.z + zz * r1.y;
    }
}

__global__ __launch_bounds__(OCC_THREADS) void occupancy_expand_segment_kernel(const int32_t* slot, const float4* outc, unsigned n,
                                                                               unsigned K, unsigned k_begin, unsigned Ks, long long m,
                                                                               float4* out) {
    for (unsigned s = blockIdx.x * (unsigned)OCC_THREADS + threadIdx.x; s < n; s += gridDim.x * (unsigned)OCC_THREADS) {
        const long long at = slot[s];
        const unsigned ray = s / Ks, col = s - ray * Ks;
        out[(size_t)ray * K + k_begin + col] = (at >= 0 && at < m) ? outc[at] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

inline unsigned capped(int64_t blocks) {
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks < (int64_t)RECON_MAX_BLOCKS ? blocks : (int64_t)RECON_MAX_BLOCKS);
}

}  // namespace

void launch_occupancy_build(const OccBuildArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(occupancy_build_kernel, dim3(capped(((int64_t)a.n_words + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st, a);
}

// the ranks inside the tiles, the scan of the tile sums level by level, the ranks; kept = int64 on the device
void launch_occupancy_classify(const OccClassifyArgs& a, const OccLayout& l, uint32_t* sums2, int64_t* kept, hipStream_t st) {
    hipLaunchKernelGGL(occupancy_classify_kernel, dim3(capped(l.n1)), dim3(OCC_THREADS), 0, st, a, (unsigned)l.n1);
    if (l.n2 == 0) {
        hipLaunchKernelGGL(occupancy_scan_sums_kernel, dim3(1), dim3(OCC_THREADS), 0, st, a.sums1, (unsigned)l.n1, (uint32_t*)nullptr, kept);
    } else {
        hipLaunchKernelGGL(occupancy_scan_sums_kernel, dim3(capped(l.n2)), dim3(OCC_THREADS), 0, st, a.sums1, (unsigned)l.n1, sums2,
                           (int64_t*)nullptr);
        hipLaunchKernelGGL(occupancy_scan_sums_kernel, dim3(1), dim3(OCC_THREADS), 0, st, sums2, (unsigned)l.n2, (uint32_t*)nullptr, kept);
        hipLaunchKernelGGL(occupancy_add_sums_kernel, dim3(capped((l.n1 + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st, a.sums1,
                           (unsigned)l.n1, (const uint32_t*)sums2);
    }
    hipLaunchKernelGGL(occupancy_add_kernel, dim3(capped(((int64_t)a.n_samples + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st,
                       a.slot, a.n_samples, (const uint32_t*)a.sums1);
}

void launch_occupancy_gather(const int32_t* slot, const float* rays, const float* z, int64_t n_samples, int K, int64_t m, float* xyz,
                             float* dirs, hipStream_t st) {
    hipLaunchKernelGGL(occupancy_gather_kernel, dim3(capped((n_samples + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st, slot,
                       rays, z, (unsigned)n_samples, (unsigned)K, (long long)m, xyz, dirs);
}

void launch_occupancy_expand(const int32_t* slot, const float* outc, int64_t n_samples, int64_t m, float* out, hipStream_t st) {
    hipLaunchKernelGGL(occupancy_expand_kernel, dim3(capped((n_samples + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st, slot,
                       reinterpret_cast<const float4*>(outc), (unsigned)n_samples, (long long)m, reinterpret_cast<float4*>(out));
}

// the segment forms: the classification's first kernel differs, the scan of the tile sums and the add pass are the same launches
void launch_occupancy_classify_segment(const OccSegmentArgs& a, const OccLayout& l, uint32_t* sums2, int64_t* kept, hipStream_t st) {
    hipLaunchKernelGGL(occupancy_classify_segment_kernel, dim3(capped(l.n1)), dim3(OCC_THREADS), 0, st, a, (unsigned)l.n1);
    if (l.n2 == 0) {
        hipLaunchKernelGGL(occupancy_scan_sums_kernel, dim3(1), dim3(OCC_THREADS), 0, st, a.sums1, (unsigned)l.n1, (uint32_t*)nullptr, kept);
    } else {
        hipLaunchKernelGGL(occupancy_scan_sums_kernel, dim3(capped(l.n2)), dim3(OCC_THREADS), 0, st, a.sums1, (unsigned)l.n1, sums2,
                           (int64_t*)nullptr);
        hipLaunchKernelGGL(occupancy_scan_sums_kernel, dim3(1), dim3(OCC_THREADS), 0, st, sums2, (unsigned)l.n2, (uint32_t*)nullptr, kept);
        hipLaunchKernelGGL(occupancy_add_sums_kernel, dim3(capped((l.n1 + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st, a.sums1,
                           (unsigned)l.n1, (const uint32_t*)sums2);
    }
    hipLaunchKernelGGL(occupancy_add_kernel, dim3(capped(((int64_t)a.n_samples + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st,
                       a.slot, a.n_samples, (const uint32_t*)a.sums1);
}

void launch_occupancy_gather_segment(const int32_t* slot, const float* rays, const float* z, int64_t n, int K, int k_begin, int k_end,
                                     int64_t m, float* xyz, float* dirs, hipStream_t st) {
    const int64_t n_samples = n * (k_end - k_begin);
    hipLaunchKernelGGL(occupancy_gather_segment_kernel, dim3(capped((n_samples + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st,
                       slot, rays, z, (unsigned)n_samples, (unsigned)K, (unsigned)k_begin, (unsigned)(k_end - k_begin), (long long)m, xyz, dirs);
}

void launch_occupancy_expand_segment(const int32_t* slot, const float* outc, int64_t n, int K, int k_begin, int k_end, int64_t m,
                                     float* out, hipStream_t st) {
    const int64_t n_samples = n * (k_end - k_begin);
    hipLaunchKernelGGL(occupancy_expand_segment_kernel, dim3(capped((n_samples + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, st,
                       slot, reinterpret_cast<const float4*>(outc), (unsigned)n_samples, (unsigned)K, (unsigned)k_begin,
                       (unsigned)(k_end - k_begin), (long long)m, reinterpret_cast<float4*>(out));
}

}  // namespace pny
