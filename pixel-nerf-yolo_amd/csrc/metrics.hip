// Scoring rendered views against the ground truth in ONE launch for all views: the clamped 8-bit image, PSNR and SSIM of
// every view (reference eval/eval.py:288-345, eval/calc_metrics.py:189-191; arithmetic in pny_metrics.h).  The reference brings
// every render to the host and calls skimage there; here the renders stay on the device and nothing waits for it.
//
// A workgroup owns one tile of METRICS_TILE_H x METRICS_TILE_W SSIM windows of one view.  It stages the tile and its 6-pixel
// apron of both images in LDS (loads and byte stores run along W * 3, the contiguous axis), then per channel forms the five
// window moments separably in fp64: row sums of 7 into LDS, column sums of 7 out of it -- 14 taps per window instead of 49.
// A pixel's squared error and byte belong to the tile that holds it as an output position; the bottom and right borders
// (6 pixels that are no window's top-left corner) belong to the last tile of their row / column of tiles.
//
// Reduction as in loss.hip: fp64 sums per thread in index order, a fixed tree over the workgroup, one row {sum of squared
// errors, sum of S} per workgroup in a table, a ticket; the workgroup that draws the last ticket adds every view's rows (one
// wave per view: lane l adds the rows l, l + 64, ... in order, then a fixed shuffle tree), divides, takes the logarithm and
// writes {psnr, ssim}.  No float atomics: the same inputs give the same bits on every run.
//
// The flat form (METRICS_GT_FLAT) is util.psnr (src/util/util.py:502-509): n plain elements per view, no clamp, no SSIM.
#include <hip/hip_runtime.h>

#include "pny_metrics.h"

namespace pny {
namespace {

constexpr int IN_H = METRICS_TILE_H + METRICS_APRON;          // staged rows
constexpr int IN_W = METRICS_TILE_W + METRICS_APRON;          // staged pixels per row
constexpr int IN_W3 = IN_W * 3;                               // staged floats per row (channel-interleaved, as in memory)
constexpr int WAVES = METRICS_THREADS / 64;

__device__ inline double wave_sum(double x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

// Sums of the workgroup's threads in a fixed order, valid in thread 0 (loss.hip block_sum).  lds: WAVES * METRICS_SUMS doubles.
__device__ inline void block_sum(double (&v)[METRICS_SUMS], double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < METRICS_SUMS; ++i) {
        const double x = wave_sum(v[i]);
        if (lane == 0) lds[wave * METRICS_SUMS + i] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < METRICS_SUMS; ++i)
        v[i] = ((lds[i] + lds[METRICS_SUMS + i]) + lds[2 * METRICS_SUMS + i]) + lds[3 * METRICS_SUMS + i];
}

__global__ __launch_bounds__(METRICS_THREADS) void view_metrics_kernel(ViewMetricsArgs a) {
    __shared__ float px[IN_H * IN_W3], py[IN_H * IN_W3];
    __shared__ double rs[5][IN_H][METRICS_TILE_W];
    __shared__ double red[WAVES * METRICS_SUMS];
    __shared__ int is_last;
    const int tid = threadIdx.x;
    const int tpv = a.tiles_y * a.tiles_x;
    const int v = blockIdx.x / tpv, t = blockIdx.x - v * tpv;
    double s[METRICS_SUMS] = {0.0, 0.0};

    if (a.layout == METRICS_GT_FLAT) {
        const size_t base = (size_t)v * a.w;
        const int e0 = t * METRICS_FLAT_CHUNK, e1 = min(e0 + METRICS_FLAT_CHUNK, a.w);
        for (int i = e0 + tid; i < e1; i += METRICS_THREADS) {
            const double d = (double)a.rgb[base + i] - (double)a.gt[base + i];
            s[0] += d * d;
        }
    } else {
        const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const int y0 = ty * METRICS_TILE_H, x0 = tx * METRICS_TILE_W;
        // staged pixels that lie inside the image; windows of this tile; pixels whose error and byte this tile owns
        const int rows = min(IN_H, a.h - y0), cols = min(IN_W, a.w - x0);
        const int out_y = min(METRICS_TILE_H, a.h - METRICS_APRON - y0), out_x = min(METRICS_TILE_W, a.w - METRICS_APRON - x0);
        const int own_rows = ty == a.tiles_y - 1 ? rows : METRICS_TILE_H, own_cols3 = (tx == a.tiles_x - 1 ? cols : METRICS_TILE_W) * 3;
        const int cols3 = cols * 3;
        const size_t plane = (size_t)a.h * a.w;
        const size_t img = (size_t)v * plane * 3;
        const bool gt_same = a.metrics && a.layout == METRICS_GT_NHWC_01;
        for (int i = tid; i < rows * cols3; i += METRICS_THREADS) {
            const int r = i / cols3, j = i - r * cols3;
            const size_t g = img + ((size_t)(y0 + r) * a.w + x0) * 3 + j;
            const float x = metrics_clamp01(a.rgb[g]);
            px[r * IN_W3 + j] = x;
            if (a.rgb8 && r < own_rows && j < own_cols3) a.rgb8[g] = metrics_byte(x);
            if (gt_same) py[r * IN_W3 + j] = a.gt[g];
        }
        if (!a.metrics) return;
        if (a.layout == METRICS_GT_NCHW_PM1) {
            const int per = rows * cols;
            for (int i = tid; i < 3 * per; i += METRICS_THREADS) {
                const int ch = i / per, rem = i - ch * per, r = rem / cols, c = rem - r * cols;
                py[r * IN_W3 + c * 3 + ch] = metrics_gt_from_pm1(a.gt[img + ch * plane + (size_t)(y0 + r) * a.w + x0 + c]);
            }
        }
        __syncthreads();
        for (int i = tid; i < own_rows * own_cols3; i += METRICS_THREADS) {
            const int r = i / own_cols3, j = i - r * own_cols3;
            const double d = (double)px[r * IN_W3 + j] - (double)py[r * IN_W3 + j];
            s[0] += d * d;
        }
        for (int ch = 0; ch < 3; ++ch) {
            for (int i = tid; i < rows * out_x; i += METRICS_THREADS) {      // row sums of 7
                const int r = i / out_x, c = i - r * out_x;
                const float* qx = px + r * IN_W3 + c * 3 + ch;
                const float* qy = py + r * IN_W3 + c * 3 + ch;
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < METRICS_WIN; ++k) {
                    const double x = (double)qx[3 * k], y = (double)qy[3 * k];
                    m[0] += x, m[1] += y, m[2] += x * x, m[3] += y * y, m[4] += x * y;
                }
#pragma unroll
                for (int q = 0; q < 5; ++q) rs[q][r][c] = m[q];
            }
            __syncthreads();
            for (int i = tid; i < out_y * out_x; i += METRICS_THREADS) {     // column sums of 7, S of the window
                const int oy = i / out_x, ox = i - oy * out_x;
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < METRICS_WIN; ++k)
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] += rs[q][oy + k][ox];
                s[1] += metrics_ssim_window(m[0], m[1], m[2], m[3], m[4]);
            }
            __syncthreads();
        }
    }

    block_sum(s, red);
    if (tid == 0) {
        // hand-off as loss.hip combine<>: plain stores of the row, agent-scope release, relaxed agent-scope ticket add
#pragma unroll
        for (int i = 0; i < METRICS_SUMS; ++i) a.partials[(size_t)blockIdx.x * METRICS_SUMS + i] = s[i];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        is_last = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    // the last arriver: every thread acquires at agent scope and reads the rows with agent-scope loads (their writers may
    // sit on another XCD with an L2 of its own)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int lane = tid & 63, wave = tid >> 6;
    const bool flat = a.layout == METRICS_GT_FLAT;
    const double n_elem = flat ? (double)a.w : (double)a.h * (double)a.w * 3.0;
    const double n_win = 3.0 * (double)(a.h - METRICS_APRON) * (double)(a.w - METRICS_APRON);
    for (int u = wave; u < a.nv; u += WAVES) {
        double sse = 0.0, ss = 0.0;
        for (int g = lane; g < tpv; g += 64) {
            const double* row = a.partials + ((size_t)u * tpv + g) * METRICS_SUMS;
            sse += __hip_atomic_load(row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ss += __hip_atomic_load(row + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        sse = wave_sum(sse);
        ss = wave_sum(ss);
        if (lane == 0) {
            a.metrics[2 * u] = metrics_psnr(sse, n_elem);
            a.metrics[2 * u + 1] = flat ? (double)__int_as_float(0x7fc00000) : ss / n_win;
        }
    }
    if (tid == 0) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch starts from zero
}

}  // namespace

void launch_view_metrics(const ViewMetricsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(view_metrics_kernel, dim3((unsigned)a.nv * a.tiles_y * a.tiles_x), dim3(METRICS_THREADS), 0, st, a);
}

}  // namespace pny
