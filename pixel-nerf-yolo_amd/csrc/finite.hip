// NaN / Inf scan over a table of fp32 tensors in ONE launch (pny_finite_check, pny_finite_check_tensors: finite_api.hip).
//
// Work: the tensors of the table laid end to end and cut into chunks of FINITE_CHUNK elements, one workgroup per chunk, as the
// multi-tensor Adam kernel does (optim.hip).  There is no chunk table: entry i carries chunk0 = the number of chunks before it,
// and a workgroup finds its entry from its chunk number (binary search in the device table, a scan of the <= 8 entries of an
// immediate call); an empty tensor owns no chunk and is never found.
// Memory: one stream in, nothing out.  A chunk starts a multiple of FINITE_CHUNK elements into its tensor, so it has the
// tensor's misalignment to 16 bytes: a scalar head of up to 3 elements reaches the boundary, the body is read as 16-byte
// words, a scalar tail takes the rest.
// Test: on the raw bits -- exponent all ones = not finite, and then a non-zero mantissa = NaN (quiet, signalling, either sign),
// else +-Inf.  No floating-point instruction touches the values.
// Result: every lane ORs what it saw into two bits; the wave combines them with two ballots, and only a wave that found
// something issues the two atomics (OR into the group's bits, MIN of the table index into the group's `first`).  A clean scan
// therefore writes nothing, and OR / MIN make the words independent of the execution order.
#include "pny_finite.h"

namespace pny {

__device__ __forceinline__ unsigned finite_bits(unsigned u) {
    if ((u & 0x7f800000u) != 0x7f800000u) return 0u;
    return (u & 0x007fffffu) ? (unsigned)PNY_FINITE_NAN : (unsigned)PNY_FINITE_INF;
}

// Chunk `chunk` (counted inside the tensor) of table entry `index`.  Called by all 256 lanes of the workgroup.
__device__ __forceinline__ void finite_scan_chunk(const FiniteEntry t, int index, long long chunk, int32_t* __restrict__ flags) {
    const long long off = chunk * FINITE_CHUNK, left = t.count - off;
    const int n = left < FINITE_CHUNK ? (int)left : (int)FINITE_CHUNK;
    const unsigned* p = reinterpret_cast<const unsigned*>(t.p) + off;
    const int tid = (int)threadIdx.x;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
    int head = (int)((4u - mis) & 3u);   // elements [0, head) scalar, [head, head + body) as 16-byte words, [head + body, n) scalar
    if (head > n) head = n;
    const int body = (n - head) & ~3;
    unsigned bits = 0u;
    for (int i = tid; i < head; i += 256) bits |= finite_bits(p[i]);
#pragma unroll 4
    for (int i = head + 4 * tid; i < head + body; i += 4 * 256) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + i);
        bits |= finite_bits(v.x) | finite_bits(v.y) | finite_bits(v.z) | finite_bits(v.w);
    }
    for (int i = head + body + tid; i < n; i += 256) bits |= finite_bits(p[i]);
    const unsigned long long nan = __ballot((bits & PNY_FINITE_NAN) != 0u), inf = __ballot((bits & PNY_FINITE_INF) != 0u);
    if ((nan | inf) != 0ull && (tid & 63) == 0) {
        atomicOr(flags + 2 * t.group, (nan ? PNY_FINITE_NAN : 0) | (inf ? PNY_FINITE_INF : 0));
        atomicMin(flags + 2 * t.group + 1, index);
    }
}

// grid = the chunks [chunk_base, chunk_base + gridDim.x) of table entries [index0, index0 + n)
__global__ __launch_bounds__(256) void finite_table_kernel(const FiniteEntry* __restrict__ table, int index0, int n, int chunk_base,
                                                           int32_t* __restrict__ flags) {
    const int c = chunk_base + (int)blockIdx.x;
    int lo = index0, hi = index0 + n - 1;   // the LAST entry with chunk0 <= c: of several entries with the same chunk0 all but the
    while (lo < hi) {                       // last are empty, and trailing empty entries start at the total, beyond every c
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk0 <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    const FiniteEntry t = table[lo];
    const long long chunk = c - t.chunk0;
    if (chunk * FINITE_CHUNK >= t.count) return;   // (never: the grid covers the entries' chunks exactly)
    finite_scan_chunk(t, lo, chunk, flags);
}

__global__ __launch_bounds__(256) void finite_immediate_kernel(const FiniteImmediate tab, int n, int32_t* __restrict__ flags) {
    const int c = (int)blockIdx.x;
    int idx = 0;
    for (int i = 1; i < PNY_FINITE_MAX_IMMEDIATE; ++i)
        if (i < n && tab.e[i].chunk0 <= c) idx = i;
    const FiniteEntry t = tab.e[idx];
    const long long chunk = c - t.chunk0;
    if (chunk * FINITE_CHUNK >= t.count) return;
    finite_scan_chunk(t, idx, chunk, flags);
}

__global__ void finite_reset_kernel(int32_t* __restrict__ flags, int n_groups) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= n_groups) return;
    flags[2 * g] = 0;
    flags[2 * g + 1] = INT32_MAX;
}

void launch_finite_table(const FiniteEntry* table_dev, int index0, int n, int chunk_base, int n_chunks, int32_t* flags, hipStream_t st) {
    if (n <= 0 || n_chunks <= 0) return;
    hipLaunchKernelGGL(finite_table_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, table_dev, index0, n, chunk_base, flags);
}

void launch_finite_immediate(const FiniteImmediate& t, int n, int n_chunks, int32_t* flags, hipStream_t st) {
    if (n <= 0 || n_chunks <= 0) return;
    hipLaunchKernelGGL(finite_immediate_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, t, n, flags);
}

void launch_finite_reset(int32_t* flags, int n_groups, hipStream_t st) {
    if (n_groups <= 0) return;
    hipLaunchKernelGGL(finite_reset_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, flags, n_groups);
}

}  // namespace pny
