// Argument blocks and launchers of the NaN / Inf monitor (finite.hip; entry points in finite_api.hip).
#pragma once
#include "pny_common.h"

namespace pny {

enum { FINITE_CHUNK = 4096 };   // elements per workgroup: 256 lanes x 4 16-byte loads

// One tensor of a scan.  chunk0 = number of chunks of the table entries before it (an empty tensor owns no chunk).
struct FiniteEntry {
    const float* p;
    long long count;
    int group;
    int chunk0;
};
struct FiniteImmediate {        // the table of pny_finite_check_tensors, by value in the kernel-argument segment
    FiniteEntry e[PNY_FINITE_MAX_IMMEDIATE];
};

// entries [index0, index0 + n) of a device-resident table; their chunks are [chunk_base, chunk_base + n_chunks)
void launch_finite_table(const FiniteEntry* table_dev, int index0, int n, int chunk_base, int n_chunks, int32_t* flags, hipStream_t st);
void launch_finite_immediate(const FiniteImmediate& t, int n, int n_chunks, int32_t* flags, hipStream_t st);
void launch_finite_reset(int32_t* flags, int n_groups, hipStream_t st);

}  // namespace pny
