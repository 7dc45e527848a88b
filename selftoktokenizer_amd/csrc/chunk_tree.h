// The pairwise tree of a binary counter over per-chunk fp64 values, shared by the statistics of csrc/fid.hip and the column means of
// csrc/gen_metrics.hip: the sum of 2^(l + 1) consecutive chunks is (earlier 2^l) + (later 2^l), and the blocks left over by the binary
// expansion of the chunk count are added from the latest (smallest) to the earliest, t = block + t.  No atomics, one fixed order.
#pragma once
#include "common.h"

namespace selftok {

constexpr int LEVELS = 23;                                        // 2^23 chunks of 256 rows: every N below 2^31

// the pairwise tree of a binary counter over the chunk values, in registers (every index is a compile-time constant)
struct chunk_tree {
    double lvl[LEVELS];
    unsigned n;
    __device__ __forceinline__ void init() { n = 0; }
    __device__ __forceinline__ void push(double v)
    {
        bool placed = false;
#pragma unroll
        for (int l = 0; l < LEVELS; ++l) {
            if (placed) continue;
            if ((n >> l) & 1u) v = lvl[l] + v;                    // (earlier 2^l chunks) + (later 2^l chunks)
            else { lvl[l] = v; placed = true; }
        }
        ++n;
    }
    __device__ __forceinline__ double total() const
    {
        double t = 0.0;
        bool have = false;
#pragma unroll
        for (int l = 0; l < LEVELS; ++l)
            if ((n >> l) & 1u) { t = have ? lvl[l] + t : lvl[l]; have = true; }
        return t;
    }
};

}  // namespace selftok
