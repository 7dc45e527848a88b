// Host stand-in for csrc/common.h + the HIP runtime, used by tests/test_image_io_standin_cpu.py and tests/test_image_views_standin_cpu.py: csrc/image_io.hip,
// csrc/image_views.hip and the headers they include (image_resample_shared.h, u8_shared.h; the tests copy them beside this file) are plain C++ around their
// launches, so with these few definitions a host compiler builds them and every "kernel" runs as nested loops over the grid.  The arithmetic
// (fp64 tap weights, integer sums, the bf16 rounding) is then the host's IEEE arithmetic -- the same operations the GPU executes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <stdio.h>
#define SELFTOK_OK 0
#define SELFTOK_EINVAL (-1)
#define SELFTOK_EHIP (-2)
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
typedef void* hipStream_t;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 threadIdx, blockIdx;
static inline void __syncthreads() {}
static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
// threads run one after the other, so a barrier cannot work; every kernel of the unit is idempotent, hence the grid simply runs TWICE: in the
// second run the plan kernel's thread 0 (the code after its barrier) sees the headers every thread wrote in the first
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) do { dim3 g_ = grid, b_ = block; for (int rep_ = 0; rep_ < 2; ++rep_) \
  for (unsigned by_ = 0; by_ < g_.y; ++by_) for (unsigned bx_ = 0; bx_ < g_.x; ++bx_) for (unsigned tx_ = 0; tx_ < b_.x; ++tx_) { \
    blockIdx.x = bx_; blockIdx.y = by_; threadIdx.x = tx_; k(__VA_ARGS__); } } while (0)
namespace selftok {
static char g_err[256];
inline void set_last_error(const char* m) { strncpy(g_err, m, 255); }
inline int check_launch(const char*) { return 0; }
}
extern "C" const char* selftok_last_error(void) { return selftok::g_err; }
