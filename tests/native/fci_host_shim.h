// Stand-in for csrc/nbx_common.h that compiles csrc/fci.hip for the HOST (tests/test_host_fci_kernels.py): a launch runs
// EVERY workgroup of the grid with ONE thread, one after the other.  With a single thread a barrier is a no-op and the
// row staged in "LDS" is complete before it is read, so the gather and scatter kernels run as written; the build raises
// NBX_FCI_PT so that the one thread can hold a whole row.  What this cannot show -- races between threads, the LDS
// budget, the GEMM -- is left to the GPU suite.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <cstring>
struct nbx_ctx { int stream; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__
#define __restrict__
// the dynamic LDS of the kernels: their block-scope extern declaration, inside the unnamed namespace, names this array
namespace { alignas(16) double srow[1 << 16]; }
static inline void __syncthreads() {}
#define NBX_OK 0
#define NBX_E_INVALID -1
#define NBX_E_HIP -2
#define NBX_E_UNSUPPORTED -5
#define hipSuccess 0
#define hipFuncAttributeMaxDynamicSharedMemorySize 0
static inline int hipFuncSetAttribute(const void*, int, int) { return 0; }
static inline void nbx_set_error(const char* fmt, ...) { fprintf(stderr, "err: %s\n", fmt); }
#define NBX_CHECK_ARG(cond) do { if (!(cond)) { fprintf(stderr, "invalid: %s\n", #cond); return NBX_E_INVALID; } } while (0)
#define NBX_HIP(call) do { (void)(call); } while (0)
#define NBX_LAUNCH_CHECK() do {} while (0)
static inline int64_t nbx_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
#define hipLaunchKernelGGL(k, g, b, s, st, ...) do { dim3 g_ = (g); gridDim = dim3(g_.x); blockDim = dim3(1); \
    threadIdx = dim3(0); for (unsigned bx = 0; bx < g_.x; ++bx) { blockIdx = dim3(bx); k(__VA_ARGS__); } } while (0)
