// Stand-in for csrc/nbx_common.h that compiles csrc/ccsd.hip for the HOST (tests/test_host_ccsd_kernels.py): a launch
// runs the kernel thread by thread, a few workgroups of two threads, which is valid for the grid-stride kernels (gather,
// Fock, same-axis permute, pair pack / unpack, tau, update without its workgroup reduction) and NOT for kernels that
// exchange data across a barrier (the tiled permute): those are left to the GPU suite.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <algorithm>
struct nbx_ctx { int stream; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
static inline void __syncthreads() {}
static inline double __shfl_xor(double v, int, int) { return v; }
static inline long long __double_as_longlong(double v) { long long r; memcpy(&r, &v, 8); return r; }
static inline void atomicMax(unsigned long long* p, unsigned long long v) { if (v > *p) *p = v; }
#define NBX_OK 0
#define NBX_E_INVALID -1
#define NBX_E_HIP -2
#define NBX_E_UNSUPPORTED -5
#define hipSuccess 0
static inline int hipMemsetAsync(void* p, int v, size_t n, int) { memset(p, v, n); return 0; }
static inline void nbx_set_error(const char* fmt, ...) { fprintf(stderr, "err: %s\n", fmt); }
#define NBX_CHECK_ARG(cond) do { if (!(cond)) { fprintf(stderr, "invalid: %s\n", #cond); return NBX_E_INVALID; } } while (0)
#define NBX_HIP(call) do { (void)(call); } while (0)
#define NBX_LAUNCH_CHECK() do {} while (0)
static inline int64_t nbx_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// at most 3 blocks of 2 threads: enough to exercise the grid-stride arithmetic
#define hipLaunchKernelGGL(k, g, b, s, st, ...) do { dim3 g_ = (g); gridDim = dim3(std::min(g_.x, 3u)); blockDim = dim3(2); \
    for (unsigned bx = 0; bx < gridDim.x; ++bx) for (unsigned tx = 0; tx < 2; ++tx) { blockIdx = dim3(bx); threadIdx = dim3(tx); k(__VA_ARGS__); } } while (0)
