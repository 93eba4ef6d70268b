// Stand-in for csrc/nbx_common.h that compiles csrc/mp2.hip for the HOST (tests/test_host_mp2_fno.py): ccsd_host_shim.h
// plus what mp2.hip uses beyond it, with a launch of ONE thread per workgroup.  mp2.hip walks the elements of a tile with
// a stride of blockDim.x, so a single thread fills both LDS tiles before it reads them back transposed: the index
// arithmetic of the tile / mirror scheme, the grid-stride over (i, j, tile) with three workgroups and the two-stage
// energy sum all run as written.  What stays with the GPU suite is the exchange between lanes across the barrier.
#pragma once
#include "ccsd_host_shim.h"
#define NBX_E_NOMEM -3
static inline double nbx_block_sum(double v, double*) { return v; }  // (one thread)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, s, st, ...) do { dim3 g_ = (g); gridDim = dim3(std::min(g_.x, 3u)); blockDim = dim3(1); \
    threadIdx = dim3(0); for (unsigned bx = 0; bx < gridDim.x; ++bx) { blockIdx = dim3(bx); k(__VA_ARGS__); } } while (0)
