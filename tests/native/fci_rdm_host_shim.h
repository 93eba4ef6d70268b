// Stand-in for csrc/nbx_common.h that compiles csrc/fci_rdm.hip (and csrc/fci.hip beside it) for the HOST
// (tests/test_host_fci_rdm.py): fci_host_shim.h -- every workgroup of a launch runs with ONE thread -- plus what the
// density kernels add to it.  The build sets NBX_RDM_WAVE=1, a wavefront of one lane, whose sum is the lane's own value.
// What this cannot show -- the butterfly across real lanes, races, the LDS budget, the GEMM -- is left to the GPU suite.
#pragma once
#include "fci_host_shim.h"
static inline double nbx_wave_sum(double v) { return v; }
