// CCSD Lambda equations and one-particle density on the device: what a GEMM cannot express
// (include/nbx.h, "coupled cluster").
//
// The contractions of the Lambda equations (nbed_amd/ccsd_gpu.py, the equations of nbed_amd/ccsd.py) are nbx_gemm
// calls between the permutes of csrc/ccsd.hip.  Two things are not products: the disconnected term
// P(ij) P(ab) l_ia F_jb of the doubles equation, an outer product antisymmetrised in both pairs, and the assembly of
// the spin-resolved density from its occupied / virtual blocks.  Both are grid-stride, one trip to memory per element,
// no atomics: equal inputs give equal bits.
#include "nbx_common.h"

namespace {

inline unsigned cl_grid(int64_t n, int block = 256) {
    int64_t g = nbx_cdiv(n, block);
    if (g > 262144) g = 262144;  // grid-stride loops below
    if (g < 1) g = 1;
    return (unsigned)g;
}

// r2[i,j,a,b] += alpha ( x_ia y_jb - x_ja y_ib - x_ib y_ja + x_jb y_ia ); an operand is (nocc, nvir), or (nvir, nocc)
// where its bit of `layout` is set (bit 0: x, bit 1: y)
__global__ __launch_bounds__(256) void lambda_outer_kernel(int no, int nv, double alpha, const double* __restrict__ x,
                                                           const double* __restrict__ y, int layout,
                                                           double* __restrict__ r2) {
    const int64_t sxo = (layout & 1) ? 1 : nv, sxv = (layout & 1) ? no : 1;
    const int64_t syo = (layout & 2) ? 1 : nv, syv = (layout & 2) ? no : 1;
    const int64_t total = (int64_t)no * no * nv * nv;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t k = idx;
        const int64_t b = k % nv; k /= nv;
        const int64_t a = k % nv; k /= nv;
        const int64_t j = k % no;
        const int64_t i = k / no;
        const double v = ((x[i * sxo + a * sxv] * y[j * syo + b * syv] - x[j * sxo + a * sxv] * y[i * syo + b * syv]) -
                          x[i * sxo + b * sxv] * y[j * syo + a * syv]) +
                         x[j * sxo + b * sxv] * y[i * syo + a * syv];
        r2[idx] += alpha * v;
    }
}

// element (x, y) of the density over the concatenated list [occupied | virtual] of spin orbitals
__device__ __forceinline__ double gamma_element(int no, int nv, const double* __restrict__ goo, const double* __restrict__ gov,
                                                const double* __restrict__ gvo, const double* __restrict__ gvv, int x, int y) {
    if (x < no) return y < no ? goo[(int64_t)x * no + y] : gov[(int64_t)x * nv + (y - no)];
    return y < no ? gvo[(int64_t)(x - no) * no + y] : gvv[(int64_t)(x - no) * nv + (y - no)];
}

// dm1[s, p, q] = 1/2 (gamma[P,Q] + gamma[Q,P]) + (P = Q occupied), P = 2p + s, Q = 2q + s, for every pair of the
// concatenated list with equal spins; max |gamma[P,Q]| over the pairs with different spins into *cross (a NaN sticks).
// ONE workgroup: the matrix has (2n)^2 elements, and a single workgroup needs neither an atomic nor a second launch.
__global__ __launch_bounds__(256) void rdm1_kernel(int n, int no, int nv, const int* __restrict__ occ,
                                                   const int* __restrict__ vir, const double* __restrict__ goo,
                                                   const double* __restrict__ gov, const double* __restrict__ gvo,
                                                   const double* __restrict__ gvv, double* __restrict__ dm1,
                                                   double* __restrict__ cross) {
    __shared__ double red[256];
    const int nso = no + nv;
    const int64_t total = (int64_t)nso * nso;
    double m = 0.0;
    for (int64_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int x = (int)(idx / nso), y = (int)(idx - (int64_t)x * nso);
        const int P = x < no ? occ[x] : vir[x - no], Q = y < no ? occ[y] : vir[y - no];
        const double gxy = gamma_element(no, nv, goo, gov, gvo, gvv, x, y);
        if ((P & 1) == (Q & 1)) {
            const double gyx = gamma_element(no, nv, goo, gov, gvo, gvv, y, x);
            double v = 0.5 * (gxy + gyx);
            if (x == y && x < no) v += 1.0;
            dm1[((int64_t)(P & 1) * n + (P >> 1)) * n + (Q >> 1)] = v;
        } else {
            const double ag = fabs(gxy);
            m = (ag > m || ag != ag) ? ag : m;
        }
    }
    red[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == blockDim.x - 1) {  // (any one thread; the last, so that a thread-by-thread host run sees every slot)
        for (int t = 0; t < (int)blockDim.x - 1; ++t) m = (red[t] > m || red[t] != red[t]) ? red[t] : m;
        *cross = m;
    }
}

}  // namespace

extern "C" {

int nbx_ccsd_lambda_outer(nbx_ctx* ctx, int64_t nocc, int64_t nvir, double alpha, const double* d_x, const double* d_y,
                          int layout, double* d_r2) {
    NBX_CHECK_ARG(ctx && nocc >= 0 && nvir >= 0 && nocc < 32768 && nvir < 32768 && layout >= 0 && layout < 4);
    const int64_t total = nocc * nocc * nvir * nvir;
    if (total == 0) return NBX_OK;
    NBX_CHECK_ARG(d_x && d_y && d_r2 && d_r2 != d_x && d_r2 != d_y);
    hipLaunchKernelGGL(lambda_outer_kernel, dim3(cl_grid(total)), dim3(256), 0, ctx->stream, (int)nocc, (int)nvir, alpha, d_x,
                       d_y, layout, d_r2);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_ccsd_rdm1(nbx_ctx* ctx, int64_t n, int64_t nocc, int64_t nvir, const int* d_occ, const int* d_vir,
                  const double* d_goo, const double* d_gov, const double* d_gvo, const double* d_gvv, double* d_dm1,
                  double* d_cross) {
    NBX_CHECK_ARG(ctx && n > 0 && n < 16384 && nocc >= 0 && nvir >= 0 && nocc + nvir == 2 * n);
    NBX_CHECK_ARG(d_dm1 && d_cross && (nocc == 0 || (d_occ && d_goo)) && (nvir == 0 || (d_vir && d_gvv)));
    NBX_CHECK_ARG(nocc == 0 || nvir == 0 || (d_gov && d_gvo));
    hipLaunchKernelGGL(rdm1_kernel, dim3(1), dim3(256), 0, ctx->stream, (int)n, (int)nocc, (int)nvir, d_occ, d_vir, d_goo, d_gov,
                       d_gvo, d_gvv, d_dm1, d_cross);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // extern "C"
