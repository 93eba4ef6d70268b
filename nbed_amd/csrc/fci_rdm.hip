// Determinant FCI on the device: one- and two-particle (transition) density matrices (include/nbx.h, "full CI",
// densities).  Bra b and ket c are CI vectors of one (n_alpha, n_beta) sector in the layout of fci.hip.
//
// The 2-RDM route reuses the sigma build's gather: with D_x[g, K] = <K| E_g |x> (x itself in the last row),
//     Graw[(s,kl),(t,mn)] = sum_K D_b[(s,kl), K] D_c[(t,mn), K] = <b| E^s_lk E^t_mn |c>,
//     Graw[(s,kl), last] = <b| E^s_lk |c>,   Graw[last, last] = <b|c>
// is one D_b . D_c^T per chunk of alpha rows (nbx_gemm, the reduction split into slabs that each own a partial
// matrix), and   <b| a+_ps a+_qt a_rt a_ss |c> = <b| E^s_ps E^t_qr |c> - delta_st delta_qs <b| E^s_pr |c>
// is an index map with one subtraction: rdm_finish_kernel.
//
// The 1-RDM alone needs no D: rdm1_kernel forms <b| E_g |c> row by row of the bra, one workgroup per alpha row,
// one wavefront per generator, into partials (Na, 2 n^2) that rdm1_reduce_kernel sums over the rows in ascending
// order.  No atomics anywhere: the same plan gives the same bits.
#include "nbx_common.h"

namespace {

#ifndef NBX_RDM_WAVE
#define NBX_RDM_WAVE 64  // (the host build of tests/test_host_fci_rdm.py runs one thread per workgroup: a wavefront of one)
#endif
constexpr int RDM_WAVE = NBX_RDM_WAVE;
// (the row cap and the block shape of fci.hip, which stages the same rows)
constexpr int64_t RDM_MAX_ROW = 13 * 1024;
constexpr int RDM_LDS_ATTR = (int)(RDM_MAX_ROW * sizeof(double));

inline unsigned rdm_grid(int64_t n, int block = 256) {
    int64_t g = nbx_cdiv(n, block);
    if (g > 262144) g = 262144;  // grid-stride loops below
    if (g < 1) g = 1;
    return (unsigned)g;
}

inline int rdm_block(int64_t nb) { return nb <= 1024 ? 256 : 1024; }

// ---------------------------------------------------------------- Graw -> dm1 (2,n,n), dm2 (3,n,n,n,n), <b|c>
// One thread per output element; every element is written.  graw: (slabs, 2n^2 + 1, 2n^2 + 1), summed in ascending
// slab order.  Row (s, k, l) of Graw carries E^s_lk, column (t, m, n) carries E^t_mn.
__global__ __launch_bounds__(256) void rdm_finish_kernel(int64_t n, int64_t slabs, const double* __restrict__ graw,
                                                         double* __restrict__ dm1, double* __restrict__ dm2,
                                                         double* __restrict__ overlap) {
    const int64_t n2 = n * n, n4 = n2 * n2, g1 = 2 * n2 + 1, gg = g1 * g1;
    const int64_t total = 3 * n4 + 2 * n2 + 1;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        if (idx < 3 * n4) {
            const int64_t x = idx / n4, pqrs = idx - x * n4;
            const int64_t p = pqrs / (n2 * n), q = (pqrs / n2) % n, r = (pqrs / n) % n, s = pqrs % n;
            const int64_t sg = x == 1 ? 1 : 0, tg = x == 0 ? 0 : 1;
            const int64_t e2 = (sg * n2 + s * n + p) * g1 + (tg * n2 + q * n + r);  // E^s_ps E^t_qr
            double v = 0.0;
            for (int64_t z = 0; z < slabs; ++z) v += graw[z * gg + e2];
            if (sg == tg && q == s) {  // - <b| E^s_pr |c>
                const int64_t e1 = (sg * n2 + r * n + p) * g1 + 2 * n2;
                double w = 0.0;
                for (int64_t z = 0; z < slabs; ++z) w += graw[z * gg + e1];
                v -= w;
            }
            dm2[idx] = v;
        } else if (idx < 3 * n4 + 2 * n2) {
            const int64_t j = idx - 3 * n4, sg = j / n2, pq = j - sg * n2, p = pq / n, q = pq - p * n;
            const int64_t e1 = (sg * n2 + q * n + p) * g1 + 2 * n2;  // <b| E^s_pq |c>
            double w = 0.0;
            for (int64_t z = 0; z < slabs; ++z) w += graw[z * gg + e1];
            dm1[j] = w;
        } else {
            double w = 0.0;
            for (int64_t z = 0; z < slabs; ++z) w += graw[z * gg + gg - 1];
            overlap[0] = w;
        }
    }
}

// ---------------------------------------------------------------- partial[Ia, (spin, k, l)] = sum_Ib b[Ia, Ib] <Ia Ib| E_kl |c>
// As gather_kernel of fci.hip: <K| E_kl |J> = <J| E_lk |K>, the source of (k, l) at K is what E_lk makes of K.  The ket
// row is staged in LDS for the beta generators, which permute within it; an alpha generator reads the linked row of
// the ket from memory.  Wavefront w takes the generators g = w, w + nwave, ...: each lane sums its elements of the row
// in ascending order, the lanes meet in the butterfly of nbx_wave_sum (a tree of fixed shape), lane 0 writes.
__global__ __launch_bounds__(1024) void rdm1_kernel(int n, int64_t Nb, const int* __restrict__ link_a,
                                                    const int* __restrict__ link_bt, const double* __restrict__ b,
                                                    const double* __restrict__ c, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) double srow[];
    const int n2 = n * n;
    const int64_t ia = blockIdx.x;
    const double* crow = c + ia * Nb;
    const double* brow = b + ia * Nb;
    for (int64_t kb = threadIdx.x; kb < Nb; kb += blockDim.x) srow[kb] = crow[kb];
    __syncthreads();
    const int lane = threadIdx.x % RDM_WAVE, wave = threadIdx.x / RDM_WAVE, nwave = blockDim.x / RDM_WAVE;
    const int* la = link_a + ia * n2;
    double* out = partial + ia * (int64_t)(2 * n2);
    for (int g2 = wave; g2 < 2 * n2; g2 += nwave) {  // (uniform over the wavefront)
        const int spin = g2 >= n2, g = g2 - spin * n2;
        const int k = g / n, l = g - k * n, lk = l * n + k;
        double acc = 0.0;
        if (spin == 0) {
            const int t = la[lk];
            if (t != 0) {
                const double* src = c + (int64_t)((t < 0 ? -t : t) - 1) * Nb;
                for (int64_t kb = lane; kb < Nb; kb += RDM_WAVE) acc += brow[kb] * src[kb];
                if (t < 0) acc = -acc;
            }
        } else {
            const int* lb = link_bt + (int64_t)lk * Nb;
            for (int64_t kb = lane; kb < Nb; kb += RDM_WAVE) {
                const int u = lb[kb];
                if (u != 0) acc += brow[kb] * (u < 0 ? -srow[-u - 1] : srow[u - 1]);
            }
        }
        acc = nbx_wave_sum(acc);
        if (lane == 0) out[g2] = acc;
    }
}

// dm1[g] = sum_Ia partial[Ia, g], Ia ascending; one thread per g
__global__ __launch_bounds__(256) void rdm1_reduce_kernel(int64_t g2, int64_t Na, const double* __restrict__ partial,
                                                          double* __restrict__ dm1) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < g2; g += (int64_t)gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int64_t ia = 0; ia < Na; ++ia) acc += partial[ia * g2 + g];
        dm1[g] = acc;
    }
}

}  // namespace

extern "C" {

int nbx_fci_rdm_finish(nbx_ctx* ctx, int64_t n, int64_t slabs, const double* d_graw, double* d_dm1, double* d_dm2,
                       double* d_overlap) {
    NBX_CHECK_ARG(ctx && n > 0 && n <= 31 && slabs > 0 && slabs <= 65535 && d_graw && d_dm1 && d_dm2 && d_overlap);
    const int64_t total = 3 * n * n * n * n + 2 * n * n + 1;
    hipLaunchKernelGGL(rdm_finish_kernel, dim3(rdm_grid(total)), dim3(256), 0, ctx->stream, n, slabs, d_graw, d_dm1, d_dm2,
                       d_overlap);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_fci_rdm1(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, const int* d_link_a,
                 const int* d_link_bt, const double* d_bra, const double* d_ket, double* d_partial, double* d_dm1) {
    NBX_CHECK_ARG(ctx && d_link_a && d_link_bt && d_bra && d_ket && d_partial && d_dm1);
    NBX_CHECK_ARG(d_partial != d_bra && d_partial != d_ket && d_dm1 != d_partial);
    NBX_CHECK_ARG(n > 0 && n <= 31 && n_alpha_str > 0 && n_beta_str > 0 && n_alpha_str < (1ll << 30));
    if (n_beta_str > RDM_MAX_ROW) {
        nbx_set_error("nbx_fci: a row of %lld beta strings exceeds the %lld the kernels stage in LDS", (long long)n_beta_str,
                      (long long)RDM_MAX_ROW);
        return NBX_E_UNSUPPORTED;
    }
    static bool attr_done = false;
    if (!attr_done) {
        NBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rdm1_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    RDM_LDS_ATTR));
        attr_done = true;
    }
    hipLaunchKernelGGL(rdm1_kernel, dim3((unsigned)n_alpha_str), dim3(rdm_block(n_beta_str)),
                       (size_t)n_beta_str * sizeof(double), ctx->stream, (int)n, n_beta_str, d_link_a, d_link_bt, d_bra, d_ket,
                       d_partial);
    NBX_LAUNCH_CHECK();
    const int64_t g2 = 2 * n * n;
    hipLaunchKernelGGL(rdm1_reduce_kernel, dim3((unsigned)nbx_cdiv(g2, 256)), dim3(256), 0, ctx->stream, g2, n_alpha_str,
                       d_partial, d_dm1);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // extern "C"
