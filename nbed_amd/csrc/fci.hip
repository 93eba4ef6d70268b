// Determinant FCI on the device: what surrounds the GEMM of a Knowles-Handy sigma build (include/nbx.h, "full CI").
//
// With the spin-orbital generators E_ps = a+_p a_s,  a+_p a+_q a_r a_s = E_ps E_qr - delta_qs E_pr, so
//     H = const + sum_g k_g E_g + sum_{g g'} G[g, g'] E_g E_g',      g = (spin, p, s) in [0, 2 n^2),
// and one sigma = H c is   D[g', K] = <K| E_g' |c>   (gather),   E = [G | k] . [D ; c]   (nbx_gemm),
// sigma_I = const c_I + sum_{g K} <I| E_g |K> E[g, K]   (a gather per output element, summed in a fixed order).
// A determinant is (alpha string, beta string), the CI vector row-major (Na, Nb).  The link tables say what a
// generator does to a string:  link[S, k n + l] = sign (rank + 1) of E_kl |S>, 0 where it vanishes.  The alpha table
// is (Na, n^2) -- a workgroup owns one alpha row and reads its entries as scalars -- the beta table (n^2, Nb), so that
// the lanes of a row read it coalesced.  Alpha generators move whole rows; beta generators permute within a row,
// which is staged in LDS.  K runs over chunks of whole alpha rows [row0, row0 + rows); every determinant index is
// 64-bit (2 n^2 Ndet passes 2^31 at n = 14 (6, 6)).
#include "nbx_common.h"

namespace {

#ifndef NBX_FCI_PT
#define NBX_FCI_PT 13  // (the host build of tests/test_host_fci_kernels.py runs one thread per workgroup and raises it)
#endif
constexpr int FCI_PT = NBX_FCI_PT;                // row elements a thread of the scatter keeps in registers
constexpr int64_t FCI_MAX_ROW = FCI_PT * 1024;    // longest beta row: C(16, 8) = 12870 doubles, 104 KB of LDS
constexpr int FCI_LDS_ATTR = (int)(FCI_MAX_ROW * sizeof(double));

inline unsigned fci_grid(int64_t n, int block = 256) {
    int64_t g = nbx_cdiv(n, block);
    if (g > 262144) g = 262144;  // grid-stride loops below
    if (g < 1) g = 1;
    return (unsigned)g;
}

inline int fci_block(int64_t nb) { return nb <= 1024 ? 256 : 1024; }

// ---------------------------------------------------------------- G' = [G | k], (2 n^2, 2 n^2 + 1)
__global__ __launch_bounds__(256) void gmat_kernel(int64_t n, const double* __restrict__ one, const double* __restrict__ tb,
                                                   double* __restrict__ g) {
    const int64_t n2 = n * n, n4 = n2 * n2, rows = 2 * n2, cols = 2 * n2 + 1, total = rows * cols;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / cols, col = idx - row * cols;
        const int64_t sg = row / n2, ps = row - sg * n2, p = ps / n, s = ps - p * n;
        double v;
        if (col == rows) {  // k^sigma_ps = one[sigma][p, s] - sum_q two[sigma sigma][p, q, s, q]
            double acc = 0.0;
            for (int64_t q = 0; q < n; ++q) acc += tb[sg * n4 + ((p * n + q) * n + s) * n + q];
            v = one[sg * n2 + ps] - acc;
        } else {
            const int64_t tg = col / n2, qr = col - tg * n2, q = qr / n, r = qr - q * n;
            if (sg == tg) v = tb[sg * n4 + ((p * n + q) * n + r) * n + s];
            else if (sg == 0) v = tb[2 * n4 + ((p * n + q) * n + r) * n + s];  // (a, b, b, a)
            else v = tb[2 * n4 + ((q * n + p) * n + s) * n + r];               // (b, a, a, b) = aabb[q, p, s, r]
        }
        g[idx] = v;
    }
}

// ---------------------------------------------------------------- D[(spin, k, l), K] = <K| E_kl |c>, last row c
// <K| E_kl |J> = <J| E_lk |K>: the source of D[(k, l), K] is what E_lk makes of K.  One workgroup per alpha row of the
// chunk; cols = rows * Nb is the leading dimension of D.
__global__ __launch_bounds__(1024) void gather_kernel(int n, int64_t Nb, int64_t row0, int64_t cols, const int* __restrict__ link_a,
                              const int* __restrict__ link_bt, const double* __restrict__ c, double* __restrict__ d) {
    extern __shared__ __attribute__((aligned(16))) double srow[];
    const int n2 = n * n;
    const int64_t ka = row0 + blockIdx.x;
    const double* crow = c + ka * Nb;
    double* dcol = d + (int64_t)blockIdx.x * Nb;
    for (int64_t kb = threadIdx.x; kb < Nb; kb += blockDim.x) {
        const double v = crow[kb];
        srow[kb] = v;
        dcol[(int64_t)(2 * n2) * cols + kb] = v;
    }
    __syncthreads();
    const int* la = link_a + ka * n2;
    for (int k = 0; k < n; ++k)
        for (int l = 0; l < n; ++l) {
            const int g = k * n + l, lk = l * n + k;
            const int t = la[lk];  // (the same for the whole workgroup)
            double* da = dcol + (int64_t)g * cols;
            if (t == 0) {
                for (int64_t kb = threadIdx.x; kb < Nb; kb += blockDim.x) da[kb] = 0.0;
            } else {
                const double* src = c + (int64_t)((t < 0 ? -t : t) - 1) * Nb;
                const double sgn = t < 0 ? -1.0 : 1.0;
                for (int64_t kb = threadIdx.x; kb < Nb; kb += blockDim.x) da[kb] = sgn * src[kb];
            }
            double* db = dcol + (int64_t)(n2 + g) * cols;
            const int* lb = link_bt + (int64_t)lk * Nb;
            for (int64_t kb = threadIdx.x; kb < Nb; kb += blockDim.x) {
                const int u = lb[kb];
                db[kb] = u == 0 ? 0.0 : (u < 0 ? -srow[-u - 1] : srow[u - 1]);
            }
        }
}

// ---------------------------------------------------------------- sigma_I (+)= sum_{g K} <I| E_g |K> E[g, K]
// <I| E_ij |K>: K is what E_ji makes of I.  One workgroup per alpha row Ia of the whole vector; the alpha generators
// read row Ka - row0 of the chunk where Ka falls into it, the beta generators the row of Ia itself (staged in LDS)
// where Ia does.  Every thread sums its elements in the order (alpha ij ascending, then beta ij ascending).
__global__ __launch_bounds__(1024) void scatter_kernel(int n, int64_t Nb, int64_t row0, int64_t rows, const int* __restrict__ link_a,
                               const int* __restrict__ link_bt, const double* __restrict__ e, double shift,
                               const double* __restrict__ c, int accumulate, double* __restrict__ sigma) {
    extern __shared__ __attribute__((aligned(16))) double srow[];
    const int n2 = n * n;
    const int64_t ia = blockIdx.x, cols = rows * Nb;
    const int* la = link_a + ia * n2;
    double acc[FCI_PT];
#pragma unroll
    for (int u = 0; u < FCI_PT; ++u) acc[u] = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int t = la[j * n + i];
            if (t == 0) continue;
            const int64_t ka = (t < 0 ? -t : t) - 1;
            if (ka < row0 || ka >= row0 + rows) continue;
            const double sgn = t < 0 ? -1.0 : 1.0;
            const double* src = e + (int64_t)(i * n + j) * cols + (ka - row0) * Nb;
#pragma unroll
            for (int u = 0; u < FCI_PT; ++u) {
                const int64_t ib = threadIdx.x + (int64_t)u * blockDim.x;
                if (ib < Nb) acc[u] += sgn * src[ib];
            }
        }
    if (ia >= row0 && ia < row0 + rows) {  // (uniform over the workgroup: the barriers below are safe)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const double* src = e + (int64_t)(n2 + i * n + j) * cols + (ia - row0) * Nb;
                __syncthreads();
                for (int64_t kb = threadIdx.x; kb < Nb; kb += blockDim.x) srow[kb] = src[kb];
                __syncthreads();
                const int* lb = link_bt + (int64_t)(j * n + i) * Nb;
#pragma unroll
                for (int u = 0; u < FCI_PT; ++u) {
                    const int64_t ib = threadIdx.x + (int64_t)u * blockDim.x;
                    if (ib < Nb) {
                        const int t = lb[ib];
                        if (t != 0) acc[u] += t < 0 ? -srow[-t - 1] : srow[t - 1];
                    }
                }
            }
    }
    double* out = sigma + ia * Nb;
    const double* crow = c + ia * Nb;
#pragma unroll
    for (int u = 0; u < FCI_PT; ++u) {
        const int64_t ib = threadIdx.x + (int64_t)u * blockDim.x;
        if (ib < Nb) out[ib] = accumulate ? out[ib] + acc[u] : shift * crow[ib] + acc[u];
    }
}

// ---------------------------------------------------------------- H_II
// const + sum_{P in I} h1[P,P] + sum_{P != Q in I} (h2[P,Q,Q,P] - h2[P,Q,P,Q]), spin block by spin block
__global__ __launch_bounds__(256) void diag_kernel(int n, int64_t Na, int64_t Nb, const int* __restrict__ str_a,
                                                   const int* __restrict__ str_b, const double* __restrict__ one,
                                                   const double* __restrict__ tb, double constant,
                                                   double* __restrict__ diag) {
    const int64_t nn = n, n2 = nn * nn, n4 = n2 * n2, total = Na * Nb;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ia = idx / Nb, ib = idx - ia * Nb;
        const unsigned ma = (unsigned)str_a[ia], mb = (unsigned)str_b[ib];
        double acc = constant;
        for (int p = 0; p < n; ++p) {
            const bool pa = (ma >> p) & 1u, pb = (mb >> p) & 1u;
            if (pa) acc += one[p * nn + p];
            if (pb) acc += one[n2 + p * nn + p];
            if (!pa && !pb) continue;
            for (int q = 0; q < n; ++q) {
                const bool qa = (ma >> q) & 1u, qb = (mb >> q) & 1u;
                const int64_t pqqp = ((p * nn + q) * nn + q) * nn + p, pqpq = ((p * nn + q) * nn + p) * nn + q;
                if (pa && qa && p != q) acc += tb[pqqp] - tb[pqpq];
                if (pb && qb && p != q) acc += tb[n4 + pqqp] - tb[n4 + pqpq];
                if (pa && qb) acc += 2.0 * tb[2 * n4 + pqqp];  // (a,b,b,a) and its (b,a,a,b) image
            }
        }
        diag[idx] = acc;
    }
}

// ---------------------------------------------------------------- Davidson correction
__global__ __launch_bounds__(256) void precond_kernel(int64_t total, double theta, double guard, const double* __restrict__ r,
                                                      const double* __restrict__ diag, double* __restrict__ out) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        double den = diag[idx] - theta;
        if (fabs(den) < guard) den = den < 0.0 ? -guard : guard;
        out[idx] = r[idx] / den;
    }
}

template <class K>
int fci_lds_attr(K kernel, bool& done) {
    if (!done) {
        NBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    FCI_LDS_ATTR));
        done = true;
    }
    return NBX_OK;
}

int fci_check_shape(int64_t n, int64_t Na, int64_t Nb, int64_t row0, int64_t rows) {
    NBX_CHECK_ARG(n > 0 && n <= 31 && Na > 0 && Nb > 0 && Na < (1ll << 30) && row0 >= 0 && rows > 0 && row0 + rows <= Na);
    if (Nb > FCI_MAX_ROW) {
        nbx_set_error("nbx_fci: a row of %lld beta strings exceeds the %lld the kernels stage in LDS", (long long)Nb,
                      (long long)FCI_MAX_ROW);
        return NBX_E_UNSUPPORTED;
    }
    return NBX_OK;
}

}  // namespace

extern "C" {

int nbx_fci_gmat(nbx_ctx* ctx, int64_t n, const double* d_one_body, const double* d_two_body, double* d_g) {
    NBX_CHECK_ARG(ctx && n > 0 && n <= 31 && d_one_body && d_two_body && d_g);
    hipLaunchKernelGGL(gmat_kernel, dim3(fci_grid(2 * n * n * (2 * n * n + 1))), dim3(256), 0, ctx->stream, n, d_one_body,
                       d_two_body, d_g);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_fci_gather(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, int64_t row0, int64_t rows,
                   const int* d_link_a, const int* d_link_bt, const double* d_c, double* d_d) {
    NBX_CHECK_ARG(ctx && d_link_a && d_link_bt && d_c && d_d && d_c != d_d);
    const int rc = fci_check_shape(n, n_alpha_str, n_beta_str, row0, rows);
    if (rc != NBX_OK) return rc;
    static bool attr_done = false;
    const int ra = fci_lds_attr(gather_kernel, attr_done);
    if (ra != NBX_OK) return ra;
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)rows), dim3(fci_block(n_beta_str)), (size_t)n_beta_str * sizeof(double),
                       ctx->stream, (int)n, n_beta_str, row0, rows * n_beta_str, d_link_a, d_link_bt, d_c, d_d);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_fci_scatter(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, int64_t row0, int64_t rows,
                    const int* d_link_a, const int* d_link_bt, const double* d_e, double shift, const double* d_c,
                    int accumulate, double* d_sigma) {
    NBX_CHECK_ARG(ctx && d_link_a && d_link_bt && d_e && d_c && d_sigma && d_sigma != d_c && d_sigma != d_e);
    const int rc = fci_check_shape(n, n_alpha_str, n_beta_str, row0, rows);
    if (rc != NBX_OK) return rc;
    static bool attr_done = false;
    const int ra = fci_lds_attr(scatter_kernel, attr_done);
    if (ra != NBX_OK) return ra;
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)n_alpha_str), dim3(fci_block(n_beta_str)),
                       (size_t)n_beta_str * sizeof(double), ctx->stream, (int)n, n_beta_str, row0, rows, d_link_a, d_link_bt,
                       d_e, shift, d_c, accumulate, d_sigma);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_fci_diag(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, const int* d_str_a, const int* d_str_b,
                 const double* d_one_body, const double* d_two_body, double constant, double* d_diag) {
    NBX_CHECK_ARG(ctx && n > 0 && n <= 31 && n_alpha_str > 0 && n_beta_str > 0);
    NBX_CHECK_ARG(d_str_a && d_str_b && d_one_body && d_two_body && d_diag);
    hipLaunchKernelGGL(diag_kernel, dim3(fci_grid(n_alpha_str * n_beta_str)), dim3(256), 0, ctx->stream, (int)n, n_alpha_str,
                       n_beta_str, d_str_a, d_str_b, d_one_body, d_two_body, constant, d_diag);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_fci_precond(nbx_ctx* ctx, int64_t ndet, double theta, double guard, const double* d_r, const double* d_diag,
                    double* d_out) {
    NBX_CHECK_ARG(ctx && ndet > 0 && guard > 0.0 && d_r && d_diag && d_out);
    hipLaunchKernelGGL(precond_kernel, dim3(fci_grid(ndet)), dim3(256), 0, ctx->stream, ndet, theta, guard, d_r, d_diag,
                       d_out);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // extern "C"
