// libnbx: batched symmetric eigensolver (include/nbx.h "symmetric eigensolver").
//
// Cyclic two-sided Jacobi with the round-robin ("chess tournament") parallel ordering,
// one workgroup per matrix.  The rows/columns are kept PHYSICALLY permuted so that the
// N/2 disjoint pivot pairs of a step are always the adjacent index pairs (2k, 2k+1):
//   * every 2x2 block (I,K) of A is then two 16-byte loads, rotated independently of all
//     other blocks as  J_I^T A_IK J_K  -- no reductions, no atomics;
//   * the results are scattered to the next step's positions (ping-pong buffers), so one
//     barrier separates the steps.
// Eigenvectors: V <- V J with the same column permutation.  Rotation angles use
// Rutishauser's formulas; a pivot is skipped once |a_pq| <= eps * sqrt(|a_pp a_qq|), which
// preserves high relative accuracy on graded matrices (the mu-shifted Fock matrix has
// eigenvalues of order 1e6 next to order 1).  Converged when a whole sweep rotates nothing.
//
// Matrices live in global memory (L2-resident: 4 * N^2 doubles of workspace per matrix);
// the solver is latency-bound for the N <= ~400 of the dense-ERI regime.
#include <cstdlib>

#include "nbx_common.h"

namespace {

constexpr int EIGH_THREADS = 1024;
constexpr int EIGH_MAX_SWEEPS = 40;
constexpr double EIGH_PAD_VALUE = 1.0e300;

// next-step position of the row/column currently at position i (m = number of pairs)
__device__ __forceinline__ int rr_next(int i, int m) {
    if (m == 1) return i;
    const int k = i >> 1;
    if ((i & 1) == 0) {  // top row
        if (k == 0) return 0;
        if (k == m - 1) return 2 * m - 1;
        return 2 * (k + 1);
    }
    // bottom row
    if (k == 0) return 2;
    return 2 * k - 1;
}

__global__ __launch_bounds__(EIGH_THREADS) void eigh_jacobi_kernel(const double* __restrict__ a_in, int N,
                                                                   double* __restrict__ w_out,
                                                                   double* __restrict__ v_out,
                                                                   double* __restrict__ work,
                                                                   int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int NP = (N + 1) & ~1;
    const int m = NP / 2;
    double* cs = smem;            // [3*m]: c, s, t per pair
    double* dg = cs + 3 * m;      // [NP] diagonal (sorting)
    int* rank = reinterpret_cast<int*>(dg + NP);  // [NP]
    int& nrot = rank[NP];            // rotations in the current sweep
    int& nrot_step = rank[NP + 1];   // rotations in the current step

    const int b = blockIdx.x;
    const int64_t np2 = (int64_t)NP * NP;
    a_in += (int64_t)b * N * N;
    w_out += (int64_t)b * N;
    v_out += (int64_t)b * N * N;
    double* A0 = work + (int64_t)b * 4 * np2;
    double* A1 = A0 + np2;
    double* V0 = A1 + np2;
    double* V1 = V0 + np2;

    const int tid = threadIdx.x;
    for (int64_t i = tid; i < np2; i += EIGH_THREADS) {
        const int r = (int)(i / NP), c = (int)(i - (int64_t)r * NP);
        double v = 0.0;
        if (r < N && c < N) v = a_in[(int64_t)r * N + c];
        else if (r == c) v = EIGH_PAD_VALUE;
        A0[i] = v;
        V0[i] = (r == c) ? 1.0 : 0.0;
    }
    __syncthreads();

    const double eps = 2.220446049250313e-16;
    const int steps = (m == 1) ? 1 : NP - 1;
    double* Ac = A0;
    double* An = A1;
    double* Vc = V0;
    double* Vn = V1;
    int sweep = 0;
    bool converged = false;
    for (; sweep < EIGH_MAX_SWEEPS && !converged; ++sweep) {
        if (tid == 0) nrot = 0;
        for (int step = 0; step < steps; ++step) {
            if (tid == 0) nrot_step = 0;
            __syncthreads();
            // ---- phase A: rotation parameters of the m adjacent pairs
            if (tid < m) {
                const int p = 2 * tid;
                const double app = Ac[(int64_t)p * NP + p];
                const double aqq = Ac[(int64_t)(p + 1) * NP + p + 1];
                const double apq = Ac[(int64_t)p * NP + p + 1];
                double c = 1.0, s = 0.0, t = 0.0;
                const double aa = fabs(apq);
                if (aa > eps * sqrt(fabs(app) * fabs(aqq)) && aa > 1.0e-290) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double at = fabs(theta);
                    t = 1.0 / (at + sqrt(at * at + 1.0));
                    if (at > 1.0e150) t = 0.5 / at;
                    if (theta < 0.0) t = -t;
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    atomicAdd(&nrot_step, 1);
                }
                cs[3 * tid] = c;
                cs[3 * tid + 1] = s;
                cs[3 * tid + 2] = t;
            }
            __syncthreads();
            const bool any = nrot_step > 0;
            if (tid == 0 && any) nrot += nrot_step;
            // ---- phase B: A' = P^T (J^T A J) P,  V' = V J P.  Items are processed four at a
            // time with all loads issued before the first store: stores and loads share the
            // in-order vmcnt counter, so interleaving them would serialise on store latency.
            {
                const double* __restrict__ src = Ac;
                double* __restrict__ dst = An;
                constexpr int U = 4;
                for (int base = tid; base < m * m; base += U * EIGH_THREADS) {
                    double2 r0[U], r1[U];
                    int II[U], KK[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int item = base + u * EIGH_THREADS;
                        II[u] = -1;
                        if (item < m * m) {
                            II[u] = item / m;
                            KK[u] = item - II[u] * m;
                            r0[u] = *reinterpret_cast<const double2*>(src + (int64_t)(2 * II[u]) * NP + 2 * KK[u]);
                            r1[u] = *reinterpret_cast<const double2*>(src + (int64_t)(2 * II[u] + 1) * NP + 2 * KK[u]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (II[u] < 0) continue;
                        const int I = II[u], K = KK[u];
                        double b00 = r0[u].x, b01 = r0[u].y, b10 = r1[u].x, b11 = r1[u].y;
                        if (any) {
                            const double ci = cs[3 * I], si = cs[3 * I + 1];
                            const double ck = cs[3 * K], sk = cs[3 * K + 1];
                            if (I == K) {
                                const double t = cs[3 * I + 2];
                                b00 = r0[u].x - t * r0[u].y;
                                b11 = r1[u].y + t * r0[u].y;
                                if (t != 0.0) {
                                    b01 = 0.0;
                                    b10 = 0.0;
                                }
                            } else {
                                // rows: J_I^T = [[c,-s],[s,c]]; cols: J_K = [[c,s],[-s,c]]
                                const double u00 = ci * r0[u].x - si * r1[u].x, u01 = ci * r0[u].y - si * r1[u].y;
                                const double u10 = si * r0[u].x + ci * r1[u].x, u11 = si * r0[u].y + ci * r1[u].y;
                                b00 = u00 * ck - u01 * sk;
                                b01 = u00 * sk + u01 * ck;
                                b10 = u10 * ck - u11 * sk;
                                b11 = u10 * sk + u11 * ck;
                            }
                        }
                        const int ri0 = rr_next(2 * I, m), ri1 = rr_next(2 * I + 1, m);
                        const int ck0 = rr_next(2 * K, m), ck1 = rr_next(2 * K + 1, m);
                        dst[(int64_t)ri0 * NP + ck0] = b00;
                        dst[(int64_t)ri0 * NP + ck1] = b01;
                        dst[(int64_t)ri1 * NP + ck0] = b10;
                        dst[(int64_t)ri1 * NP + ck1] = b11;
                    }
                }
                const double* __restrict__ vsrc = Vc;
                double* __restrict__ vdst = Vn;
                for (int base = tid; base < NP * m; base += U * EIGH_THREADS) {
                    double2 v[U];
                    int RR[U], KK[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int item = base + u * EIGH_THREADS;
                        RR[u] = -1;
                        if (item < NP * m) {
                            RR[u] = item / m;
                            KK[u] = item - RR[u] * m;
                            v[u] = *reinterpret_cast<const double2*>(vsrc + (int64_t)RR[u] * NP + 2 * KK[u]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (RR[u] < 0) continue;
                        const int K = KK[u];
                        double v0 = v[u].x, v1 = v[u].y;
                        if (any) {
                            const double ck = cs[3 * K], sk = cs[3 * K + 1];
                            v0 = ck * v[u].x - sk * v[u].y;
                            v1 = sk * v[u].x + ck * v[u].y;
                        }
                        vdst[(int64_t)RR[u] * NP + rr_next(2 * K, m)] = v0;
                        vdst[(int64_t)RR[u] * NP + rr_next(2 * K + 1, m)] = v1;
                    }
                }
            }
            __syncthreads();
            double* tA = Ac; Ac = An; An = tA;
            double* tV = Vc; Vc = Vn; Vn = tV;
        }
        __syncthreads();
        converged = (nrot == 0);
        __syncthreads();
    }

    // ---- sort ascending and write out (padded index carries EIGH_PAD_VALUE -> last)
    for (int i = tid; i < NP; i += EIGH_THREADS) dg[i] = Ac[(int64_t)i * NP + i];
    __syncthreads();
    for (int i = tid; i < NP; i += EIGH_THREADS) {
        const double di = dg[i];
        int rk = 0;
        for (int j = 0; j < NP; ++j) {
            const double dj = dg[j];
            rk += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        rank[i] = rk;
        if (rk < N) w_out[rk] = di;
    }
    __syncthreads();
    for (int64_t item = tid; item < (int64_t)N * NP; item += EIGH_THREADS) {
        const int r = (int)(item / NP), i = (int)(item - (int64_t)r * NP);
        const int rk = rank[i];
        if (rk < N) v_out[(int64_t)r * N + rk] = Vc[(int64_t)r * NP + i];
    }
    if (tid == 0) status[b] = converged ? sweep : -sweep;
}

__global__ void pow_kernel(int64_t n, double p, const double* __restrict__ w, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pow(w[i], p);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

static size_t eigh_global_worksize(int64_t n, int64_t batch) {
    const int64_t np = (n + 1) & ~1ll;
    return align256((size_t)(4 * np * np * batch) * sizeof(double)) + align256((size_t)batch * sizeof(int));
}

static size_t eigh_jacobi_global_total(int64_t n, int64_t batch) {
    // global-memory Jacobi + (for warm starts) V0^T A V0 and a GEMM temporary
    return eigh_global_worksize(n, batch) + 2 * align256((size_t)(n * n * batch) * sizeof(double));
}

// COLD starts of the sizes the LDS Jacobi solver covers go through the Householder / multisection /
// inverse-iteration pipeline all the same from this size on: one workgroup per matrix sweeping nine
// times is 2.98 ms at N = 148 (two matrices), the pipeline 1.93 ms (5.9 -> 3.1 ms at N = 196), with
// smaller residuals; the Jacobi solver stays the warm-start fallback and the polisher.
static bool eigh_cold_tridiag(int64_t n) {
    static const bool off = getenv("NBX_EIGH_COLD_JACOBI") != nullptr;  // A/B switch
    return !off && n >= 64 && nbx_eigh_lds_supported(n);
}

static size_t eigh_tridiag_route_worksize(int64_t n, int64_t batch) {
    // tridiagonal pipeline, then (only if needed) the Jacobi polisher, then a copy of V, then the
    // warm-start refinement buffers
    return nbx_eigh_tridiag_worksize(n, batch) + eigh_jacobi_global_total(n, batch) +
           align256((size_t)(n * n * batch) * sizeof(double)) +
           (nbx_eigh_refine_supported(n, batch) ? nbx_eigh_refine_worksize(n, batch) : 0);
}

extern "C" size_t nbx_eigh_worksize(int64_t n, int64_t batch) {
    if (n <= 0 || batch <= 0) return 0;
    if (nbx_eigh_lds_supported(n)) {
        const size_t a = nbx_eigh_lds_worksize(n, batch);
        const size_t b = eigh_cold_tridiag(n) ? nbx_eigh_tridiag_worksize(n, batch) : 0;
        return a > b ? a : b;
    }
    return eigh_tridiag_route_worksize(n, batch);
}

static int eigh_global(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, double* d_w, double* d_v,
                       void* d_work) {
    const int64_t np = (n + 1) & ~1ll;
    double* work = static_cast<double*>(d_work);
    int* status = reinterpret_cast<int*>(static_cast<char*>(d_work) +
                                         align256((size_t)(4 * np * np * batch) * sizeof(double)));
    const size_t lds = (size_t)(3 * (np / 2) + np) * sizeof(double) + (size_t)(np + 2) * sizeof(int);
    {
        nbx_prof_scope prof(ctx, NBX_PROF_EIGH);
        hipLaunchKernelGGL(eigh_jacobi_kernel, dim3((unsigned)batch), dim3(EIGH_THREADS), lds, ctx->stream, d_a,
                           (int)n, d_w, d_v, work, status);
    }
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

// Jacobi in global memory warm-started from orthonormal V0: solve V0^T A V0 = U w U^T, V = V0 U
static int eigh_global_warm(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, const double* d_v0,
                            double* d_w, double* d_v, void* d_work) {
    char* extra = static_cast<char*>(d_work) + eigh_global_worksize(n, batch);
    double* a0 = reinterpret_cast<double*>(extra);
    double* tmp = reinterpret_cast<double*>(extra + align256((size_t)(n * n * batch) * sizeof(double)));
    int rc = nbx_gemm(ctx, 'T', 'N', n, n, n, 1.0, d_v0, n, n * n, d_a, n, n * n, 0.0, tmp, n, n * n, batch);
    if (rc != NBX_OK) return rc;
    rc = nbx_gemm(ctx, 'N', 'N', n, n, n, 1.0, tmp, n, n * n, d_v0, n, n * n, 0.0, a0, n, n * n, batch);
    if (rc != NBX_OK) return rc;
    rc = eigh_global(ctx, n, batch, a0, d_w, tmp, d_work);
    if (rc != NBX_OK) return rc;
    return nbx_gemm(ctx, 'N', 'N', n, n, n, 1.0, d_v0, n, n * n, tmp, n, n * n, 0.0, d_v, n, n * n, batch);
}

extern "C" int nbx_eigh_warm(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, const double* d_v0,
                             double* d_w, double* d_v, void* d_work, size_t work_bytes) {
    return nbx_eigh_warm_ex(ctx, n, batch, d_a, d_v0, d_w, d_v, d_work, work_bytes, NBX_EIGH_REFINE_ITERS);
}

extern "C" size_t nbx_eigh_status_offset(int64_t n, int64_t batch) {
    if (n <= 0 || batch <= 0) return 0;
    if (nbx_eigh_lds_supported(n)) return nbx_eigh_lds_status_offset(n, batch);
    const int64_t np = (n + 1) & ~1ll;
    return nbx_eigh_tridiag_worksize(n, batch) + align256((size_t)(4 * np * np * batch) * sizeof(double));
}

extern "C" int nbx_eigh_warm_ex(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, const double* d_v0,
                                double* d_w, double* d_v, void* d_work, size_t work_bytes, int refine_iters) {
    NBX_CHECK_ARG(refine_iters >= 0);
    NBX_CHECK_ARG(ctx && d_a && d_w && d_v && n > 0 && batch > 0 && batch <= 1024);
    NBX_CHECK_ARG(n <= 2048);
    const size_t need = nbx_eigh_worksize(n, batch);
    if (d_work == nullptr || work_bytes < need) {
        nbx_set_error("nbx_eigh: workspace %zu < %zu bytes", work_bytes, need);
        return NBX_E_NOMEM;
    }
    NBX_CHECK_ARG((reinterpret_cast<uintptr_t>(d_work) & 15) == 0);
    if (nbx_eigh_lds_supported(n)) {
        if (d_v0 == nullptr && eigh_cold_tridiag(n)) {
            // Verdict and fallback on the device (this call sits inside queued SCF cycles -- nbx_huz_cycle -- and on
            // side streams: it must not wait for the host).  The tridiagonal route leaves 1 ("one sweep") in the
            // status word of every matrix it delivered to 1e-13, 0 otherwise (clustered spectrum the inverse
            // iteration did not resolve, NaN); the Jacobi solver is queued behind it from scratch, skipping the
            // delivered ones.  Its status words lie beyond the tridiagonal route's workspace.
            int* status = const_cast<int*>(nbx_eigh_lds_status_ptr(n, batch, d_work));
            int* skip = nbx_eigh_lds_skip_ptr(n, batch, d_work);
            const size_t td = nbx_eigh_tridiag_worksize(n, batch);
            if (nbx_eigh_lds_status_offset(n, batch) >= td) {
                int rc = nbx_eigh_tridiag_dev(ctx, n, batch, d_a, d_w, d_v, d_work, td, status, skip);
                if (rc != NBX_OK) return rc;
                return nbx_eigh_lds(ctx, n, batch, d_a, nullptr, d_w, d_v, d_work, work_bytes, refine_iters, skip);
            }
        }
        return nbx_eigh_lds(ctx, n, batch, d_a, d_v0, d_w, d_v, d_work, work_bytes, refine_iters);
    }

    // N > 196: Householder + multisection + inverse iteration; Jacobi only as a polisher.
    char* base = static_cast<char*>(d_work);
    const size_t td = nbx_eigh_tridiag_worksize(n, batch);
    char* jac = base + td;
    double* vcopy = reinterpret_cast<double*>(jac + eigh_jacobi_global_total(n, batch));
    if (d_v0 != nullptr && refine_iters > 0 && nbx_eigh_refine_supported(n, batch)) {
        // Warm start: the same GEMM-only refinement as for small N (~10 GEMMs instead of the
        // whole tridiagonal pipeline).  The pipeline below is many launches with host decisions
        // in between, so here the status words are read back (one short wait) to decide.
        char* rf = reinterpret_cast<char*>(vcopy) + align256((size_t)(n * n * batch) * sizeof(double));
        int* jstatus = reinterpret_cast<int*>(jac + align256((size_t)(4 * ((n + 1) & ~1ll) * ((n + 1) & ~1ll) * batch) *
                                                              sizeof(double)));
        const int* rstatus = nullptr;
        int rc0;
        {
            nbx_prof_scope prof(ctx, NBX_PROF_EIGH);
            rc0 = nbx_eigh_refine(ctx, n, batch, d_a, d_v0, d_w, d_v, rf, jstatus, &rstatus,
                                  refine_iters < NBX_EIGH_REFINE_MAX ? refine_iters : NBX_EIGH_REFINE_MAX);
        }
        if (rc0 != NBX_OK) return rc0;
        std::vector<int> st((size_t)batch, 0);
        rc0 = nbx_memcpy_d2h(ctx, st.data(), rstatus, (size_t)batch * sizeof(int));
        if (rc0 != NBX_OK) return rc0;
        bool all_ok = true;
        for (int v : st) all_ok = all_ok && (v > 0);
        if (all_ok) return NBX_OK;
        // otherwise solve every matrix of the batch from scratch below (results overwrite)
    }
    std::vector<double> quality((size_t)batch, 0.0);
    int rc = nbx_eigh_tridiag(ctx, n, batch, d_a, d_w, d_v, base, td, quality.data());
    if (rc != NBX_OK) return rc;
    double worst = 0.0;
    for (double q : quality) worst = q > worst ? q : worst;
    int* status = reinterpret_cast<int*>(jac + align256((size_t)(4 * ((n + 1) & ~1ll) * ((n + 1) & ~1ll) * batch) * sizeof(double)));
    if (!(worst <= 1.0e-13)) {  // also catches NaN
        rc = nbx_memcpy_d2d(ctx, vcopy, d_v, (size_t)(n * n * batch) * sizeof(double));
        if (rc != NBX_OK) return rc;
        return eigh_global_warm(ctx, n, batch, d_a, vcopy, d_w, d_v, jac);
    }
    // accepted as is: report "1 sweep" through the status words the Jacobi kernel would have written
    std::vector<int> ones((size_t)batch, 1);
    return nbx_memcpy_h2d(ctx, status, ones.data(), (size_t)batch * sizeof(int));
}

extern "C" int nbx_eigh(nbx_ctx* ctx, int64_t n, int64_t batch, const double* d_a, double* d_w, double* d_v,
                        void* d_work, size_t work_bytes) {
    return nbx_eigh_warm(ctx, n, batch, d_a, nullptr, d_w, d_v, d_work, work_bytes);
}

extern "C" int nbx_eigh_status(nbx_ctx* ctx, int64_t n, int64_t batch, const void* d_work, int* h_sweeps) {
    NBX_CHECK_ARG(ctx && d_work && h_sweeps && n > 0 && batch > 0);
    const int64_t np = (n + 1) & ~1ll;
    const char* status = static_cast<const char*>(d_work) + nbx_eigh_tridiag_worksize(n, batch) +
                         align256((size_t)(4 * np * np * batch) * sizeof(double));
    if (nbx_eigh_lds_supported(n)) status = reinterpret_cast<const char*>(nbx_eigh_lds_status_ptr(n, batch, d_work));
    int rc = nbx_memcpy_d2h(ctx, h_sweeps, status, (size_t)batch * sizeof(int));
    if (rc != NBX_OK) return rc;
    for (int64_t b = 0; b < batch; ++b)
        if (h_sweeps[b] <= 0) {
            nbx_set_error("nbx_eigh: matrix %lld did not converge in %d sweeps", (long long)b, -h_sweeps[b]);
            return NBX_E_NOCONV;
        }
    return NBX_OK;
}

extern "C" size_t nbx_sym_pow_worksize(int64_t n) {
    if (n <= 0) return 0;
    return nbx_eigh_worksize(n, 1) + align256((size_t)(2 * n * n + 2 * n) * sizeof(double));
}

extern "C" int nbx_sym_pow(nbx_ctx* ctx, int64_t n, const double* d_s, double p, double* d_out, void* d_work,
                           size_t work_bytes) {
    NBX_CHECK_ARG(ctx && d_s && d_out && n > 0);
    const size_t need = nbx_sym_pow_worksize(n);
    if (d_work == nullptr || work_bytes < need) {
        nbx_set_error("nbx_sym_pow: workspace %zu < %zu bytes", work_bytes, need);
        return NBX_E_NOMEM;
    }
    char* base = static_cast<char*>(d_work);
    const size_t ew = nbx_eigh_worksize(n, 1);
    double* u = reinterpret_cast<double*>(base + ew);  // eigenvectors
    double* us = u + n * n;                             // U * diag(w^p)
    double* w = us + n * n;
    double* wp = w + n;
    int rc = nbx_eigh(ctx, n, 1, d_s, w, u, base, ew);
    if (rc != NBX_OK) return rc;
    hipLaunchKernelGGL(pow_kernel, dim3((unsigned)nbx_cdiv(n, 256)), dim3(256), 0, ctx->stream, n, p, w, wp);
    NBX_LAUNCH_CHECK();
    rc = nbx_memcpy_d2d(ctx, us, u, (size_t)(n * n) * sizeof(double));
    if (rc != NBX_OK) return rc;
    rc = nbx_scale_cols(ctx, n, n, 1, wp, us);
    if (rc != NBX_OK) return rc;
    // out = (U diag(w^p)) U^T
    return nbx_gemm(ctx, 'N', 'T', n, n, n, 1.0, us, n, 0, u, n, 0, 0.0, d_out, n, 0, 1);
}

// ------------------------------------------------------------------ S^p by the coupled Newton-Schulz iteration, in one call
// (fractional_matrix_power(S, -1/2) of nbed/scf/huzinaga_scf.py:128, (S, 1/2) of spade.py:99, inv of concentric.py:147 for
// a symmetric positive definite S: Higham, Functions of Matrices, eq. 6.35.)  With A = S / c, c >= ||S||_inf:
//     Y_0 = A, Z_0 = I;   T = 3 I - Z Y;   Y <- Y T / 2 -> A^1/2,   Z <- T Z / 2 -> A^-1/2
// -- three products and one element-wise kernel per step, queued from here (from Python a step was four ctypes calls and
// a device copy, ~50 us of host time against ~25 us of kernels: half a millisecond of every SCF set-up at N = 148).  The
// residual ||I - Z Y||_F is read back every `check_every` steps as the host version did, with its stopping rule.
namespace {

__global__ void ns_init_kernel(int64_t n, const double* __restrict__ s, double inv_c, double* __restrict__ y, double* __restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * n) return;
    y[i] = s[i] * inv_c;
    z[i] = (i / n == i % n) ? 1.0 : 0.0;
}

// t = 3 I - p in place; partial[blockIdx.x] = this block's share of ||I - p||_F^2
__global__ __launch_bounds__(256) void ns_t_kernel(int64_t n, double* __restrict__ p, double* __restrict__ partial) {
    __shared__ double red[17];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * n; i += (int64_t)gridDim.x * blockDim.x) {
        const double d = (i / n == i % n) ? 1.0 : 0.0;
        const double v = p[i];
        const double r = d - v;
        acc = fma(r, r, acc);
        p[i] = 3.0 * d - v;
    }
    acc = nbx_block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// out = scale (a + a^T) / 2
__global__ void ns_finish_kernel(int64_t n, const double* __restrict__ a, double scale, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * n) return;
    const int64_t r = i / n, c = i % n;
    out[i] = 0.5 * scale * (a[i] + a[c * n + r]);
}

}  // namespace

extern "C" size_t nbx_sym_pow_ns_worksize(int64_t n) { return n <= 0 ? 0 : align256((size_t)(5 * n * n + 1024) * sizeof(double)); }

// p in {-1/2, +1/2, -1}; c: a bound of the spectrum (the caller's ||S||_inf).  *h_iters: steps taken, or -1 when the
// iteration did not converge within max_iter (S not positive definite, condition number beyond ~1e6) or met a NaN -- the
// caller then takes nbx_sym_pow (the eigendecomposition); d_out is only written on success.  Synchronises.
extern "C" int nbx_sym_pow_ns(nbx_ctx* ctx, int64_t n, const double* d_s, double p, double c, double* d_out, void* d_work,
                              size_t work_bytes, int max_iter, int check_every, int* h_iters) {
    NBX_CHECK_ARG(ctx && d_s && d_out && h_iters && n > 0 && c > 0.0 && max_iter > 0 && check_every > 0);
    NBX_CHECK_ARG(p == -0.5 || p == 0.5 || p == -1.0);
    if (d_work == nullptr || work_bytes < nbx_sym_pow_ns_worksize(n)) {
        nbx_set_error("nbx_sym_pow_ns: workspace %zu < %zu bytes", work_bytes, nbx_sym_pow_ns_worksize(n));
        return NBX_E_NOMEM;
    }
    const int64_t n2 = n * n;
    double* y[2] = {static_cast<double*>(d_work), static_cast<double*>(d_work) + n2};
    double* z[2] = {y[1] + n2, y[1] + 2 * n2};
    double* t = z[1] + n2;
    double* partial = t + n2;
    const unsigned eb = (unsigned)nbx_cdiv(n2, 256);
    const int tb = (int)(eb < 128 ? eb : 128);
    *h_iters = -1;
    hipLaunchKernelGGL(ns_init_kernel, dim3(eb), dim3(256), 0, ctx->stream, n, d_s, 1.0 / c, y[0], z[0]);
    NBX_LAUNCH_CHECK();
    int cur = 0;
    double prev = -1.0;
    bool converged = false;
    int last = -1;  // the step whose iterates are delivered, once the quadratic phase is reached
    int it = 0;
    for (; it < max_iter; ++it) {
        int rc = nbx_gemm(ctx, 'N', 'N', n, n, n, 1.0, z[cur], n, 0, y[cur], n, 0, 0.0, t, n, 0, 1);  // Z Y
        if (rc != NBX_OK) return rc;
        hipLaunchKernelGGL(ns_t_kernel, dim3((unsigned)tb), dim3(256), 0, ctx->stream, n, t, partial);  // T = 3 I - Z Y
        NBX_LAUNCH_CHECK();
        if (it % check_every == check_every - 1 || it == last) {
            double hp[128];
            rc = nbx_memcpy_d2h(ctx, hp, partial, (size_t)tb * sizeof(double));
            if (rc != NBX_OK) return rc;
            double ss = 0.0;
            for (int b = 0; b < tb; ++b) ss += hp[b];
            const double res = sqrt(ss);
            if (!(res == res) || res > 1.0e300) return NBX_OK;  // NaN / inf: not converged (*h_iters stays -1)
            // Z is off by r / 2 at a residual r: below 2 N eps these iterates are at rounding level already (a well
            // conditioned S sits at ~1e-15 here from its seventh step on)
            if (it == last || res < 2.0 * 2.220446049250313e-16 * (double)n) {
                converged = true;
                break;
            }
            // quadratic phase reached: a step takes the residual r to 3 r^2 / 4, so one more step reaches rounding level
            // from below 1e-8 and two from below 1e-6.  (Stopping one step after r < 1e-6 left 4e-13, and stopping AT
            // r < 1e-14 N left 5e-13 at N = 181: 16 times and 2.4 times N eps cond(S) at cond 10.)
            if (last < 0) {
                if (res < 1.0e-8 || (prev >= 0.0 && res > 0.5 * prev && res < 1.0e-9)) last = it + 1;
                else if (res < 1.0e-6) last = it + 2;
            }
            prev = res;
        }
        rc = nbx_gemm(ctx, 'N', 'N', n, n, n, 0.5, y[cur], n, 0, t, n, 0, 0.0, y[cur ^ 1], n, 0, 1);  // Y T / 2
        if (rc != NBX_OK) return rc;
        rc = nbx_gemm(ctx, 'N', 'N', n, n, n, 0.5, t, n, 0, z[cur], n, 0, 0.0, z[cur ^ 1], n, 0, 1);  // T Z / 2
        if (rc != NBX_OK) return rc;
        cur ^= 1;
    }
    if (!converged) return NBX_OK;
    const double* src = p == 0.5 ? y[cur] : z[cur];
    double scale = p == 0.5 ? sqrt(c) : 1.0 / sqrt(c);
    if (p == -1.0) {  // A^-1 = Z Z
        const int rc = nbx_gemm(ctx, 'N', 'N', n, n, n, 1.0, z[cur], n, 0, z[cur], n, 0, 0.0, t, n, 0, 1);
        if (rc != NBX_OK) return rc;
        src = t;
        scale = 1.0 / c;
    }
    hipLaunchKernelGGL(ns_finish_kernel, dim3(eb), dim3(256), 0, ctx->stream, n, src, scale, d_out);
    NBX_LAUNCH_CHECK();
    *h_iters = it + 1;
    return NBX_OK;
}
