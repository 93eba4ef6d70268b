// libnbx: AO -> MO four-index transform from a factor of the integrals (include/nbx.h "four-index transform from a
// factor").
//
//   (pq|rs) ~ sum_L B_L[p][q] B_L[r][s]   (nbx_eri_cholesky, B_L symmetric)
//   M_L^x    = C_x^T B_L C_x               x = a[, b]
//   (ij|kl)_xy = sum_L M_L^x[i][j] M_L^y[k][l]
//
// The N^4 tensor the dense transform (ao2mo.hip) reads never exists.  Three stages:
//   1  ao2mo_factor_half_kernel   P[x][L][i(i+1)/2 + j] = M_L^x[i][j], j <= i          2 naux N (N + n) nset n flop
//   2  nbx_gemm 'T','N'           G_xy = P_x^T P_y  (npair x npair, k = naux)           2 naux npair^2 flop per block
//   3  ao2mo_factor_expand_kernel out[i][j][k][l] = G[pair(i,j)][pair(k,l)]             no arithmetic
// Stage 2 holds the flops (n = 148, naux = 1203: 0.29 TFLOP per block, 0.88 TFLOP for aa, bb, ab; stage 1 is 0.04).
//
// Stage 1.  One workgroup (256 threads, four waves) owns one L and one tile of 16 columns j of the right-hand side
// [C_a | C_b] (a tile never straddles the two spins): the grid is (naux, nset * ceil(n / 16)), so every tile of one L
// re-reads B_L (8 N^2 bytes, 175 KB at N = 148) through the caches and nothing else of B.  It walks the rows p of B_L
// in chunks of 64:
//   A  T[p][j] = sum_q B_L[p][q] C[q][j]   16 rows per wave, the whole q range: the chunk's (64 x 16) piece of
//      T = B_L C, accumulated in MFMA registers, stored into LDS.  B_L[p][q] is read as B_L[q][p] (the slices are
//      symmetric), 16 adjacent doubles per k.  The tile's 16 columns of C are staged in LDS once per workgroup
//      (N <= 444; read from global memory above that).
//   B  M[i][j] += sum_(p in chunk) C[p][i] T[p][j]   for the row tiles of 16 i with i >= the tile's first j; they
//      are dealt round robin to the four waves (at most 6 each: n <= 361) and stay in accumulator registers over
//      all chunks.
// T never leaves the chip.  Both products run on v_mfma_f64_4x4x4_4b_f64 with the operand layout of gemm_m4_tn_kernel
// (gemm.hip): the A operand is a 16-row fragment (lane l: row l & 15, k = l >> 4), the B operand the four adjacent
// columns 4 (l & 3) .. + 3 at k = l >> 4, MFMA t takes column 4 (l & 3) + t, and the lane ends up with
// C[4 ((l >> 2) & 3) + (l >> 4)][4 (l & 3) + t].
//   LDS        8 KB for the chunk of T (64 x 16 doubles, 32 bytes per lane per read: four k rows are 512 contiguous
//              bytes) + 128 bytes per row of C: 26.5 KB at N = 148, 35.5 KB at N = 220, 63.5 KB at N = 444 -- five,
//              four and two workgroups per CU of its 160 KB
//   registers  6 x 4 (M) + 4 (T) accumulator doubles, 1 + 4 (phase A) or 6 + 4 (phase B) operand doubles per lane
// Operands past an edge (q, p >= N; i, j >= n) are loaded as zero, so nothing outside the arrays is read and what
// is multiplied there is 0 * finite.  Every sum has one fixed order (k ascending inside a chunk, chunks ascending),
// every address of P has one writer, nothing is atomic: two calls give the same bits.
#include "nbx_common.h"

namespace {

typedef double af_v4 __attribute__((ext_vector_type(4)));

constexpr int AF_W = 16;    // columns of [C_a | C_b] per workgroup
constexpr int AF_PC = 64;   // rows of T per chunk: 16 per wave
constexpr int AF_MAXT = 6;  // row tiles of M per wave: 4 * 6 * 16 = 384 >= 361
constexpr int AF_NMAX = 361;
constexpr int AF_CLDS_NMAX = 444;  // 8 KB of T + 16 columns of C: 63.5 KB of LDS at N = 444

size_t af_align(size_t x) { return (x + 255) & ~(size_t)255; }

extern __shared__ __attribute__((aligned(32))) double af_lds[];

// C_LDS: the tile's 16 columns of C (all N rows, zero past the edges) are staged in LDS once and phase A reads its B
// operand from there; otherwise (N > AF_CLDS_NMAX) from global memory.  Same values, same order: the same bits.
template <bool C_LDS>
__global__ __launch_bounds__(256) void ao2mo_factor_half_kernel(const double* __restrict__ B, int N, int64_t naux,
                                                                const double* __restrict__ ca, int64_t ldca,
                                                                const double* __restrict__ cb, int64_t ldcb, int n,
                                                                int tiles_per_set, double* __restrict__ P, int64_t npair,
                                                                int64_t naux_rows) {
    double* tl = af_lds;                  // (AF_PC x AF_W) chunk of T
    double* cl = af_lds + AF_PC * AF_W;   // C_LDS: ((N + 3) & ~3) x AF_W tile of C
    const int64_t L = blockIdx.x;
    const int x = (int)blockIdx.y / tiles_per_set, jt = (int)blockIdx.y - x * tiles_per_set;
    const double* __restrict__ C = x ? cb : ca;
    const int64_t ld = x ? ldcb : ldca;
    const int j0 = jt * AF_W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fk = lane >> 4, q4 = 4 * (lane & 3);
    double* __restrict__ pout = P + ((int64_t)x * naux_rows + L) * npair;
    if (L >= naux) {  // a padding row of P (the k extent of stage 2 rounded up to a multiple of 4): zeros
        for (int e = threadIdx.x; e < (n - j0) * AF_W; e += 256) {
            const int i = j0 + e / AF_W, j = j0 + e % AF_W;
            if (j < n && j <= i) pout[(int64_t)i * (i + 1) / 2 + j] = 0.0;
        }
        return;
    }
    const double* __restrict__ bl = B + L * (int64_t)N * N;
    const int nI = (n + 15) / 16;
    af_v4 acc[AF_MAXT];
#pragma unroll
    for (int s = 0; s < AF_MAXT; ++s) acc[s] = (af_v4){0.0, 0.0, 0.0, 0.0};
    if constexpr (C_LDS) {
        const int n4 = (N + 3) & ~3;
        for (int e = threadIdx.x; e < n4 * AF_W; e += 256) {
            const int q = e / AF_W, j = j0 + e % AF_W;
            cl[e] = (q < N && j < n) ? C[(int64_t)q * ld + j] : 0.0;
        }
        __syncthreads();
    }

    for (int p0 = 0; p0 < N; p0 += AF_PC) {
        // A: this wave's 16 rows of T = B_L C, columns j0 .. j0 + 15
        af_v4 tacc = (af_v4){0.0, 0.0, 0.0, 0.0};
        const int prow = p0 + 16 * wave + fr;
        for (int q0 = 0; q0 < N; q0 += 4) {
            const int q = q0 + fk;
            const bool qok = q < N;
            const double a = (qok && prow < N) ? bl[(int64_t)q * N + prow] : 0.0;
            af_v4 b;
            if constexpr (C_LDS) {
                b = *reinterpret_cast<const af_v4*>(&cl[q * AF_W + q4]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t] = (qok && j0 + q4 + t < n) ? C[(int64_t)q * ld + j0 + q4 + t] : 0.0;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) tacc[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b[t], tacc[t], 0, 0, 0);
        }
        __syncthreads();  // nobody reads the chunk before this one any more
        *reinterpret_cast<af_v4*>(&tl[(16 * wave + 4 * ((lane >> 2) & 3) + fk) * AF_W + q4]) = tacc;
        __syncthreads();
        // B: M[i][j] += sum_p C[p][i] T[p][j] over the chunk (rows of T past N are zero)
        const int pc = N - p0 < AF_PC ? N - p0 : AF_PC;
        for (int kk = 0; kk < pc; kk += 4) {
            const int p = p0 + kk + fk;
            const af_v4 b = *reinterpret_cast<const af_v4*>(&tl[(kk + fk) * AF_W + q4]);
#pragma unroll
            for (int s = 0; s < AF_MAXT; ++s) {
                const int it = jt + wave + 4 * s;  // (wave uniform)
                if (it < nI) {
                    const int i = it * 16 + fr;
                    const double a = (p < N && i < n) ? C[(int64_t)p * ld + i] : 0.0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b[t], acc[s][t], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < AF_MAXT; ++s) {
        const int it = jt + wave + 4 * s;
        if (it >= nI) continue;
        const int i = it * 16 + 4 * ((lane >> 2) & 3) + fk;
        if (i >= n) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + q4 + t;
            if (j < n && j <= i) pout[(int64_t)i * (i + 1) / 2 + j] = acc[s][t];
        }
    }
}

// out[i][j][k][l] = G[pair(i, j)][pair(k, l)], pair(a, b) = max (max + 1) / 2 + min: one workgroup per (i, j), a row of G
// gathered into n^2 contiguous doubles.  A copy: the four images of an integral are the same double.
__global__ __launch_bounds__(256) void ao2mo_factor_expand_kernel(const double* __restrict__ G, int n, int64_t npair,
                                                                  double* __restrict__ out) {
    const int64_t ij = blockIdx.x;
    const int i = (int)(ij / n), j = (int)(ij - (int64_t)i * n);
    const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
    const double* __restrict__ g = G + (hi * (hi + 1) / 2 + lo) * npair;
    double* __restrict__ o = out + ij * n * n;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int k = e / n, l = e - k * n;
        const int kh = k > l ? k : l, kl = k > l ? l : k;
        o[e] = g[kh * (kh + 1) / 2 + kl];
    }
}

int af_check_half(const char* who, nbx_ctx* ctx, int64_t nao, int64_t naux, const double* d_b, int64_t nset, const double* d_ca,
                  int64_t ldca, const double* d_cb, int64_t ldcb, int64_t n) {
    if (!(ctx && d_b && d_ca && nao > 0 && nao < (1ll << 31) && naux > 0 && naux < (1ll << 31) && (nset == 1 || nset == 2) &&
          n > 0 && ldca >= n && (nset == 1 || (d_cb && ldcb >= n)))) {
        nbx_set_error("%s: invalid argument (nao = %lld, naux = %lld, nset = %lld, n = %lld, ldca = %lld, ldcb = %lld)", who,
                      (long long)nao, (long long)naux, (long long)nset, (long long)n, (long long)ldca, (long long)ldcb);
        return NBX_E_INVALID;
    }
    if (n > AF_NMAX) {
        nbx_set_error("%s: n = %lld is more than %d orbitals (65535 pairs)", who, (long long)n, AF_NMAX);
        return NBX_E_UNSUPPORTED;
    }
    return NBX_OK;
}

int af_launch_half(nbx_ctx* ctx, int64_t nao, int64_t naux, const double* d_b, int64_t nset, const double* d_ca, int64_t ldca,
                   const double* d_cb, int64_t ldcb, int64_t n, double* d_p, int64_t naux_rows) {
    const int tiles = (int)nbx_cdiv(n, AF_W);
    const dim3 grid((unsigned)naux_rows, (unsigned)(nset * tiles));
    const double* cb = nset == 2 ? d_cb : d_ca;
    const int64_t ldb = nset == 2 ? ldcb : ldca;
    size_t lds = (size_t)AF_PC * AF_W * sizeof(double);
    if (nao <= AF_CLDS_NMAX) {
        lds += (size_t)((nao + 3) & ~(int64_t)3) * AF_W * sizeof(double);
        hipLaunchKernelGGL(ao2mo_factor_half_kernel<true>, grid, dim3(256), lds, ctx->stream, d_b, (int)nao, naux, d_ca, ldca, cb, ldb,
                           (int)n, tiles, d_p, n * (n + 1) / 2, naux_rows);
    } else {
        hipLaunchKernelGGL(ao2mo_factor_half_kernel<false>, grid, dim3(256), lds, ctx->stream, d_b, (int)nao, naux, d_ca, ldca, cb, ldb,
                           (int)n, tiles, d_p, n * (n + 1) / 2, naux_rows);
    }
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int af_launch_expand(nbx_ctx* ctx, int64_t n, const double* d_g, double* d_out) {
    hipLaunchKernelGGL(ao2mo_factor_expand_kernel, dim3((unsigned)(n * n)), dim3(256), 0, ctx->stream, d_g, (int)n, n * (n + 1) / 2,
                       d_out);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // namespace

extern "C" size_t nbx_ao2mo_factor_worksize(int64_t nao, int64_t naux, int64_t n, int64_t nset) {
    if (nao <= 0 || naux <= 0 || naux >= (1ll << 31) || n <= 0 || n > AF_NMAX || (nset != 1 && nset != 2)) return 0;
    const size_t npair = (size_t)(n * (n + 1) / 2), rows = (size_t)((naux + 3) & ~(int64_t)3);
    return af_align((size_t)nset * rows * npair * sizeof(double)) + af_align(npair * npair * sizeof(double));
}

extern "C" int nbx_ao2mo_factor_half(nbx_ctx* ctx, int64_t nao, int64_t naux, const double* d_b, int64_t nset, const double* d_ca,
                                     int64_t ldca, const double* d_cb, int64_t ldcb, int64_t n, double* d_p) {
    const int rc = af_check_half("nbx_ao2mo_factor_half", ctx, nao, naux, d_b, nset, d_ca, ldca, d_cb, ldcb, n);
    if (rc != NBX_OK) return rc;
    NBX_CHECK_ARG(d_p != nullptr);
    return af_launch_half(ctx, nao, naux, d_b, nset, d_ca, ldca, d_cb, ldcb, n, d_p, naux);
}

extern "C" int nbx_ao2mo_factor_expand(nbx_ctx* ctx, int64_t n, const double* d_g, double* d_out) {
    NBX_CHECK_ARG(ctx && d_g && d_out && n > 0);
    if (n > AF_NMAX) {
        nbx_set_error("nbx_ao2mo_factor_expand: n = %lld is more than %d orbitals (65535 pairs)", (long long)n, AF_NMAX);
        return NBX_E_UNSUPPORTED;
    }
    return af_launch_expand(ctx, n, d_g, d_out);
}

extern "C" int nbx_ao2mo_factor(nbx_ctx* ctx, int64_t nao, int64_t naux, const double* d_b, int64_t nset, const double* d_ca,
                                int64_t ldca, const double* d_cb, int64_t ldcb, int64_t n, double* d_aaaa, double* d_bbbb,
                                double* d_aabb, void* d_work, size_t work_bytes) {
    int rc = af_check_half("nbx_ao2mo_factor", ctx, nao, naux, d_b, nset, d_ca, ldca, d_cb, ldcb, n);
    if (rc != NBX_OK) return rc;
    NBX_CHECK_ARG(d_aaaa != nullptr && (nset == 1 || (d_bbbb != nullptr && d_aabb != nullptr)));
    const size_t need = nbx_ao2mo_factor_worksize(nao, naux, n, nset);
    if (d_work == nullptr || work_bytes < need) {
        nbx_set_error("nbx_ao2mo_factor: workspace %zu < %zu bytes", work_bytes, need);
        return NBX_E_NOMEM;
    }
    const int64_t npair = n * (n + 1) / 2, rows = (naux + 3) & ~(int64_t)3;
    double* p = static_cast<double*>(d_work);
    double* g = reinterpret_cast<double*>(static_cast<char*>(d_work) + af_align((size_t)(nset * rows * npair) * sizeof(double)));
    nbx_prof_scope prof_all(ctx, NBX_PROF_AO2MO);
    rc = af_launch_half(ctx, nao, naux, d_b, nset, d_ca, ldca, d_cb, ldcb, n, p, rows);
    if (rc != NBX_OK) return rc;
    // (x, y, out): aa, then bb and ab; G is reused, the stream orders product and expansion
    const int nblk = nset == 2 ? 3 : 1;
    const int64_t bx[3] = {0, 1, 0}, by[3] = {0, 1, 1};
    double* outs[3] = {d_aaaa, d_bbbb, d_aabb};
    for (int k = 0; k < nblk; ++k) {
        rc = nbx_gemm(ctx, 'T', 'N', npair, npair, rows, 1.0, p + bx[k] * rows * npair, npair, 0, p + by[k] * rows * npair, npair,
                      0, 0.0, g, npair, 0, 1);
        if (rc != NBX_OK) return rc;
        rc = af_launch_expand(ctx, n, g, outs[k]);
        if (rc != NBX_OK) return rc;
    }
    return NBX_OK;
}
