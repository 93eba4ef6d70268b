// Pivoted, incomplete Cholesky decomposition of V[pq][rs] = (pq|rs) of a real molecule:
// (pq|rs) ~ sum_L B_L[pq] B_L[rs] with the residual's diagonal <= tol, from the diagonal and the columns the
// decomposition pivots on only (eri.hip's diagonal and column sinks) -- the N^4 tensor never exists.
//
//   host    per step ONE read-back: the rank so far and the shell pairs with the largest residual diagonal; it picks the
//           pivot's shell pair and, in descending order, those of the next best ones that still fit into CD_MAXCOL
//           columns (a pair that does not fit is passed over, a smaller one after it may be taken), and builds their lists
//   device  cd_pair_max / cd_pick   the pivot search: largest d[p][q] (q <= p), fixed reduction order, ties to the lowest (p, q)
//           column sink             the fresh columns of the picked shell pairs
//           cd_gather + nbx_gemm    col[m][:] -= sum_J L_J[:] L_J[m]  (the earlier vectors)
//           cd_block                one workgroup factorises the (<= 64)^2 block of the columns at their own pivots, in
//                                   descending residual diagonal, and leaves order, roots and the triangular factor
//           cd_apply                every (p, q <= p): the forward substitution that makes the new vectors, straight
//                                   into the caller's B (both (p, q) and (q, p)), and d -= L^2
// Every sum runs in a fixed order and every address has one writer: two calls give the same bits.
#include "eri_device.h"

#include <cmath>

namespace {

using namespace nbx_eri;

constexpr int CD_MAXCOL = 64;     // columns computed in one step (a (dd| pair of Cartesian shells has 36)
constexpr int CD_PICKS = 16;      // shell pairs the pivot search offers per step
constexpr double CD_SPAN = 1e-2;  // a function pair qualifies with d > max(tol, CD_SPAN * dmax)
constexpr double CD_TOL_MIN = 1e-12;
constexpr int CD_TRI = CD_MAXCOL * (CD_MAXCOL + 1) / 2;

struct CdPick { double val; int pq; int pair; };
struct CdHead { long long rank; long long pad; CdPick pick[CD_PICKS]; };  // the read-back of a step
struct CdBlock {                                                         // cd_block_kernel -> cd_apply_kernel
    long long rank0;
    int k, pad;
    int order[CD_MAXCOL];    // column of the j-th new vector
    double root[CD_MAXCOL];  // sqrt(its residual diagonal)
    double lb[CD_TRI];       // lb[j (j + 1) / 2 + i] = L_i at the pivot of vector j, i <= j
};

// (value, p * nao + q) of the largest d[p][q], q <= p, among the function pairs of each shell pair; ties to the lowest index
__global__ void cd_pair_max_kernel(const DevShell* __restrict__ shells, const DevPair* __restrict__ pairs, int npairs, int nao,
                                   const double* __restrict__ d, double* __restrict__ pm_val, int* __restrict__ pm_pq) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npairs) return;
    const DevPair pr = pairs[t];
    const DevShell sa = shells[pr.ia], sb = shells[pr.ib];
    double best = -INFINITY;
    int at = -1;
    for (int a = 0; a < sa.nsph; ++a)
        for (int b = 0; b < (pr.ia == pr.ib ? a + 1 : sb.nsph); ++b) {
            const int pq = (sa.ao0 + a) * nao + sb.ao0 + b;
            const double v = d[pq];
            if (v > best) { best = v; at = pq; }
        }
    pm_val[t] = best;
    pm_pq[t] = at;
}

__device__ __forceinline__ bool cd_better(double v, int pq, double bv, int bpq) { return v > bv || (v == bv && pq < bpq); }

// The CD_PICKS best shell pairs in descending order (one workgroup; a pair taken is struck out of pm_val), and the rank.
__global__ __launch_bounds__(256) void cd_pick_kernel(int npairs, double* __restrict__ pm_val, const int* __restrict__ pm_pq,
                                                      const long long* __restrict__ rank, CdHead* __restrict__ head) {
    __shared__ double sv[256];
    __shared__ int spq[256], sp[256];
    const int tid = threadIdx.x;
    for (int r = 0; r < CD_PICKS; ++r) {
        double bv = -INFINITY;
        int bpq = 0x7fffffff, bp = -1;
        for (int t = tid; t < npairs; t += 256) {
            const double v = pm_val[t];
            const int pq = pm_pq[t];
            if (pq >= 0 && v > -INFINITY && cd_better(v, pq, bv, bpq)) { bv = v; bpq = pq; bp = t; }  // (-inf: struck out)
        }
        sv[tid] = bv; spq[tid] = bpq; sp[tid] = bp;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s && cd_better(sv[tid + s], spq[tid + s], sv[tid], spq[tid])) {
                sv[tid] = sv[tid + s]; spq[tid] = spq[tid + s]; sp[tid] = sp[tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) {
            head->pick[r].val = sv[0];
            head->pick[r].pq = sp[0] >= 0 ? spq[0] : -1;
            head->pick[r].pair = sp[0];
            if (sp[0] >= 0) pm_val[sp[0]] = -INFINITY;
        }
        __syncthreads();
    }
    if (tid == 0) { head->rank = *rank; head->pad = 0; }
}

// w[J][m] = L_J at the pivot of column m
__global__ void cd_gather_kernel(const double* __restrict__ b, long long n2, const int* __restrict__ col_pq, int nm,
                                 long long rank, double* __restrict__ w) {
    const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (idx >= rank * nm) return;
    const long long j = idx / nm;
    w[idx] = b[j * n2 + col_pq[idx - j * nm]];
}

// The tiny triangular part of a step, one wavefront: thread m owns column m.  Of the columns with d > max(tol, span dmax)
// the one with the largest current residual diagonal is taken next (ties to the lowest column) while that is > tol and
// max_rank is not reached; the others' entries at its pivot and their diagonals are updated in the order cd_apply uses.
__global__ __launch_bounds__(CD_MAXCOL) void cd_block_kernel(const double* __restrict__ cols, long long n2,
                                                             const int* __restrict__ col_pq, int nm, const double* __restrict__ d,
                                                             const CdHead* __restrict__ head, double tol, long long max_rank,
                                                             long long* __restrict__ rank, CdBlock* __restrict__ blk) {
    __shared__ double lb[CD_MAXCOL][CD_MAXCOL + 1], dq[CD_MAXCOL];
    __shared__ int state[CD_MAXCOL], order[CD_MAXCOL], s_pick;  // state: 0 candidate, 1 taken, 2 not qualified
    const int m = threadIdx.x;
    const double thr = fmax(tol, CD_SPAN * head->pick[0].val);
    const int pq = m < nm ? col_pq[m] : 0;
    if (m < nm) {
        dq[m] = d[pq];
        state[m] = dq[m] > thr ? 0 : 2;
    }
    __syncthreads();
    const long long rank0 = *rank;
    const long long room = max_rank - rank0;
    int k = 0;
    while (k < room && k < nm) {
        if (m == 0) {
            double best = -INFINITY;
            int at = -1;
            for (int c = 0; c < nm; ++c)
                if (state[c] == 0 && dq[c] > best) { best = dq[c]; at = c; }
            s_pick = (at >= 0 && best > tol) ? at : -1;
        }
        __syncthreads();
        const int pv = s_pick;
        if (pv < 0) break;
        const double root = sqrt(dq[pv]);
        __syncthreads();  // dq[pv] has been read by everyone before its owner updates it
        if (m < nm && state[m] == 0) {
            double v = cols[pv * n2 + pq];
            for (int i = 0; i < k; ++i) v = fma(-lb[m][i], lb[pv][i], v);
            v /= root;
            lb[m][k] = v;
            dq[m] = fma(-v, v, dq[m]);
        }
        if (m == 0) order[k] = pv;
        __syncthreads();
        if (m == 0) {
            state[pv] = 1;
            blk->root[k] = root;
        }
        ++k;
    }
    __syncthreads();
    for (int j = m; j < k; j += CD_MAXCOL) {
        blk->order[j] = order[j];
        for (int i = 0; i <= j; ++i) blk->lb[j * (j + 1) / 2 + i] = lb[order[j]][i];
    }
    if (m == 0) {
        blk->k = k;
        blk->pad = 0;
        blk->rank0 = rank0;
        *rank = rank0 + k;
    }
}

// New vectors by forward substitution, for every (p, q <= p): L_j = (col[order_j] - sum_{i<j} L_i lb[j][i]) / root_j, stored to
// B[rank0 + j] at (p, q) and (q, p), and d -= L_j^2 in the order j = 0, 1, ..  A lane keeps its L_0 .. L_{j-1} in LDS.
constexpr int CD_APPLY_BLOCK = 64;
__global__ __launch_bounds__(CD_APPLY_BLOCK) void cd_apply_kernel(const double* __restrict__ cols, long long n2, int nao,
                                                                  const CdBlock* __restrict__ blk, double* __restrict__ d,
                                                                  double* __restrict__ b) {
    __shared__ double lb[CD_TRI], root[CD_MAXCOL], l[CD_MAXCOL * CD_APPLY_BLOCK];
    __shared__ int order[CD_MAXCOL];
    const int lane = threadIdx.x;
    const int k = blk->k;
    const long long rank0 = blk->rank0;
    for (int i = lane; i < k * (k + 1) / 2; i += CD_APPLY_BLOCK) lb[i] = blk->lb[i];
    for (int i = lane; i < k; i += CD_APPLY_BLOCK) { root[i] = blk->root[i]; order[i] = blk->order[i]; }
    __syncthreads();
    // the packed triangle t = p (p + 1) / 2 + q, so that every lane has an element
    const long long ntri = (long long)nao * (nao + 1) / 2;
    for (long long t = blockIdx.x * (long long)CD_APPLY_BLOCK + lane; t < ntri; t += gridDim.x * (long long)CD_APPLY_BLOCK) {
        long long p = (long long)((sqrt(8.0 * double(t) + 1.0) - 1.0) * 0.5);
        while (p * (p + 1) / 2 > t) --p;
        while ((p + 1) * (p + 2) / 2 <= t) ++p;
        const long long q = t - p * (p + 1) / 2;
        const long long x = p * nao + q, xt = q * nao + p;
        double dx = d[x];
        for (int j = 0; j < k; ++j) {
            double v = cols[order[j] * n2 + x];
            const double* row = lb + j * (j + 1) / 2;
            for (int i = 0; i < j; ++i) v = fma(-l[i * CD_APPLY_BLOCK + lane], row[i], v);
            v /= root[j];
            l[j * CD_APPLY_BLOCK + lane] = v;
            dx = fma(-v, v, dx);
            b[(rank0 + j) * n2 + x] = v;
            b[(rank0 + j) * n2 + xt] = v;
        }
        d[x] = dx;
        d[xt] = dx;
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

thread_local int64_t t_steps = 0, t_columns = 0;

}  // namespace

extern "C" int nbx_eri_cholesky(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc,
                                const double* centres, const double* exps, const double* coefs, const double* sph,
                                double cutoff, double tol, int64_t max_rank, double* d_b, int64_t* rank_out,
                                double* resid_out) {
    NBX_CHECK_ARG(ctx != nullptr);
    NBX_CHECK_ARG(d_b != nullptr);
    NBX_CHECK_ARG(rank_out != nullptr);
    NBX_CHECK_ARG(resid_out != nullptr);
    if (!std::isfinite(tol) || tol < CD_TOL_MIN) {
        nbx_set_error("nbx_eri_cholesky: tol = %g; a finite tol >= %g is required (the integral engines agree to 2e-13, below "
                      "that the residual is not reliably positive)", tol, CD_TOL_MIN);
        return NBX_E_INVALID;
    }
    if (max_rank < 1) {
        nbx_set_error("nbx_eri_cholesky: max_rank = %lld; at least 1 is required", (long long)max_rank);
        return NBX_E_INVALID;
    }
    t_steps = t_columns = 0;
    Session s;
    int rc = session_open(ctx, nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, s);
    if (rc == NBX_E_INVALID)
        nbx_set_error("nbx_eri_cholesky: invalid shells (angular momentum 0 .. 2, nfunc = 2l+1 or (l+1)(l+2)/2)");
    if (rc != NBX_OK) return rc;
    const int64_t n = s.eng.nao, n2 = n * n;
    const int npairs = int(s.eng.pairs.size());

    // scratch of the whole call out of the stream's pool: residual diagonal, the step's columns, the gathered entries of the
    // earlier vectors, the pivot search's per-pair maxima, the columns' pivots, the rank, the read-back and the block record
    const size_t o_d = 0, o_cols = align256(o_d + sizeof(double) * n2), o_w = align256(o_cols + sizeof(double) * CD_MAXCOL * n2),
                 o_pmv = align256(o_w + sizeof(double) * CD_MAXCOL * size_t(max_rank)),
                 o_pmq = align256(o_pmv + sizeof(double) * npairs), o_pq = align256(o_pmq + sizeof(int) * npairs),
                 o_rank = align256(o_pq + sizeof(int) * CD_MAXCOL), o_head = align256(o_rank + sizeof(long long)),
                 o_blk = align256(o_head + sizeof(CdHead)), bytes = align256(o_blk + sizeof(CdBlock));
    char* d_work = nullptr;
    CdHead* h_head = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&d_work), bytes, ctx->stream) != hipSuccess) {
        session_close(s);
        nbx_set_error("nbx_eri_cholesky: %zu bytes of scratch do not fit", bytes);
        return NBX_E_NOMEM;
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&h_head), sizeof(CdHead), hipHostMallocDefault) != hipSuccess) {
        (void)hipFreeAsync(d_work, ctx->stream);
        session_close(s);
        nbx_set_error("nbx_eri_cholesky: no pinned memory for the read-back");
        return NBX_E_NOMEM;
    }
    double* d_d = reinterpret_cast<double*>(d_work + o_d);
    double* d_cols = reinterpret_cast<double*>(d_work + o_cols);
    double* d_w = reinterpret_cast<double*>(d_work + o_w);
    double* d_pmv = reinterpret_cast<double*>(d_work + o_pmv);
    int* d_pmq = reinterpret_cast<int*>(d_work + o_pmq);
    int* d_pq = reinterpret_cast<int*>(d_work + o_pq);
    long long* d_rank = reinterpret_cast<long long*>(d_work + o_rank);
    CdHead* d_head = reinterpret_cast<CdHead*>(d_work + o_head);
    CdBlock* d_blk = reinterpret_cast<CdBlock*>(d_work + o_blk);

    auto hip_fail = [&](hipError_t e, const char* what) {
        nbx_set_error("nbx_eri_cholesky: %s -> %s", what, hipGetErrorString(e));
        rc = NBX_E_HIP;
    };
    hipError_t e = hipMemsetAsync(d_rank, 0, sizeof(long long), ctx->stream);
    if (e != hipSuccess) hip_fail(e, "hipMemsetAsync");
    if (rc == NBX_OK) rc = session_diagonal(s, d_d);

    int64_t rank = 0, last_rank = -1;
    double resid = 0.0;
    const unsigned apply_grid = unsigned(std::min<int64_t>(nbx_cdiv(n * (n + 1) / 2, CD_APPLY_BLOCK), 256 * 8));
    while (rc == NBX_OK) {
        hipLaunchKernelGGL(cd_pair_max_kernel, dim3(unsigned(nbx_cdiv(npairs, 256))), dim3(256), 0, ctx->stream, s.args.shells,
                           s.args.pairs, npairs, int(n), d_d, d_pmv, d_pmq);
        hipLaunchKernelGGL(cd_pick_kernel, dim3(1), dim3(256), 0, ctx->stream, npairs, d_pmv, d_pmq, d_rank, d_head);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_head, d_head, sizeof(CdHead), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the one wait of a step
        if (e != hipSuccess) { hip_fail(e, "pivot search"); break; }
        rank = h_head->rank;
        resid = h_head->pick[0].val;
        if (!(resid > tol) || rank >= max_rank) break;
        if (rank == last_rank || h_head->pick[0].pair < 0) {
            nbx_set_error("nbx_eri_cholesky: a step appended no vector at rank %lld (residual %g)", (long long)rank, resid);
            rc = NBX_E_NOCONV;
            break;
        }
        last_rank = rank;
        // the pivot's shell pair, then the next best ones that qualify and still fit the column budget
        const double thr = std::fmax(tol, CD_SPAN * resid);
        int64_t sel[CD_PICKS];
        int nsel = 0, ncols = 0;
        for (int r = 0; r < CD_PICKS; ++r) {
            const CdPick& pk = h_head->pick[r];
            if (pk.pair < 0 || !(pk.val > thr)) break;
            const int c = pair_columns(s.eng, s.eng.pairs[size_t(pk.pair)]);
            if (ncols + c > CD_MAXCOL) continue;  // (a smaller pair further down the list may still fit)
            sel[nsel++] = pk.pair;
            ncols += c;
        }
        rc = session_columns(s, nsel, sel, d_cols, d_pq);
        if (rc != NBX_OK) break;
        if (rank > 0) {
            hipLaunchKernelGGL(cd_gather_kernel, dim3(unsigned(nbx_cdiv(rank * ncols, 256))), dim3(256), 0, ctx->stream, d_b,
                               (long long)n2, d_pq, ncols, (long long)rank, d_w);
            e = hipGetLastError();
            if (e != hipSuccess) { hip_fail(e, "cd_gather_kernel"); break; }
            rc = nbx_gemm(ctx, 'T', 'N', ncols, n2, rank, -1.0, d_w, ncols, 0, d_b, n2, 0, 1.0, d_cols, n2, 0, 1);
            if (rc != NBX_OK) break;
        }
        hipLaunchKernelGGL(cd_block_kernel, dim3(1), dim3(CD_MAXCOL), 0, ctx->stream, d_cols, (long long)n2, d_pq, ncols, d_d, d_head,
                           tol, (long long)max_rank, d_rank, d_blk);
        hipLaunchKernelGGL(cd_apply_kernel, dim3(apply_grid), dim3(CD_APPLY_BLOCK), 0, ctx->stream, d_cols, (long long)n2, int(n),
                           d_blk, d_d, d_b);
        e = hipGetLastError();
        if (e != hipSuccess) { hip_fail(e, "in-block factorisation"); break; }
        ++t_steps;
        t_columns += ncols;
    }
    if (rc != NBX_OK) (void)hipStreamSynchronize(ctx->stream);  // the session's lists may still be on their way
    (void)hipFreeAsync(d_work, ctx->stream);
    (void)hipHostFree(h_head);
    session_close(s);
    if (rc == NBX_OK) {
        *rank_out = rank;
        *resid_out = resid;
    }
    return rc;
}

extern "C" int nbx_eri_cholesky_steps(int64_t* steps, int64_t* columns) {
    if (!steps || !columns) return NBX_E_INVALID;
    *steps = t_steps;
    *columns = t_columns;
    return NBX_OK;
}
