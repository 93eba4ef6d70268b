// Spin-orbital CCSD on the device: what surrounds the GEMMs (include/nbx.h, "coupled cluster").
//
// The contractions of the amplitude equations are nbx_gemm calls; these kernels do what the host solver
// (nbed_amd/ccsd.py) does with np.ix_, transpose and broadcasting: cut antisymmetrised blocks <PQ||RS> out of the
// three spatial spin blocks, permute four-index tensors so that a contraction becomes a matrix product, pack and
// unpack antisymmetric index pairs, build tau, and divide the residual by the denominators.
#include "nbx_common.h"

namespace {

constexpr int PT = 32;  // tile edge of the permute (32 x 33 doubles of LDS)

inline unsigned cc_grid(int64_t n, int block = 256) {
    int64_t g = nbx_cdiv(n, block);
    if (g > 262144) g = 262144;  // grid-stride loops below
    if (g < 1) g = 1;
    return (unsigned)g;
}

__host__ __device__ inline int64_t npair(int64_t n) { return n * (n - 1) / 2; }

// pair index k = e (2n - e - 1) / 2 + (f - e - 1) of e < f < n (rows of the strict upper triangle) -> (e, f)
__device__ __forceinline__ void pair_decode(int64_t k, int n, int& e, int& f) {
    const double b = 2.0 * n - 1.0;
    int r = (int)((b - sqrt(b * b - 8.0 * (double)k)) * 0.5);
    if (r < 0) r = 0;
    if (r > n - 2) r = n - 2;
    while (r > 0 && (int64_t)r * (2 * n - r - 1) / 2 > k) --r;
    while (r < n - 2 && (int64_t)(r + 1) * (2 * n - r - 2) / 2 <= k) ++r;
    e = r;
    f = (int)(k - (int64_t)r * (2 * n - r - 1) / 2) + r + 1;
}

// ---------------------------------------------------------------- antisymmetrised blocks of the spatial Hamiltonian
// h2[P,Q,R,S] of SpatialHamiltonian.h2_element: alpha on the even spin-orbital indices
__device__ __forceinline__ double h2_element(const double* __restrict__ tb, int64_t n, int P, int Q, int R, int S) {
    const int sp = (P & 1) | ((Q & 1) << 1) | ((R & 1) << 2) | ((S & 1) << 3);
    const int64_t p = P >> 1, q = Q >> 1, r = R >> 1, s = S >> 1;
    const int64_t n4 = n * n * n * n;
    if (sp == 0) return tb[((p * n + q) * n + r) * n + s];
    if (sp == 15) return tb[n4 + ((p * n + q) * n + r) * n + s];
    if (sp == 6) return tb[2 * n4 + ((p * n + q) * n + r) * n + s];   // (a, b, b, a)
    if (sp == 9) return tb[2 * n4 + ((q * n + p) * n + s) * n + r];   // (b, a, a, b): bbaa[p,q,r,s] = aabb[q,p,s,r]
    return 0.0;
}

// ccsd.antisymmetrized(), term by term: w[p,q,r,s] = 2 h2[p,q,s,r]; g = w - w(r<->s); 0.5 (g - g(p<->q))
__device__ __forceinline__ double antisym_element(const double* __restrict__ tb, int64_t n, int P, int Q, int R, int S) {
    const double w1 = 2.0 * h2_element(tb, n, P, Q, S, R);
    const double w2 = 2.0 * h2_element(tb, n, P, Q, R, S);
    const double w3 = 2.0 * h2_element(tb, n, Q, P, S, R);
    const double w4 = 2.0 * h2_element(tb, n, Q, P, R, S);
    return 0.5 * ((w1 - w2) - (w3 - w4));
}

__global__ __launch_bounds__(256) void gather_kernel(const double* __restrict__ tb, int64_t n, const int* __restrict__ i1,
                                                     int n1, const int* __restrict__ i2, int n2,
                                                     const int* __restrict__ i3, int n3, const int* __restrict__ i4,
                                                     int n4, int pack_first, int pack_last, double* __restrict__ out) {
    const int64_t rows = pack_first ? npair(n1) : (int64_t)n1 * n2;
    const int64_t cols = pack_last ? npair(n3) : (int64_t)n3 * n4;
    const int64_t total = rows * cols;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / cols, col = idx - row * cols;
        int a, b, c, d;
        if (pack_first) pair_decode(row, n1, a, b);
        else { a = (int)(row / n2); b = (int)(row - (int64_t)a * n2); }
        if (pack_last) pair_decode(col, n3, c, d);
        else { c = (int)(col / n4); d = (int)(col - (int64_t)c * n4); }
        out[idx] = antisym_element(tb, n, i1[a], i2[b], i3[c], i4[d]);
    }
}

// f[P,Q] = h1[P,Q] + sum_{I in occ} <P I || Q I>
__global__ __launch_bounds__(256) void fock_kernel(const double* __restrict__ tb, int64_t n, const double* __restrict__ h1,
                                                   const int* __restrict__ occ, int nocc, double* __restrict__ f) {
    const int64_t nso = 2 * n, total = nso * nso;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int P = (int)(idx / nso), Q = (int)(idx - (int64_t)P * nso);
        double acc = 0.0;
        for (int i = 0; i < nocc; ++i) acc += antisym_element(tb, n, P, occ[i], Q, occ[i]);
        f[idx] = h1[idx] + acc;
    }
}

// ---------------------------------------------------------------- four-index permute
struct Perm4 {
    int64_t ext[4];   // extents of the INPUT axes
    int64_t sin[4];   // input strides
    int64_t sout[4];  // output stride of each INPUT axis
};

// the fastest axis is the same on both sides: plain copy with index arithmetic over the output
__global__ __launch_bounds__(256) void permute_same_kernel(Perm4 p, int o0, int o1, int o2, double alpha,
                                                           const double* __restrict__ in, double beta,
                                                           double* __restrict__ out) {
    // o0, o1, o2: the input axes that are output axes 0, 1, 2 (output axis 3 = input axis 3)
    const int64_t e3 = p.ext[3], e2 = p.ext[o2], e1 = p.ext[o1], e0 = p.ext[o0];
    const int64_t total = e0 * e1 * e2 * e3;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = idx;
        const int64_t x3 = r % e3; r /= e3;
        const int64_t x2 = r % e2; r /= e2;
        const int64_t x1 = r % e1; r /= e1;
        const int64_t x0 = r;
        const double v = alpha * in[x0 * p.sin[o0] + x1 * p.sin[o1] + x2 * p.sin[o2] + x3];
        out[idx] = beta == 0.0 ? v : v + beta * out[idx];
    }
}

// the fastest output axis is input axis `b` != 3: 32 x 32 tiles over (input axis 3, input axis b) through LDS, so that
// reads run along input axis 3 and writes along input axis b; the two remaining axes c, d are walked by the grid
__global__ __launch_bounds__(256) void permute_tile_kernel(Perm4 p, int b, int c, int d, int64_t tiles_a, int64_t tiles_b,
                                                           double alpha, const double* __restrict__ in, double beta,
                                                           double* __restrict__ out) {
    __shared__ double tile[PT][PT + 1];
    const int64_t ea = p.ext[3], eb = p.ext[b], ed = p.ext[d];
    int64_t blk = blockIdx.x;
    const int64_t ta = blk % tiles_a; blk /= tiles_a;
    const int64_t tb = blk % tiles_b; blk /= tiles_b;
    const int64_t xd = blk % ed, xc = blk / ed;
    const int64_t base_in = xc * p.sin[c] + xd * p.sin[d];
    const int64_t base_out = xc * p.sout[c] + xd * p.sout[d];
    const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;  // 32 x 8
    const int64_t a0 = ta * PT, b0 = tb * PT;
    for (int j = ty; j < PT; j += 8) {
        const int64_t xa = a0 + tx, xb = b0 + j;
        if (xa < ea && xb < eb) tile[j][tx] = in[base_in + xb * p.sin[b] + xa];
    }
    __syncthreads();
    for (int j = ty; j < PT; j += 8) {
        const int64_t xa = a0 + j, xb = b0 + tx;
        if (xa < ea && xb < eb) {
            const int64_t o = base_out + xa * p.sout[3] + xb;  // (sout[b] = 1)
            const double v = alpha * tile[tx][j];
            out[o] = beta == 0.0 ? v : v + beta * out[o];
        }
    }
}

// ---------------------------------------------------------------- antisymmetric pairs
// packed[l, (e<f), t] = x[l, e, f, t]
__global__ __launch_bounds__(256) void pair_pack_kernel(int64_t lead, int n, int64_t trail, const double* __restrict__ x,
                                                        double* __restrict__ packed) {
    const int64_t np_ = npair(n), total = lead * np_ * trail;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = idx % trail;
        const int64_t k = (idx / trail) % np_;
        const int64_t l = idx / (trail * np_);
        int e, f;
        pair_decode(k, n, e, f);
        packed[idx] = x[((l * n + e) * n + f) * trail + t];
    }
}

// x[l, e, f, t] = alpha * (e < f ? packed[l, ef, t] : e > f ? -packed[l, fe, t] : 0) + beta * x[l, e, f, t]
__global__ __launch_bounds__(256) void pair_unpack_kernel(int64_t lead, int n, int64_t trail, double alpha,
                                                          const double* __restrict__ packed, double beta,
                                                          double* __restrict__ x) {
    const int64_t np_ = npair(n), total = lead * n * n * trail;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = idx % trail;
        int64_t r = idx / trail;
        const int f = (int)(r % n); r /= n;
        const int e = (int)(r % n);
        const int64_t l = r / n;
        double v = 0.0;
        if (e != f) {
            const int64_t lo = e < f ? e : f, hi = e < f ? f : e;
            const int64_t k = lo * (2 * (int64_t)n - lo - 1) / 2 + (hi - lo - 1);
            const double pv = packed[(l * np_ + k) * trail + t];
            v = e < f ? pv : -pv;
        }
        v = alpha * v;
        x[idx] = beta == 0.0 ? v : v + beta * x[idx];
    }
}

// ---------------------------------------------------------------- tau
// out[i,j,a,b] = c2 t2[i,j,a,b] + cd t1[i,a] t1[j,b] - cx t1[i,b] t1[j,a]; packed: over (i<j, a<b) only
__global__ __launch_bounds__(256) void tau_kernel(int no, int nv, const double* __restrict__ t1, const double* __restrict__ t2,
                                                  double c2, double cd, double cx, int packed, double* __restrict__ out) {
    const int64_t rows = packed ? npair(no) : (int64_t)no * no, cols = packed ? npair(nv) : (int64_t)nv * nv;
    const int64_t total = rows * cols;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / cols, col = idx - row * cols;
        int i, j, a, b;
        if (packed) { pair_decode(row, no, i, j); pair_decode(col, nv, a, b); }
        else { i = (int)(row / no); j = (int)(row - (int64_t)i * no); a = (int)(col / nv); b = (int)(col - (int64_t)a * nv); }
        const double x = t2[(((int64_t)i * no + j) * nv + a) * nv + b];
        out[idx] = (c2 * x + cd * (t1[(int64_t)i * nv + a] * t1[(int64_t)j * nv + b])) -
                   cx * (t1[(int64_t)i * nv + b] * t1[(int64_t)j * nv + a]);
    }
}

// ---------------------------------------------------------------- amplitude update
// over the concatenated [t1 | t2] vector: t_new = r / D, err = t_new - t_old; max |err| into *maxerr (bit pattern of a
// non-negative double: ordered like the unsigned integer), which the caller zeroed
__global__ __launch_bounds__(256) void update_kernel(int no, int nv, const double* __restrict__ r, const double* __restrict__ told,
                                                     const double* __restrict__ eo, const double* __restrict__ ev,
                                                     double* __restrict__ tnew, double* __restrict__ err,
                                                     unsigned long long* __restrict__ maxerr) {
    __shared__ double red[17];
    const int64_t n1 = (int64_t)no * nv, total = n1 + n1 * n1;
    double m = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        double den;
        if (idx < n1) {
            const int i = (int)(idx / nv), a = (int)(idx - (int64_t)i * nv);
            den = eo[i] - ev[a];
        } else {
            int64_t k = idx - n1;
            const int b = (int)(k % nv); k /= nv;
            const int a = (int)(k % nv); k /= nv;
            const int j = (int)(k % no);
            const int i = (int)(k / no);
            den = ((eo[i] + eo[j]) - ev[a]) - ev[b];
        }
        const double tn = r[idx] / den;
        const double e = tn - told[idx];
        tnew[idx] = tn;
        err[idx] = e;
        const double ae = fabs(e);
        m = (ae > m || ae != ae) ? ae : m;  // (a NaN sticks: it shows up as "not converged", never as zero)
    }
    // workgroup maximum, then one atomic per workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = (o > m || o != o) ? o : m;
    }
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = (red[w] > m || red[w] != red[w]) ? red[w] : m;
        atomicMax(maxerr, (unsigned long long)__double_as_longlong(m));
    }
}

}  // namespace

extern "C" {

int nbx_ccsd_gather(nbx_ctx* ctx, int64_t n, const double* d_two_body, const int* d_idx1, int64_t n1, const int* d_idx2,
                    int64_t n2, const int* d_idx3, int64_t n3, const int* d_idx4, int64_t n4, int pack_first,
                    int pack_last, double* d_out) {
    NBX_CHECK_ARG(ctx && n > 0 && n < 16384 && n1 >= 0 && n2 >= 0 && n3 >= 0 && n4 >= 0);
    NBX_CHECK_ARG(n1 <= 2 * n && n2 <= 2 * n && n3 <= 2 * n && n4 <= 2 * n);
    NBX_CHECK_ARG(!pack_first || n1 == n2);
    NBX_CHECK_ARG(!pack_last || n3 == n4);
    const int64_t rows = pack_first ? npair(n1) : n1 * n2, cols = pack_last ? npair(n3) : n3 * n4;
    if (rows <= 0 || cols <= 0) return NBX_OK;
    NBX_CHECK_ARG(d_two_body && d_idx1 && d_idx2 && d_idx3 && d_idx4 && d_out);
    hipLaunchKernelGGL(gather_kernel, dim3(cc_grid(rows * cols)), dim3(256), 0, ctx->stream, d_two_body, n, d_idx1, (int)n1,
                       d_idx2, (int)n2, d_idx3, (int)n3, d_idx4, (int)n4, pack_first, pack_last, d_out);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_ccsd_fock(nbx_ctx* ctx, int64_t n, const double* d_two_body, const double* d_h1, const int* d_occ, int64_t nocc,
                  double* d_fock) {
    NBX_CHECK_ARG(ctx && n > 0 && n < 16384 && nocc >= 0 && nocc <= 2 * n && d_two_body && d_h1 && d_fock);
    NBX_CHECK_ARG(nocc == 0 || d_occ != nullptr);
    hipLaunchKernelGGL(fock_kernel, dim3(cc_grid(4 * n * n)), dim3(256), 0, ctx->stream, d_two_body, n, d_h1, d_occ, (int)nocc,
                       d_fock);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_permute4(nbx_ctx* ctx, const int64_t* h_extents, const int* h_perm, double alpha, const double* d_in, double beta,
                 double* d_out) {
    NBX_CHECK_ARG(ctx && h_extents && h_perm);
    int seen = 0;
    for (int k = 0; k < 4; ++k) {
        NBX_CHECK_ARG(h_perm[k] >= 0 && h_perm[k] < 4 && h_extents[k] >= 0);
        seen |= 1 << h_perm[k];
    }
    NBX_CHECK_ARG(seen == 15);
    const int64_t total = h_extents[0] * h_extents[1] * h_extents[2] * h_extents[3];
    if (total == 0) return NBX_OK;
    NBX_CHECK_ARG(d_in && d_out && d_in != d_out);
    Perm4 p;
    for (int k = 0; k < 4; ++k) p.ext[k] = h_extents[k];
    p.sin[3] = 1;
    for (int k = 2; k >= 0; --k) p.sin[k] = p.sin[k + 1] * p.ext[k + 1];
    int64_t so = 1;
    for (int k = 3; k >= 0; --k) {  // output axis k is input axis perm[k]
        p.sout[h_perm[k]] = so;
        so *= p.ext[h_perm[k]];
    }
    if (h_perm[3] == 3) {
        hipLaunchKernelGGL(permute_same_kernel, dim3(cc_grid(total)), dim3(256), 0, ctx->stream, p, h_perm[0], h_perm[1],
                           h_perm[2], alpha, d_in, beta, d_out);
        NBX_LAUNCH_CHECK();
        return NBX_OK;
    }
    const int b = h_perm[3];
    int rest[2], nr = 0;
    for (int k = 0; k < 3; ++k)
        if (k != b) rest[nr++] = k;
    const int64_t tiles_a = nbx_cdiv(p.ext[3], PT), tiles_b = nbx_cdiv(p.ext[b], PT);
    const int64_t blocks = tiles_a * tiles_b * p.ext[rest[0]] * p.ext[rest[1]];
    if (blocks >= (1ll << 31)) {
        nbx_set_error("nbx_permute4: %lld tiles exceed one grid", (long long)blocks);
        return NBX_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(permute_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, p, b, rest[0], rest[1],
                       tiles_a, tiles_b, alpha, d_in, beta, d_out);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_pair_pack(nbx_ctx* ctx, int64_t lead, int64_t n, int64_t trail, const double* d_x, double* d_packed) {
    NBX_CHECK_ARG(ctx && lead >= 0 && n >= 0 && n < (1 << 30) && trail >= 0);
    if (lead * npair(n) * trail == 0) return NBX_OK;
    NBX_CHECK_ARG(d_x && d_packed && d_x != d_packed);
    hipLaunchKernelGGL(pair_pack_kernel, dim3(cc_grid(lead * npair(n) * trail)), dim3(256), 0, ctx->stream, lead, (int)n,
                       trail, d_x, d_packed);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_pair_unpack(nbx_ctx* ctx, int64_t lead, int64_t n, int64_t trail, double alpha, const double* d_packed, double beta,
                    double* d_x) {
    NBX_CHECK_ARG(ctx && lead >= 0 && n >= 0 && n < (1 << 30) && trail >= 0);
    if (lead * n * n * trail == 0) return NBX_OK;
    NBX_CHECK_ARG(d_x && (d_packed || n < 2) && d_x != d_packed);
    hipLaunchKernelGGL(pair_unpack_kernel, dim3(cc_grid(lead * n * n * trail)), dim3(256), 0, ctx->stream, lead, (int)n,
                       trail, alpha, d_packed, beta, d_x);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_ccsd_tau(nbx_ctx* ctx, int64_t nocc, int64_t nvir, const double* d_t1, const double* d_t2, double c_t2,
                 double c_direct, double c_exchange, int packed, double* d_out) {
    NBX_CHECK_ARG(ctx && nocc >= 0 && nvir >= 0 && nocc < 32768 && nvir < 32768);
    const int64_t total = packed ? npair(nocc) * npair(nvir) : nocc * nocc * nvir * nvir;
    if (total == 0) return NBX_OK;
    NBX_CHECK_ARG(d_t1 && d_t2 && d_out && d_out != d_t2);
    hipLaunchKernelGGL(tau_kernel, dim3(cc_grid(total)), dim3(256), 0, ctx->stream, (int)nocc, (int)nvir, d_t1, d_t2, c_t2,
                       c_direct, c_exchange, packed, d_out);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

int nbx_ccsd_update(nbx_ctx* ctx, int64_t nocc, int64_t nvir, const double* d_r, const double* d_t_old, const double* d_eo,
                    const double* d_ev, double* d_t_new, double* d_err, double* d_maxerr) {
    NBX_CHECK_ARG(ctx && nocc > 0 && nvir > 0 && nocc < 32768 && nvir < 32768);
    NBX_CHECK_ARG(d_r && d_t_old && d_eo && d_ev && d_t_new && d_err && d_maxerr);
    NBX_HIP(hipMemsetAsync(d_maxerr, 0, sizeof(double), ctx->stream));
    const int64_t n1 = nocc * nvir;
    hipLaunchKernelGGL(update_kernel, dim3(cc_grid(n1 + n1 * n1)), dim3(256), 0, ctx->stream, (int)nocc, (int)nvir, d_r,
                       d_t_old, d_eo, d_ev, d_t_new, d_err, (unsigned long long*)d_maxerr);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // extern "C"
