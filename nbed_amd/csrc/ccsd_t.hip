// Perturbative triples of the spin-orbital CCSD on the device (include/nbx.h, "coupled cluster", (T)).
//
// The v x v^2 x v products that build a cube W[a,b,c] of one occupied triple i < j < k are nbx_gemm calls
// (nbed_amd/ccsd_gpu.py); this kernel does the rest in one pass over a batch of cubes: the three-index antisymmetriser
//      w = W[a,b,c] - W[b,a,c] - W[c,b,a],
// the nine-term disconnected part, the semicanonical denominator and the energy sum over a < b < c.  No atomics: every
// workgroup stores its partial sum, a second one-workgroup kernel adds the partials in a fixed order.
#include "nbx_common.h"

namespace {

// Tile of the cube: TT along a and along c, TB along b.  The three reads are W[a,b,c], W[b,a,c] (both contiguous along
// c) and W[c,b,a] (contiguous along a), so a and c both want a long edge -- 16 doubles = one 128-byte line -- and b,
// never the fastest index of a read, takes the short one.  3 x 16 x 4 x 16 doubles = 24.8 KB of LDS with the padding.
constexpr int TT = 16;
constexpr int TB = 4;
// row stride (doubles) of the tile that is read transposed, s3[c][b][a]: with 66 = 2 (mod 32) the 32 lanes of one
// ds_read_b64 group (c = 0..15, two values of a) fall on 2c + a, 32 different 8-byte bank pairs
constexpr int S3 = TB * TT + 2;

__global__ __launch_bounds__(256) void triples_energy_kernel(int no, int nv, int nta, int ntb, const double* __restrict__ cubes,
                                                             const int* __restrict__ ijk, const double* __restrict__ t1,
                                                             const double* __restrict__ fov, const double* __restrict__ t2,
                                                             const double* __restrict__ oovv, const double* __restrict__ eo,
                                                             const double* __restrict__ ev, double* __restrict__ partial) {
    __shared__ double s1[TT * TB * TT];  // [a][b][c] = W[a,b,c]
    __shared__ double s2[TB * TT * TT];  // [b][a][c] = W[b,a,c]
    __shared__ double s3[TT * S3];       // [c][b][a] = W[c,b,a]
    __shared__ double red[17];
    int blk = blockIdx.x;
    const int tc = blk % nta; blk /= nta;
    const int tb = blk % ntb;
    const int ta = blk / ntb;
    const int a0 = ta * TT, b0 = tb * TB, c0 = tc * TT;
    const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    // is there any a < b < c in this tile?  (the same answer in every thread)
    const int bmax = min(b0 + TB, nv) - 1, cmax = min(c0 + TT, nv) - 1;
    const int bmin = max(a0 + 1, b0);
    if (a0 >= nv || bmin > bmax || bmin + 1 > cmax) {
        if (threadIdx.x == 0) partial[slot] = 0.0;
        return;
    }
    const int x = threadIdx.x & (TT - 1), y = threadIdx.x >> 4;  // 16 x 16
    const double* __restrict__ w = cubes + (int64_t)blockIdx.y * nv * nv * nv;
    const int64_t v1 = nv, v2 = (int64_t)nv * nv;
#pragma unroll
    for (int b = 0; b < TB; ++b) {
        const bool in_b = b0 + b < nv;
        const bool in1 = in_b && a0 + y < nv && c0 + x < nv;  // (rows a0 + y, columns c0 + x)
        s1[(y * TB + b) * TT + x] = in1 ? w[(a0 + y) * v2 + (b0 + b) * v1 + (c0 + x)] : 0.0;
        s2[(b * TT + y) * TT + x] = in1 ? w[(b0 + b) * v2 + (a0 + y) * v1 + (c0 + x)] : 0.0;
        const bool in3 = in_b && c0 + y < nv && a0 + x < nv;  // (rows c0 + y, columns a0 + x)
        s3[y * S3 + b * TT + x] = in3 ? w[(c0 + y) * v2 + (b0 + b) * v1 + (a0 + x)] : 0.0;
    }
    __syncthreads();

    const int i = ijk[3 * blockIdx.y], j = ijk[3 * blockIdx.y + 1], k = ijk[3 * blockIdx.y + 2];
    const int a = a0 + y, c = c0 + x;
    const int ac = min(a, nv - 1), cc = min(c, nv - 1);  // (clamped: loads stay inside the arrays for idle threads)
    // the occupied side of P(i/jk): (p | q r) = (i | j k), -(j | i k), +(k | i j)   [ -(k | j i) with q < r ]
    const int po[3] = {i, j, k};
    const int64_t qr[3] = {((int64_t)j * no + k) * v2, ((int64_t)i * no + k) * v2, ((int64_t)i * no + j) * v2};
    double t1a[3], fa[3], t1c[3], fc[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        t1a[p] = t1[(int64_t)po[p] * nv + ac];
        fa[p] = fov[(int64_t)po[p] * nv + ac];
        t1c[p] = t1[(int64_t)po[p] * nv + cc];
        fc[p] = fov[(int64_t)po[p] * nv + cc];
    }
    const double e3 = (eo[i] + eo[j]) + eo[k];
    double acc = 0.0;
#pragma unroll
    for (int bb = 0; bb < TB; ++bb) {
        const int b = b0 + bb;
        if (a < b && b < c && c < nv) {
            const double wv = (s1[(y * TB + bb) * TT + x] - s2[(bb * TT + y) * TT + x]) - s3[x * S3 + bb * TT + y];
            // the virtual side of P(a/bc): (x | y z) = (a | b c), -(b | a c), +(c | a b)
            const int64_t bc = b * v1 + c, ac2 = a * v1 + c, ab = a * v1 + b;
            double td = 0.0;
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const double t1b = t1[(int64_t)po[p] * nv + b], fb = fov[(int64_t)po[p] * nv + b];
                const double* __restrict__ g = oovv + qr[p];
                const double* __restrict__ t = t2 + qr[p];
                const double term = ((t1a[p] * g[bc] + fa[p] * t[bc]) - (t1b * g[ac2] + fb * t[ac2])) +
                                    (t1c[p] * g[ab] + fc[p] * t[ab]);
                td = p == 1 ? td - term : td + term;
            }
            const double den = e3 - ((ev[a] + ev[b]) + ev[c]);
            acc += wv * (wv + td) / den;
        }
    }
    const double total = nbx_block_sum(acc, red);
    if (threadIdx.x == 0) partial[slot] = total;
}

// out[0] = sum of n partials: thread t adds t, t + 256, ... in that order, then the fixed tree of nbx_block_sum
__global__ __launch_bounds__(256) void triples_reduce_kernel(int64_t n, const double* __restrict__ partial,
                                                             double* __restrict__ out) {
    __shared__ double red[17];
    double acc = 0.0;
    for (int64_t idx = threadIdx.x; idx < n; idx += 256) acc += partial[idx];
    const double total = nbx_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = total;
}

}  // namespace

extern "C" {

size_t nbx_ccsd_triples_worksize(int64_t nvir, int64_t ncubes) {
    if (nvir < 3 || ncubes <= 0) return 0;
    const int64_t nta = nbx_cdiv(nvir, TT), ntb = nbx_cdiv(nvir, TB);
    return (size_t)(nta * ntb * nta * ncubes) * sizeof(double);
}

int nbx_ccsd_triples_tile(void) { return TT; }

int nbx_ccsd_triples_energy(nbx_ctx* ctx, int64_t nocc, int64_t nvir, int64_t ncubes, const double* d_cubes,
                            const int* d_ijk, const double* d_t1, const double* d_fov, const double* d_t2,
                            const double* d_oovv, const double* d_eo, const double* d_ev, void* d_work,
                            size_t work_bytes, double* d_energy) {
    NBX_CHECK_ARG(ctx && nocc >= 0 && nvir >= 0 && nocc < 32768 && nvir < 32768 && ncubes >= 0 && ncubes <= 65535);
    NBX_CHECK_ARG(d_energy != nullptr);
    if (nocc < 3 || nvir < 3 || ncubes == 0) {  // no triple: the sum is empty
        NBX_HIP(hipMemsetAsync(d_energy, 0, sizeof(double), ctx->stream));
        return NBX_OK;
    }
    NBX_CHECK_ARG(d_cubes && d_ijk && d_t1 && d_fov && d_t2 && d_oovv && d_eo && d_ev && d_work);
    const int64_t nta = nbx_cdiv(nvir, TT), ntb = nbx_cdiv(nvir, TB);
    const int64_t tiles = nta * ntb * nta;
    NBX_CHECK_ARG(tiles < (1ll << 31));
    if (work_bytes < nbx_ccsd_triples_worksize(nvir, ncubes)) {
        nbx_set_error("nbx_ccsd_triples_energy: workspace of %zu bytes, %zu needed", work_bytes,
                      nbx_ccsd_triples_worksize(nvir, ncubes));
        return NBX_E_NOMEM;
    }
    double* d_partials = (double*)d_work;  // one slot per workgroup, every one of them written
    hipLaunchKernelGGL(triples_energy_kernel, dim3((unsigned)tiles, (unsigned)ncubes), dim3(256), 0, ctx->stream, (int)nocc,
                       (int)nvir, (int)nta, (int)ntb, d_cubes, d_ijk, d_t1, d_fov, d_t2, d_oovv, d_eo, d_ev, d_partials);
    NBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(triples_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, tiles * ncubes, d_partials, d_energy);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // extern "C"
