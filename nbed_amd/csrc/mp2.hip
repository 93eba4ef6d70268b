// Second-order amplitudes and pair energy of one spin pair on the device (include/nbx.h, "MP2").
//
// One pass over the chemist block V[i,a,j,b] = (ia|jb): the antisymmetriser of the same-spin case, the semicanonical
// denominator, the amplitude store and the energy sum.  The same-spin case needs V[i,b,j,a] next to V[i,a,j,b], a
// transposed read: a workgroup takes an (i, j) pair and a 32 x 32 tile of (a, b) TOGETHER WITH ITS MIRROR TILE, reads
// both along b (coalesced), exchanges them through LDS and writes t for the tile and for the mirror, so that no lane
// ever reads the mirror element from memory with a stride.  The diagonal tile and a == b (an exact 0) take the same
// path.  No atomics: every workgroup stores the partial sum of the items it walked (a fixed order), a one-workgroup
// kernel adds the partials in a fixed order.
//
// Every loop over the threads of a workgroup is written with a stride of blockDim.x, so the file also runs on the
// host (tests/native/mp2_host_shim.h: one thread per workgroup, for which the barrier is trivially satisfied).
#include "nbx_common.h"

namespace {

constexpr int MT = 32;        // tile edge over (a, b)
constexpr int MS = MT + 1;    // row stride of an LDS tile in doubles: 33 x 8 bytes = 66 banks = 2 (mod 64), so the 32 lanes
                              // of one ds_read_b64 group that walk a COLUMN fall on 32 different bank pairs
constexpr int MP2_MAX_GROUPS = 4096;  // workgroups (= partial sums) of one launch; 2 x 8.25 KB of LDS each

__host__ __device__ inline int64_t mp2_tiles(int64_t nv1, int64_t nv2, int same) {
    const int64_t t1 = (nv1 + MT - 1) / MT, t2 = (nv2 + MT - 1) / MT;
    return same ? t1 * (t1 + 1) / 2 : t1 * t2;
}

// V (no1, nv1, no2, nv2) -> T (nv1, no1, no2, nv2), partial[blockIdx.x] = this workgroup's share of the pair energy.
// SAME: t = (V[i,a,j,b] - V[i,b,j,a]) / d, energy 1/4 t (V[i,a,j,b] - V[i,b,j,a]); otherwise t = V / d, energy t V.
// d = ((eo1[i] + eo2[j]) - ev1[a]) - ev2[b], in this order, for the tile and (with a and b exchanged) for the mirror.
template <bool SAME>
__global__ __launch_bounds__(256) void mp2_pairs_kernel(int no1, int nv1, int no2, int nv2, const double* __restrict__ v,
                                                        const double* __restrict__ eo1, const double* __restrict__ ev1,
                                                        const double* __restrict__ eo2, const double* __restrict__ ev2,
                                                        double* __restrict__ t, double* __restrict__ partial) {
    __shared__ double sa[MT * MS];  // [y][x] = V[i, a0 + y, j, b0 + x]
    __shared__ double sm[MT * MS];  // [y][x] = V[i, b0 + y, j, a0 + x]   (same spin only)
    __shared__ double red[17];
    const int nt1 = (nv1 + MT - 1) / MT, nt2 = (nv2 + MT - 1) / MT;
    const int64_t tiles = mp2_tiles(nv1, nv2, SAME);
    const int64_t items = (int64_t)no1 * no2 * tiles;
    const int64_t sv_a = (int64_t)no2 * nv2;          // stride of a in V
    const int64_t sv_i = (int64_t)nv1 * sv_a;         // stride of i in V
    const int64_t st_i = sv_a;                        // stride of i in T
    const int64_t st_a = (int64_t)no1 * sv_a;         // stride of a in T
    double acc = 0.0;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        int64_t r = w;
        const int64_t p = r % tiles; r /= tiles;
        const int j = (int)(r % no2);
        const int i = (int)(r / no2);
        int ta, tb;
        if (SAME) {  // p -> (ta <= tb), rows of the upper triangle of tiles
            int rem = (int)p;
            ta = 0;
            while (rem >= nt1 - ta) { rem -= nt1 - ta; ++ta; }
            tb = ta + rem;
        } else {
            ta = (int)(p / nt2);
            tb = (int)(p - (int64_t)ta * nt2);
        }
        const int a0 = ta * MT, b0 = tb * MT;
        const int64_t base_v = i * sv_i + (int64_t)j * nv2;
        const int64_t base_t = i * st_i + (int64_t)j * nv2;
        const double eij = eo1[i] + eo2[j];
        if (SAME) {
            for (int e = threadIdx.x; e < MT * MT; e += blockDim.x) {
                const int y = e / MT, x = e - y * MT;
                const bool in_a = a0 + y < nv1 && b0 + x < nv2;
                const bool in_m = b0 + y < nv1 && a0 + x < nv2;
                sa[y * MS + x] = in_a ? v[base_v + (a0 + y) * sv_a + (b0 + x)] : 0.0;
                sm[y * MS + x] = in_m ? v[base_v + (b0 + y) * sv_a + (a0 + x)] : 0.0;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < MT * MT; e += blockDim.x) {
                const int y = e / MT, x = e - y * MT;
                if (a0 + y < nv1 && b0 + x < nv2) {  // the tile: (a, b) = (a0 + y, b0 + x)
                    const double g = sa[y * MS + x] - sm[x * MS + y];
                    const double tv = g / ((eij - ev1[a0 + y]) - ev2[b0 + x]);
                    t[base_t + (a0 + y) * st_a + (b0 + x)] = tv;
                    acc += 0.25 * (tv * g);
                }
                if (ta != tb && b0 + y < nv1 && a0 + x < nv2) {  // its mirror: (a, b) = (b0 + y, a0 + x)
                    const double g = sm[y * MS + x] - sa[x * MS + y];
                    const double tv = g / ((eij - ev1[b0 + y]) - ev2[a0 + x]);
                    t[base_t + (b0 + y) * st_a + (a0 + x)] = tv;
                    acc += 0.25 * (tv * g);
                }
            }
            __syncthreads();  // (the next item overwrites the tiles)
        } else {
            for (int e = threadIdx.x; e < MT * MT; e += blockDim.x) {
                const int y = e / MT, x = e - y * MT;
                if (a0 + y < nv1 && b0 + x < nv2) {
                    const double g = v[base_v + (a0 + y) * sv_a + (b0 + x)];
                    const double tv = g / ((eij - ev1[a0 + y]) - ev2[b0 + x]);
                    t[base_t + (a0 + y) * st_a + (b0 + x)] = tv;
                    acc += tv * g;
                }
            }
        }
    }
    const double total = nbx_block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// out[0] = sum of n partials: thread t adds t, t + blockDim.x, ... in that order, then the fixed tree of nbx_block_sum
__global__ __launch_bounds__(256) void mp2_reduce_kernel(int64_t n, const double* __restrict__ partial,
                                                         double* __restrict__ out) {
    __shared__ double red[17];
    double acc = 0.0;
    for (int64_t idx = threadIdx.x; idx < n; idx += blockDim.x) acc += partial[idx];
    const double total = nbx_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = total;
}

inline int64_t mp2_groups(int64_t no1, int64_t nv1, int64_t no2, int64_t nv2, int same) {
    const int64_t items = no1 * no2 * mp2_tiles(nv1, nv2, same);
    return items < MP2_MAX_GROUPS ? items : MP2_MAX_GROUPS;
}

}  // namespace

extern "C" {

size_t nbx_mp2_pairs_worksize(int64_t no1, int64_t nv1, int64_t no2, int64_t nv2, int same_spin) {
    if (no1 <= 0 || nv1 <= 0 || no2 <= 0 || nv2 <= 0) return 0;
    return (size_t)mp2_groups(no1, nv1, no2, nv2, same_spin) * sizeof(double);
}

int nbx_mp2_pairs_tile(void) { return MT; }

int nbx_mp2_pairs(nbx_ctx* ctx, int64_t no1, int64_t nv1, int64_t no2, int64_t nv2, const double* d_v, const double* d_eo1,
                  const double* d_ev1, const double* d_eo2, const double* d_ev2, int same_spin, double* d_t, void* d_work,
                  size_t work_bytes, double* d_energy) {
    NBX_CHECK_ARG(ctx && no1 >= 0 && nv1 >= 0 && no2 >= 0 && nv2 >= 0);
    NBX_CHECK_ARG(no1 < 32768 && nv1 < 32768 && no2 < 32768 && nv2 < 32768);
    NBX_CHECK_ARG(!same_spin || (nv1 == nv2 && no1 <= no2));
    NBX_CHECK_ARG(d_energy != nullptr);
    if (no1 == 0 || nv1 == 0 || no2 == 0 || nv2 == 0) {  // an empty block: the sum is empty
        NBX_HIP(hipMemsetAsync(d_energy, 0, sizeof(double), ctx->stream));
        return NBX_OK;
    }
    NBX_CHECK_ARG(d_v && d_eo1 && d_ev1 && d_eo2 && d_ev2 && d_t && d_work && d_t != d_v);
    if (work_bytes < nbx_mp2_pairs_worksize(no1, nv1, no2, nv2, same_spin)) {
        nbx_set_error("nbx_mp2_pairs: workspace of %zu bytes, %zu needed", work_bytes,
                      nbx_mp2_pairs_worksize(no1, nv1, no2, nv2, same_spin));
        return NBX_E_NOMEM;
    }
    const int64_t groups = mp2_groups(no1, nv1, no2, nv2, same_spin);
    double* d_partials = (double*)d_work;  // one slot per workgroup, every one of them written
    if (same_spin) {
        hipLaunchKernelGGL(mp2_pairs_kernel<true>, dim3((unsigned)groups), dim3(256), 0, ctx->stream, (int)no1, (int)nv1,
                           (int)no2, (int)nv2, d_v, d_eo1, d_ev1, d_eo2, d_ev2, d_t, d_partials);
    } else {
        hipLaunchKernelGGL(mp2_pairs_kernel<false>, dim3((unsigned)groups), dim3(256), 0, ctx->stream, (int)no1, (int)nv1,
                           (int)no2, (int)nv2, d_v, d_eo1, d_ev1, d_eo2, d_ev2, d_t, d_partials);
    }
    NBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(mp2_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream, groups, d_partials, d_energy);
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

}  // extern "C"
