// libnbx: occupied-orbital localisation by Jacobi sweeps (include/nbx.h "Localisation").
//
// Pipek-Mezey and Boys both maximise  f(U) = sum_k sum_i ((U^T Q_k U)_ii)^2  over orthogonal U for a set of
// symmetric n x n matrices Q_k (Pipek & Mezey, J. Chem. Phys. 90, 4916 (1989)).  On a pair (s, t):
//     A = sum_k [ Q_k[s,t]^2 - 1/4 (Q_k[s,s] - Q_k[t,t])^2 ],   B = sum_k Q_k[s,t] (Q_k[s,s] - Q_k[t,t])
//     f(gamma) = const - A cos 4 gamma + B sin 4 gamma   ->   gamma = 1/4 atan2(B, -A),  gain = A + hypot(A, B)
//     s' = cos(gamma) s + sin(gamma) t,   t' = -sin(gamma) s + cos(gamma) t.
// Two rounding guards, with P = sum_k (Q_ss^2 + Q_tt^2 + 2 Q_st^2) the scale of the pair's terms:
//   * hypot(A, B) <= LOC_FLAT P: the pair is flat in gamma (a degenerate maximum, or a zero padding column) and is
//     not rotated -- its angle would be noise;
//   * |sin gamma| hypot(A, B) <= LOC_NOISE P: the rotation is applied, but it is below what the sums resolve and
//     does not count for the stopping rule (a nearly flat pair would otherwise keep the sweeps going for ever).
//
//   * Pipek-Mezey (one-sided): Q_A = 1/2 (X_A^T Y_A + Y_A^T X_A) over the AO rows of atom A.  The working set is the
//     columns of X (and of Y when it differs) stored as contiguous rows, as svd_lds_kernel stores them; a pair's
//     three per-atom sums are taken by its 16-lane group (one lane per atom, or -- fewer than 16 atoms -- all 16 lanes
//     per atom), then the two rows are rotated in place.
//   * Boys (two-sided): the three dipole matrices, n x n each; rows s, t of every pair in one phase, columns s, t in a
//     second, as the Jacobi eigensolver rotates its one matrix.
// U^T is accumulated in place (rows s, t rotated with the working set).  All sweeps run inside one launch, pairs
// from the tournament ring of jacobi_ring.h; a sweep whose largest counted |sin gamma| is below tol ends the solve.
// One workgroup per problem (alpha and beta in one launch), no workgroup waits on another.  The working set lives in
// LDS while it fits (LOC_LDS_MAX), else in a global workspace with the same code.  Every sum has a fixed order:
// repeated calls and identical problems give identical bits.
#include <cmath>
#include <vector>

#include "jacobi_ring.h"
#include "nbx_common.h"

namespace {

constexpr int LOC_THREADS = 1024;
constexpr int LOC_GROUPS = LOC_THREADS / 16;  // a 16-lane group owns a pair
constexpr size_t LOC_LDS_MAX = 150 * 1024;    // working-set bytes kept in LDS
constexpr int LOC_LDS_ATTR = 160 * 1024;
constexpr int64_t LOC_MAX_N = 4096;
constexpr double LOC_FLAT = 1.0e-13;
constexpr double LOC_NOISE = 1.0e-13;

__device__ __forceinline__ double group16_sum(double v) {
    v += nbx_dpp_f64<NBX_DPP_XOR1>(v);
    v += nbx_dpp_f64<NBX_DPP_XOR2>(v);
    v += nbx_dpp_f64<NBX_DPP_HALF_MIRROR>(v);
    v += nbx_dpp_f64<NBX_DPP_MIRROR>(v);
    return v;
}

// max over the block (all threads get it); red: >= 17 doubles
__device__ __forceinline__ double loc_block_max(double v, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t = fmax(t, red[w]);
        red[16] = t;
    }
    __syncthreads();
    return red[16];
}

// Q_A[s,s], Q_A[t,t], Q_A[s,t] of every atom folded into (A, B, P) of the pair; every lane of the group gets them
__device__ __forceinline__ void pm_pair_terms(const double* xs, const double* xt, const double* ys, const double* yt,
                                              const int* __restrict__ off, int natm, int gl, double& A, double& B,
                                              double& P) {
    double a = 0.0, b = 0.0, p = 0.0;
    auto fold = [&](double ss, double tt, double st) {
        const double d = ss - tt;
        a += fma(st, st, -0.25 * d * d);
        b = fma(st, d, b);
        p += fma(ss, ss, fma(tt, tt, 2.0 * st * st));
    };
    if (natm >= 16) {  // one lane per atom
        for (int at = gl; at < natm; at += 16) {
            const int i0 = off[at], i1 = off[at + 1];
            double ss = 0.0, tt = 0.0, st = 0.0;
            for (int i = i0; i < i1; ++i) {
                const double x1 = xs[i], x2 = xt[i], y1 = ys[i], y2 = yt[i];
                ss = fma(x1, y1, ss);
                tt = fma(x2, y2, tt);
                st = fma(x1, y2, fma(y1, x2, st));
            }
            fold(ss, tt, 0.5 * st);
        }
    } else {  // all 16 lanes on each atom
        for (int at = 0; at < natm; ++at) {
            const int i0 = off[at], i1 = off[at + 1];
            double ss = 0.0, tt = 0.0, st = 0.0;
            for (int i = i0 + gl; i < i1; i += 16) {
                const double x1 = xs[i], x2 = xt[i], y1 = ys[i], y2 = yt[i];
                ss = fma(x1, y1, ss);
                tt = fma(x2, y2, tt);
                st = fma(x1, y2, fma(y1, x2, st));
            }
            ss = group16_sum(ss);
            tt = group16_sum(tt);
            st = 0.5 * group16_sum(st);
            if (gl == 0) fold(ss, tt, st);
        }
    }
    A = group16_sum(a);
    B = group16_sum(b);
    P = group16_sum(p);
}

// sum_A Q_A[i,i]^2 of one orbital (valid in every lane of the group)
__device__ __forceinline__ double pm_diag_f(const double* xi, const double* yi, const int* __restrict__ off, int natm,
                                            int gl) {
    double f = 0.0;
    if (natm >= 16) {
        for (int at = gl; at < natm; at += 16) {
            double q = 0.0;
            for (int i = off[at]; i < off[at + 1]; ++i) q = fma(xi[i], yi[i], q);
            f = fma(q, q, f);
        }
    } else {
        for (int at = 0; at < natm; ++at) {
            double q = 0.0;
            for (int i = off[at] + gl; i < off[at + 1]; i += 16) q = fma(xi[i], yi[i], q);
            q = group16_sum(q);
            if (gl == 0) f = fma(q, q, f);
        }
    }
    return group16_sum(f);
}

// (c, s) of the pair from its (A, B, P), s == 0: no rotation; returns the |sin gamma| the stopping rule counts
__device__ __forceinline__ double pair_angle(double A, double B, double P, double& c, double& sn) {
    c = 1.0;
    sn = 0.0;
    const double amp = hypot(A, B);
    if (!(amp > LOC_FLAT * P)) return 0.0;
    sincos(0.25 * atan2(B, -A), &sn, &c);
    return fabs(sn) * amp > LOC_NOISE * P ? fabs(sn) : 0.0;
}

__device__ __forceinline__ void rotate_rows(double* rs, double* rt, int len, int gl, double c, double sn) {
    for (int i = gl; i < len; i += 16) {
        const double x1 = rs[i], x2 = rt[i];
        rs[i] = fma(c, x1, sn * x2);
        rt[i] = fma(c, x2, -sn * x1);
    }
}

// Small per-workgroup LDS behind the working set: the pair angles of a step (Boys), per-orbital f terms, reductions.
struct LocSmall {
    double2* cs;  // [NP/2]
    double* fi;   // [NP]
    double* red;  // [17]
};
__device__ __forceinline__ LocSmall loc_small(double* p, int NP) {
    LocSmall s;
    s.cs = reinterpret_cast<double2*>(p);
    s.fi = p + NP;  // NP/2 double2 = NP doubles
    s.red = s.fi + NP;
    return s;
}
inline int64_t loc_small_doubles(int64_t np) { return 2 * np + 17; }

// stat[2b] = sweeps, stat[2b + 1] = 1 if the sweep limit ended the solve (all zero: converged without a sweep)
template <bool LDS>
__global__ __launch_bounds__(LOC_THREADS) void loc_pm_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                              int M, int N, int NP, int steps, int natm,
                                                              const int* __restrict__ off, double* __restrict__ u_out,
                                                              int max_sweeps, double tol, double* __restrict__ gwork,
                                                              int64_t ws_doubles, int* __restrict__ stat,
                                                              double* __restrict__ f_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = blockIdx.x, tid = threadIdx.x, grp = tid >> 4, gl = tid & 15;
    const int mp = NP / 2, R = NP - 1;
    const bool same = (y == nullptr);
    const int64_t xy_elems = (int64_t)NP * M;
    double* W = LDS ? smem : gwork + (int64_t)b * ws_doubles;
    double* Xt = W;                            // [NP][M]: column j of X is row j
    double* Yt = same ? Xt : Xt + xy_elems;    // [NP][M]
    double* Ut = (same ? Xt : Yt) + xy_elems;  // [NP][NP]: column j of U is row j
    const LocSmall sm = loc_small(LDS ? Ut + (int64_t)NP * NP : smem, NP);

    x += (int64_t)b * M * N;
    if (!same) y += (int64_t)b * M * N;
    for (int64_t idx = tid; idx < xy_elems; idx += LOC_THREADS) {
        const int i = (int)(idx / NP), j = (int)(idx - (int64_t)i * NP);  // consecutive threads: a row of X
        Xt[(int64_t)j * M + i] = (j < N) ? x[(int64_t)i * N + j] : 0.0;
        if (!same) Yt[(int64_t)j * M + i] = (j < N) ? y[(int64_t)i * N + j] : 0.0;
    }
    for (int64_t idx = tid; idx < (int64_t)NP * NP; idx += LOC_THREADS) {
        const int r = (int)(idx / NP), c = (int)(idx - (int64_t)r * NP);
        Ut[idx] = (r == c) ? 1.0 : 0.0;
    }
    __syncthreads();

    auto index_at = [&](int pos, int t) {  // original index at ring position `pos` after t turns
        if (pos < 0) return 0;
        int q = pos - t;
        if (q < 0) q += R;
        return ring_index0(q, mp);
    };

    int sweep = 0;
    bool converged = N < 2;
    for (; sweep < max_sweeps && !converged; ++sweep) {
        double smax = 0.0;
        for (int step = 0; step < steps; ++step) {
            for (int k = grp; k < mp; k += LOC_GROUPS) {
                const int s = index_at(k == 0 ? -1 : ring_pos_top(k), step);
                const int t = index_at(ring_pos_bot(k, mp), step);
                double* xs = Xt + (int64_t)s * M;
                double* xt = Xt + (int64_t)t * M;
                double* ys = Yt + (int64_t)s * M;
                double* yt = Yt + (int64_t)t * M;
                double A, B, P, c, sn;
                pm_pair_terms(xs, xt, ys, yt, off, natm, gl, A, B, P);
                smax = fmax(smax, pair_angle(A, B, P, c, sn));
                if (sn != 0.0) {  // uniform over the group
                    rotate_rows(xs, xt, M, gl, c, sn);
                    if (!same) rotate_rows(ys, yt, M, gl, c, sn);
                    rotate_rows(Ut + (int64_t)s * NP, Ut + (int64_t)t * NP, NP, gl, c, sn);
                }
            }
            __syncthreads();
        }
        converged = loc_block_max(smax, sm.red) < tol;
    }

    for (int i = grp; i < NP; i += LOC_GROUPS) {
        const double fi = pm_diag_f(Xt + (int64_t)i * M, Yt + (int64_t)i * M, off, natm, gl);
        if (gl == 0) sm.fi[i] = (i < N) ? fi : 0.0;
    }
    u_out += (int64_t)b * N * N;
    for (int64_t idx = tid; idx < (int64_t)N * N; idx += LOC_THREADS) {
        const int i = (int)(idx / N), j = (int)(idx - (int64_t)i * N);
        u_out[idx] = Ut[(int64_t)j * NP + i];
    }
    __syncthreads();
    if (tid == 0) {
        double f = 0.0;
        for (int i = 0; i < N; ++i) f += sm.fi[i];
        f_out[b] = f;
        stat[2 * b] = sweep;
        stat[2 * b + 1] = converged ? 0 : 1;
    }
}

template <bool LDS>
__global__ __launch_bounds__(LOC_THREADS) void loc_boys_kernel(const double* __restrict__ q, int N, int NP, int steps,
                                                                double* __restrict__ u_out, int max_sweeps, double tol,
                                                                double* __restrict__ gwork, int64_t ws_doubles,
                                                                int* __restrict__ stat, double* __restrict__ f_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = blockIdx.x, tid = threadIdx.x, grp = tid >> 4, gl = tid & 15;
    const int mp = NP / 2, R = NP - 1;
    const int64_t nn = (int64_t)NP * NP;
    double* W = LDS ? smem : gwork + (int64_t)b * ws_doubles;
    double* Q = W;            // [3][NP][NP]
    double* Ut = W + 3 * nn;  // [NP][NP]: column j of U is row j
    const LocSmall sm = loc_small(LDS ? Ut + nn : smem, NP);

    q += (int64_t)b * 3 * N * N;
    for (int64_t idx = tid; idx < 3 * nn; idx += LOC_THREADS) {
        const int d = (int)(idx / nn);
        const int64_t rem = idx - (int64_t)d * nn;
        const int i = (int)(rem / NP), j = (int)(rem - (int64_t)i * NP);
        Q[idx] = (i < N && j < N) ? q[((int64_t)d * N + i) * N + j] : 0.0;
    }
    for (int64_t idx = tid; idx < nn; idx += LOC_THREADS) {
        const int r = (int)(idx / NP), c = (int)(idx - (int64_t)r * NP);
        Ut[idx] = (r == c) ? 1.0 : 0.0;
    }
    __syncthreads();

    auto index_at = [&](int pos, int t) {
        if (pos < 0) return 0;
        int qq = pos - t;
        if (qq < 0) qq += R;
        return ring_index0(qq, mp);
    };

    int sweep = 0;
    bool converged = N < 2;
    for (; sweep < max_sweeps && !converged; ++sweep) {
        double smax = 0.0;
        for (int step = 0; step < steps; ++step) {
            // the angle of each pair from the diagonals and [s,t]; rows s, t of the three matrices and of U^T
            for (int k = grp; k < mp; k += LOC_GROUPS) {
                const int s = index_at(k == 0 ? -1 : ring_pos_top(k), step);
                const int t = index_at(ring_pos_bot(k, mp), step);
                double A = 0.0, B = 0.0, P = 0.0;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double* Qd = Q + d * nn;
                    const double ss = Qd[(int64_t)s * NP + s], tt = Qd[(int64_t)t * NP + t];
                    const double st = Qd[(int64_t)s * NP + t];
                    const double df = ss - tt;
                    A += fma(st, st, -0.25 * df * df);
                    B = fma(st, df, B);
                    P += fma(ss, ss, fma(tt, tt, 2.0 * st * st));
                }
                double c, sn;
                smax = fmax(smax, pair_angle(A, B, P, c, sn));
                if (gl == 0) sm.cs[k] = make_double2(c, sn);
                if (sn != 0.0) {
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        rotate_rows(Q + d * nn + (int64_t)s * NP, Q + d * nn + (int64_t)t * NP, NP, gl, c, sn);
                    rotate_rows(Ut + (int64_t)s * NP, Ut + (int64_t)t * NP, NP, gl, c, sn);
                }
            }
            __syncthreads();
            // columns s, t of the three matrices
            for (int k = grp; k < mp; k += LOC_GROUPS) {
                const double2 r = sm.cs[k];
                if (r.y == 0.0) continue;
                const int s = index_at(k == 0 ? -1 : ring_pos_top(k), step);
                const int t = index_at(ring_pos_bot(k, mp), step);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double* Qd = Q + d * nn;
                    for (int i = gl; i < NP; i += 16) {
                        const double x1 = Qd[(int64_t)i * NP + s], x2 = Qd[(int64_t)i * NP + t];
                        Qd[(int64_t)i * NP + s] = fma(r.x, x1, r.y * x2);
                        Qd[(int64_t)i * NP + t] = fma(r.x, x2, -r.y * x1);
                    }
                }
            }
            __syncthreads();
        }
        converged = loc_block_max(smax, sm.red) < tol;
    }

    for (int i = tid; i < NP; i += LOC_THREADS) {
        double fi = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double v = Q[d * nn + (int64_t)i * NP + i];
            fi = fma(v, v, fi);
        }
        sm.fi[i] = (i < N) ? fi : 0.0;
    }
    u_out += (int64_t)b * N * N;
    for (int64_t idx = tid; idx < (int64_t)N * N; idx += LOC_THREADS) {
        const int i = (int)(idx / N), j = (int)(idx - (int64_t)i * N);
        u_out[idx] = Ut[(int64_t)j * NP + i];
    }
    __syncthreads();
    if (tid == 0) {
        double f = 0.0;
        for (int i = 0; i < N; ++i) f += sm.fi[i];
        f_out[b] = f;
        stat[2 * b] = sweep;
        stat[2 * b + 1] = converged ? 0 : 1;
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// working-set doubles of one problem
int64_t loc_ws_doubles(int kind, int64_t nao, int64_t n, bool same) {
    const int64_t np = (n + 1) & ~1ll;
    if (kind == NBX_LOC_BOYS) return 4 * np * np;
    return (same ? 1 : 2) * np * nao + np * np;
}

bool loc_fits_lds(int kind, int64_t nao, int64_t n, bool same) {
    const int64_t np = (n + 1) & ~1ll;
    return (size_t)(loc_ws_doubles(kind, nao, n, same) + loc_small_doubles(np)) * sizeof(double) <= LOC_LDS_MAX;
}

// workspace: [sweeps, limit-hit flag per problem | f per problem | atom offsets | global working sets]
struct LocLayout {
    size_t f_off, atm_off, ws_off, total;
    int64_t ws_stride;  // doubles between two problems' working sets (0: in LDS)
};

LocLayout loc_layout(int kind, int64_t batch, int64_t nao, int64_t n, int64_t natm) {
    LocLayout L;
    L.f_off = align256((size_t)(2 * batch) * sizeof(int));
    L.atm_off = L.f_off + align256((size_t)batch * sizeof(double));
    L.ws_off = L.atm_off + (kind == NBX_LOC_PM ? align256((size_t)(natm + 1) * sizeof(int)) : 0);
    // sized for Y != X, the larger case: whatever does not fit LDS then has its slot here
    L.ws_stride = loc_fits_lds(kind, nao, n, false)
                      ? 0
                      : (int64_t)(align256((size_t)loc_ws_doubles(kind, nao, n, false) * sizeof(double)) / sizeof(double));
    L.total = L.ws_off + (size_t)(L.ws_stride * batch) * sizeof(double);
    return L;
}

template <class K>
int set_lds_attr(K kernel, bool& done) {
    if (!done) {
        NBX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    LOC_LDS_ATTR));
        done = true;
    }
    return NBX_OK;
}

int loc_check_work(const char* who, int kind, int batch, int64_t nao, int64_t n, int64_t natm, const void* d_work,
                   size_t work_bytes) {
    const size_t need = loc_layout(kind, batch, nao, n, natm).total;
    if (d_work == nullptr || work_bytes < need) {
        nbx_set_error("%s: workspace %zu < %zu bytes", who, work_bytes, need);
        return NBX_E_INVALID;
    }
    return NBX_OK;
}

}  // namespace

extern "C" size_t nbx_loc_worksize(int kind, int batch, int64_t nao, int64_t n, int64_t natm) {
    if ((kind != NBX_LOC_PM && kind != NBX_LOC_BOYS) || batch < 0 || nao < 0 || n < 0 || natm < 0) return 0;
    return loc_layout(kind, batch, nao, n, natm).total;
}

extern "C" int nbx_loc_pm(nbx_ctx* ctx, int batch, int64_t nao, int64_t n, int64_t natm, const int64_t* h_ao_offsets,
                          const double* d_x, const double* d_y, double* d_u, int max_sweeps, double tol, void* d_work,
                          size_t work_bytes) {
    NBX_CHECK_ARG(ctx && batch >= 0 && nao >= 0 && n >= 0 && natm >= 0 && max_sweeps >= 0 && tol >= 0.0);
    NBX_CHECK_ARG(n <= LOC_MAX_N && nao <= (1 << 20) && natm <= nao + 1);
    int rc = loc_check_work("nbx_loc_pm", NBX_LOC_PM, batch, nao, n, natm, d_work, work_bytes);
    if (rc != NBX_OK) return rc;
    const LocLayout L = loc_layout(NBX_LOC_PM, batch, nao, n, natm);
    if (batch == 0) return NBX_OK;
    if (n == 0) return nbx_memset(ctx, d_work, 0, L.atm_off);
    NBX_CHECK_ARG(d_x && d_u && h_ao_offsets && natm >= 1 && nao >= 1);
    if (h_ao_offsets[0] != 0 || h_ao_offsets[natm] != nao) {
        nbx_set_error("nbx_loc_pm: the atom AO offsets must run from 0 to nao = %lld", (long long)nao);
        return NBX_E_INVALID;
    }
    std::vector<int> off((size_t)natm + 1);
    for (int64_t a = 0; a <= natm; ++a) {
        if (a > 0 && h_ao_offsets[a] < h_ao_offsets[a - 1]) {
            nbx_set_error("nbx_loc_pm: the atom AO offsets descend at atom %lld", (long long)a);
            return NBX_E_INVALID;
        }
        off[(size_t)a] = (int)h_ao_offsets[a];
    }
    char* base = static_cast<char*>(d_work);
    int* d_off = reinterpret_cast<int*>(base + L.atm_off);
    rc = nbx_memcpy_h2d(ctx, d_off, off.data(), off.size() * sizeof(int));
    if (rc != NBX_OK) return rc;
    const int64_t np = (n + 1) & ~1ll;
    const int steps = np == 2 ? 1 : (int)(np - 1);
    const bool same = (d_y == nullptr);
    int* stat = reinterpret_cast<int*>(base);
    double* f = reinterpret_cast<double*>(base + L.f_off);
    nbx_prof_scope prof(ctx, NBX_PROF_LOC);
    if (loc_fits_lds(NBX_LOC_PM, nao, n, same)) {
        static bool attr = false;
        rc = set_lds_attr(loc_pm_kernel<true>, attr);
        if (rc != NBX_OK) return rc;
        const size_t lds = (size_t)(loc_ws_doubles(NBX_LOC_PM, nao, n, same) + loc_small_doubles(np)) * sizeof(double);
        hipLaunchKernelGGL(loc_pm_kernel<true>, dim3((unsigned)batch), dim3(LOC_THREADS), lds, ctx->stream, d_x, d_y,
                           (int)nao, (int)n, (int)np, steps, (int)natm, d_off, d_u, max_sweeps, tol, (double*)nullptr,
                           (int64_t)0, stat, f);
    } else {  // (then Y != X does not fit either: L.ws_stride > 0)
        static bool attr = false;
        rc = set_lds_attr(loc_pm_kernel<false>, attr);
        if (rc != NBX_OK) return rc;
        const size_t lds = (size_t)loc_small_doubles(np) * sizeof(double);
        hipLaunchKernelGGL(loc_pm_kernel<false>, dim3((unsigned)batch), dim3(LOC_THREADS), lds, ctx->stream, d_x, d_y,
                           (int)nao, (int)n, (int)np, steps, (int)natm, d_off, d_u, max_sweeps, tol,
                           reinterpret_cast<double*>(base + L.ws_off), L.ws_stride, stat, f);
    }
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

extern "C" int nbx_loc_boys(nbx_ctx* ctx, int batch, int64_t n, const double* d_q, double* d_u, int max_sweeps,
                            double tol, void* d_work, size_t work_bytes) {
    NBX_CHECK_ARG(ctx && batch >= 0 && n >= 0 && max_sweeps >= 0 && tol >= 0.0 && n <= LOC_MAX_N);
    int rc = loc_check_work("nbx_loc_boys", NBX_LOC_BOYS, batch, 0, n, 0, d_work, work_bytes);
    if (rc != NBX_OK) return rc;
    const LocLayout L = loc_layout(NBX_LOC_BOYS, batch, 0, n, 0);
    if (batch == 0) return NBX_OK;
    if (n == 0) return nbx_memset(ctx, d_work, 0, L.atm_off);
    NBX_CHECK_ARG(d_q && d_u);
    char* base = static_cast<char*>(d_work);
    const int64_t np = (n + 1) & ~1ll;
    const int steps = np == 2 ? 1 : (int)(np - 1);
    int* stat = reinterpret_cast<int*>(base);
    double* f = reinterpret_cast<double*>(base + L.f_off);
    nbx_prof_scope prof(ctx, NBX_PROF_LOC);
    if (L.ws_stride == 0) {
        static bool attr = false;
        rc = set_lds_attr(loc_boys_kernel<true>, attr);
        if (rc != NBX_OK) return rc;
        const size_t lds = (size_t)(loc_ws_doubles(NBX_LOC_BOYS, 0, n, true) + loc_small_doubles(np)) * sizeof(double);
        hipLaunchKernelGGL(loc_boys_kernel<true>, dim3((unsigned)batch), dim3(LOC_THREADS), lds, ctx->stream, d_q,
                           (int)n, (int)np, steps, d_u, max_sweeps, tol, (double*)nullptr, (int64_t)0, stat, f);
    } else {
        static bool attr = false;
        rc = set_lds_attr(loc_boys_kernel<false>, attr);
        if (rc != NBX_OK) return rc;
        const size_t lds = (size_t)loc_small_doubles(np) * sizeof(double);
        hipLaunchKernelGGL(loc_boys_kernel<false>, dim3((unsigned)batch), dim3(LOC_THREADS), lds, ctx->stream, d_q,
                           (int)n, (int)np, steps, d_u, max_sweeps, tol, reinterpret_cast<double*>(base + L.ws_off),
                           L.ws_stride, stat, f);
    }
    NBX_LAUNCH_CHECK();
    return NBX_OK;
}

extern "C" int nbx_loc_status(nbx_ctx* ctx, int batch, const void* d_work, int* h_sweeps, double* h_f) {
    NBX_CHECK_ARG(ctx && d_work && batch >= 0);
    if (batch == 0) return NBX_OK;
    std::vector<int> st((size_t)(2 * batch));
    std::vector<double> f((size_t)batch);
    int rc = nbx_memcpy_d2h(ctx, st.data(), d_work, st.size() * sizeof(int));
    if (rc != NBX_OK) return rc;
    rc = nbx_memcpy_d2h(ctx, f.data(), static_cast<const char*>(d_work) + align256((size_t)(2 * batch) * sizeof(int)),
                        f.size() * sizeof(double));
    if (rc != NBX_OK) return rc;
    int bad = -1;
    for (int b = 0; b < batch; ++b) {
        if (h_sweeps) h_sweeps[b] = st[(size_t)(2 * b)];
        if (h_f) h_f[b] = f[(size_t)b];
        if (st[(size_t)(2 * b + 1)] != 0 && bad < 0) bad = b;
    }
    if (bad >= 0) {
        nbx_set_error("nbx_loc: problem %d did not converge in %d sweeps", bad, st[(size_t)(2 * bad)]);
        return NBX_E_NOCONV;
    }
    return NBX_OK;
}
