// Potential of an MM environment in the AO basis, on the device.
//
//   V[mu nu] = - sum_c q_c (mu nu | erf(sqrt(zeta_c) r_C) / r_C)
//
// what qmmm.mm_charge adds to get_hcore() (nbed/driver.py:171-180, 246-253), for 10^3 .. 10^5 charges: the one
// one-electron term whose cost grows with the environment.  The pair data (Hermite densities, p, P, Boys table) is
// nbx_eri::Session's, the scheme nbx_host_mm_potential's (ints_host.cpp):
//
//   mm_pair_kernel<L>   one wavefront owns a shell pair of order L = la + lb and a chunk of MM_CHUNK charges.  Per
//                       primitive pair every lane evaluates F_0 .. F_L and the recursion to R_tuv for its charges in
//                       registers (every index a compile-time constant) and sums
//                       A_tuv = - sum_c q_c (1 + p / zeta_c)^(-1/2) R_tuv(rho_c, P - C_c); a butterfly over the lanes adds
//                       the 64 partial A; lane ab < nab contracts (2 pi / p) H[ab][.] A.  Cartesian -> spherical through
//                       LDS, and the block goes to the chunk's slice of a partials buffer.
//   mm_sum_kernel       V[r][c] = V[c][r] = sum over the chunks, in chunk order, of the partial of (r >= c).
//
// No atomics; lanes, butterfly and chunks add in an order that depends on (shells, number of charges) alone, so two
// calls give the same bits.  Every element of V is written: a shell pair whose primitives are all screened out still
// has its workgroups, which write zeros.
#include "eri_device.h"

#include <type_traits>

namespace {

using namespace nbx_md;
using namespace nbx_eri;

constexpr int MM_LMAX = 2;              // per shell, as the session
constexpr int MM_NLP = 2 * MM_LMAX + 1;  // pair orders 0 .. 4
constexpr int MM_BLOCK = 64;            // one wavefront per workgroup
constexpr int MM_CHUNK = 512;           // charges of one workgroup: eight per lane
constexpr int MM_NAB_MAX = 36;          // dd

__host__ __device__ constexpr int mm_nherm(int l) { return (l + 1) * (l + 2) * (l + 3) / 6; }
// position of (t, u, v) in HermIndex(l): t, then u, then v ascending -- the order of the Hermite densities
__host__ __device__ constexpr int mm_hidx(int l, int t, int u, int v) {
    int n = 0;
    for (int tt = 0; tt < t; ++tt) n += (l - tt + 1) * (l - tt + 2) / 2;
    for (int uu = 0; uu < u; ++uu) n += l - t - uu + 1;
    return n + v;
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

struct MmArgs {
    const double* cx;  // five planes of ncharge doubles: x, y, z, q, 1 / zeta (0: a point charge)
    const double* cy;
    const double* cz;
    const double* cq;
    const double* ciz;
    const int* pairs;  // the shell pairs of this launch's order
    double* part;      // (nchunk, nao, nao)
    int ncharge, nchunk;
};

// pot[k] += - q (1 + p / zeta)^(-1/2) R_tuv(rho, P - C), k = mm_hidx(L, t, u, v): hermite_r of ints_md.h with both cubes
// in registers
template <int L>
__device__ __forceinline__ void mm_add_charge(const double* __restrict__ boys, double p, double x, double y, double z,
                                              double q, double iz, double (&pot)[mm_nherm(L)]) {
    constexpr int E = L + 1;
    const double s = 1.0 + p * iz, rho = p / s, w = -q / sqrt(s);
    double f[L + 1], pw[L + 1], cube[2][E * E * E];
    boys_eval<L>(boys, rho * (x * x + y * y + z * z), f);
    pw[0] = 1.0;
#pragma unroll
    for (int n = 1; n <= L; ++n) pw[n] = pw[n - 1] * (-2.0 * rho);
    static_for<0, L + 1>([&](auto top_) {
        constexpr int top = decltype(top_)::value, n = L - top, c = top & 1, o = c ^ 1;
        static_for<0, top + 1>([&](auto t_) {
            constexpr int t = decltype(t_)::value;
            static_for<0, top - t + 1>([&](auto u_) {
                constexpr int u = decltype(u_)::value;
                static_for<0, top - t - u + 1>([&](auto v_) {
                    constexpr int v = decltype(v_)::value;
                    double val;
                    if constexpr (t + u + v == 0) {
                        val = pw[n] * f[n];
                    } else if constexpr (t > 0) {
                        val = x * cube[o][((t - 1) * E + u) * E + v];
                        if constexpr (t > 1) val += (t - 1) * cube[o][((t - 2) * E + u) * E + v];
                    } else if constexpr (u > 0) {
                        val = y * cube[o][(t * E + u - 1) * E + v];
                        if constexpr (u > 1) val += (u - 1) * cube[o][(t * E + u - 2) * E + v];
                    } else {
                        val = z * cube[o][(t * E + u) * E + v - 1];
                        if constexpr (v > 1) val += (v - 1) * cube[o][(t * E + u) * E + v - 2];
                    }
                    cube[c][(t * E + u) * E + v] = val;
                    if constexpr (top == L) pot[mm_hidx(L, t, u, v)] += w * val;
                });
            });
        });
    });
}

template <int L>
__global__ __launch_bounds__(MM_BLOCK) void mm_pair_kernel(EriArgs a, MmArgs m) {
    constexpr int NH = mm_nherm(L);
    __shared__ double s_buf[2 * MM_NAB_MAX];
    const int lane = threadIdx.x;
    const int chunk = int(blockIdx.x % unsigned(m.nchunk));
    const DevPair pr = a.pairs[m.pairs[blockIdx.x / unsigned(m.nchunk)]];
    const DevShell sa = a.shells[pr.ia], sb = a.shells[pr.ib];
    const int nab = pr.nab;
    const int c0 = chunk * MM_CHUNK, c1 = min(c0 + MM_CHUNK, m.ncharge);

    double acc = 0.0;  // Cartesian component pair `lane` (< nab)
    for (int i = 0; i < pr.nprim; ++i) {
        const double* pp = a.prim + 4 * (pr.prim_off + i);
        const double p = pp[0], px = pp[1], py = pp[2], pz = pp[3];
        double pot[NH];
#pragma unroll
        for (int k = 0; k < NH; ++k) pot[k] = 0.0;
        for (int c = c0 + lane; c < c1; c += MM_BLOCK)
            mm_add_charge<L>(a.boys, p, px - m.cx[c], py - m.cy[c], pz - m.cz[c], m.cq[c], m.ciz[c], pot);
#pragma unroll
        for (int k = 0; k < NH; ++k) pot[k] = nbx_wave_sum(pot[k]);
        if (lane < nab) {
            const double* h = a.h + pr.h_off + (size_t(i) * nab + lane) * NH;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NH; ++k) s += h[k] * pot[k];
            acc += 2.0 * M_PI / p * s;
        }
    }

    // Cartesian (na, nb) -> AOs, axis by axis (block_to_ao of ints_host.cpp), then the block's place in this chunk's slice
    double* src = s_buf;
    double* dst = s_buf + MM_NAB_MAX;
    if (lane < nab) src[lane] = acc;
    __syncthreads();
    int dims[2] = {sa.ncart, sb.ncart};
    const DevShell sh[2] = {sa, sb};
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        if (sh[ax].l < 2) continue;  // identity for s and p
        const int nc = dims[ax], ns = sh[ax].nsph;
        const int outer = ax == 0 ? 1 : dims[0], inner = ax == 0 ? dims[1] : 1;
        const double* sm = a.sph + sh[ax].sph_off;
        for (int idx = lane; idx < outer * ns * inner; idx += MM_BLOCK) {
            const int o = idx / (ns * inner), rem = idx - o * ns * inner, mm = rem / inner, in = rem - mm * inner;
            double s = 0.0;
            for (int c = 0; c < nc; ++c) s += sm[mm * nc + c] * src[(o * nc + c) * inner + in];
            dst[idx] = s;
        }
        dims[ax] = ns;
        __syncthreads();
        double* t = src; src = dst; dst = t;
    }
    const size_t n = size_t(a.nao);
    double* slice = m.part + size_t(chunk) * n * n;
    for (int idx = lane; idx < dims[0] * dims[1]; idx += MM_BLOCK) {
        const int x = idx / dims[1], y = idx - x * dims[1];
        slice[(sa.ao0 + x) * n + sb.ao0 + y] = src[idx];
    }
}

// The element (r >= c) lies in the block of the shell pair (ia >= ib) that holds it; within one shell both (r, c) and
// (c, r) were computed, and as in the host engine the one with r >= c is what both places receive.
__global__ void mm_sum_kernel(const double* __restrict__ part, int nchunk, int nao, double* __restrict__ out) {
    const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long nn = (long long)nao * nao;
    if (idx >= nn) return;
    const int r = int(idx / nao), c = int(idx - (long long)r * nao);
    if (r < c) return;
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += part[k * nn + idx];
    out[idx] = s;
    out[(long long)c * nao + r] = s;
}

template <int L>
void launch_pairs(hipStream_t stream, const EriArgs& a, const MmArgs& m, int64_t npairs) {
    hipLaunchKernelGGL((mm_pair_kernel<L>), dim3((unsigned)(npairs * m.nchunk)), dim3(MM_BLOCK), 0, stream, a, m);
}
using launch_fn = void (*)(hipStream_t, const EriArgs&, const MmArgs&, int64_t);
const launch_fn LAUNCH[MM_NLP] = {launch_pairs<0>, launch_pairs<1>, launch_pairs<2>, launch_pairs<3>, launch_pairs<4>};

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

extern "C" int nbx_mm_potential(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc,
                                const double* centres, const double* exps, const double* coefs, const double* sph,
                                double cutoff, int ncharge, const double* q, const double* xyz, const double* zeta,
                                double* v_device) {
    NBX_CHECK_ARG(ctx != nullptr);
    NBX_CHECK_ARG(v_device != nullptr);
    NBX_CHECK_ARG(ncharge >= 0 && ncharge <= (1 << 30) && (ncharge == 0 || (q != nullptr && xyz != nullptr)));
    for (int c = 0; c < ncharge; ++c)  // (a NaN would index the Boys table out of bounds)
        if (!std::isfinite(q[c]) || !std::isfinite(xyz[3 * c]) || !std::isfinite(xyz[3 * c + 1]) ||
            !std::isfinite(xyz[3 * c + 2]) || (zeta && !(zeta[c] > 0.0))) {
            nbx_set_error("nbx_mm_potential: charge %d is not finite, or its exponent is not positive", c);
            return NBX_E_INVALID;
        }
    Session s;
    int rc = session_open(ctx, nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, s);
    if (rc == NBX_E_INVALID)
        nbx_set_error("%s: invalid shells (angular momentum 0 .. %d, nfunc = 2l+1 or (l+1)(l+2)/2)", "nbx_mm_potential", MM_LMAX);
    if (rc != NBX_OK) return rc;

    const size_t n = size_t(s.eng.nao), npair = s.eng.pairs.size(), nc = size_t(ncharge);
    const int nchunk = int((nc + MM_CHUNK - 1) / MM_CHUNK);
    // one host image: the charges as five planes, then the shell pairs order after order
    const size_t o_list = align256(5 * nc * sizeof(double)), o_part = align256(o_list + npair * sizeof(int));
    const size_t bytes = o_part + std::max<size_t>(size_t(nchunk) * n * n * sizeof(double), 8);
    std::vector<char> img(o_part, 0);
    double* hc = reinterpret_cast<double*>(img.data());
    for (size_t c = 0; c < nc; ++c) {
        hc[c] = xyz[3 * c];
        hc[nc + c] = xyz[3 * c + 1];
        hc[2 * nc + c] = xyz[3 * c + 2];
        hc[3 * nc + c] = q[c];
        hc[4 * nc + c] = zeta ? 1.0 / zeta[c] : 0.0;
    }
    int* hl = reinterpret_cast<int*>(img.data() + o_list);
    int64_t counts[MM_NLP] = {};
    size_t fill = 0;
    for (int l = 0; l < MM_NLP; ++l)
        for (size_t ij = 0; ij < npair; ++ij)
            if (s.eng.pairs[ij].lab == l) {
                hl[fill++] = int(ij);
                ++counts[l];
            }

    char* d_buf = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&d_buf), bytes, s.stream) != hipSuccess) {
        (void)hipGetLastError();
        session_close(s);
        nbx_set_error("nbx_mm_potential: %zu bytes of charges and partial sums do not fit", bytes);
        return NBX_E_NOMEM;
    }
    hipError_t e = hipMemcpyAsync(d_buf, img.data(), o_part, hipMemcpyHostToDevice, s.stream);
    MmArgs m;
    const double* dc = reinterpret_cast<const double*>(d_buf);
    m.cx = dc; m.cy = dc + nc; m.cz = dc + 2 * nc; m.cq = dc + 3 * nc; m.ciz = dc + 4 * nc;
    m.part = reinterpret_cast<double*>(d_buf + o_part);
    m.ncharge = ncharge;
    m.nchunk = nchunk;
    for (int l = 0; l < MM_NLP; ++l)
        if (counts[l] * nchunk > int64_t(INT32_MAX)) {  // one workgroup per (pair, chunk): the grid's x extent
            (void)hipFreeAsync(d_buf, s.stream);
            session_close(s);
            nbx_set_error("nbx_mm_potential: %lld shell pairs x %d chunks of charges exceed one launch", (long long)counts[l], nchunk);
            return NBX_E_UNSUPPORTED;
        }
    int64_t off = 0;
    for (int l = 0; l < MM_NLP && e == hipSuccess; ++l) {
        if (counts[l] == 0 || nchunk == 0) { off += counts[l]; continue; }
        m.pairs = reinterpret_cast<const int*>(d_buf + o_list) + off;
        LAUNCH[l](s.stream, s.args, m, counts[l]);
        e = hipGetLastError();
        off += counts[l];
    }
    if (e == hipSuccess) {
        const long long nn = (long long)(n * n);
        hipLaunchKernelGGL(mm_sum_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s.stream, m.part, nchunk, int(n), v_device);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        nbx_set_error("nbx_mm_potential: upload / launches -> %s", hipGetErrorString(e));
        rc = NBX_E_HIP;
    }
    (void)hipFreeAsync(d_buf, s.stream);
    session_close(s);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == NBX_OK) rc = NBX_E_HIP;  // the image dies with this call
    return rc;
}
