// Two-electron AO integrals of a real molecule, on the device.
//
// The same McMurchie-Davidson scheme as the host engine (ints_host.cpp; both include ints_md.h), for shells of
// angular momentum <= 2, with the dense (nao)^4 tensor written straight into device memory:
//
//   host    shell checks, pair data (Hermite densities, p, P, Schwarz bounds) and the Boys table by the host
//           engine's own code; the canonical quartets (kl <= ij) that pass its Schwarz test, sorted into the 25
//           classes (l_ab, l_cd) = (la + lb, lc + ld); one upload of the pair data, one of the lists
//   device  one launch per non-empty class with the Hermite orders as template parameters.  A wavefront owns a
//           quartet: per primitive pair (i, j) every lane evaluates F_0 .. F_L, the lanes share the downward
//           recursion of R_tuv (two cubes in LDS), then the ket contraction w[c][k_ab] and the bra contraction
//           into per-lane accumulators; Cartesian -> spherical through LDS, and ONE lane stores a value to its
//           eight images.  No atomics: a quartet's sums run in the host engine's order, so two runs are
//           bit-identical, and where shells coincide the lane that stores is the one whose value the host engine's
//           last write leaves, so the images are the same double.
//
// The last stage is one of three sinks chosen at compile time: the dense tensor above; the
// diagonal d[p][q] = (pq|pq) from the quartets (ij, ij); and the columns (pq|rs) of selected shell pairs, which
// csrc/eri_cd.hip decomposes.  All three store by the same rule, so an integral is the same double in each.
#include "eri_device.h"

#include <algorithm>
#include <mutex>

namespace {

using namespace nbx_md;
using namespace nbx_eri;

constexpr int DEV_LMAX = 2;              // per shell on the device (f shells stay on the host engine)
constexpr int NLP = 2 * DEV_LMAX + 1;    // pair orders l_ab = 0 .. 4
constexpr int NCLASS = NLP * NLP;        // 25
constexpr int NH_MAX = 35;               // nherm(4)
constexpr int NR_MAX = 165;              // nherm(8)
constexpr int ERI_BLOCK = 64;            // one wavefront per workgroup: the workgroup barrier is a wave barrier
constexpr int ERI_CUS = 256;             // MI355X
constexpr int ERI_LDS_PER_CU = 160 * 1024;
constexpr int ERI_MAX_WG_PER_CU = 16;

__host__ __device__ constexpr int nherm_c(int l) { return (l + 1) * (l + 2) * (l + 3) / 6; }
// most Cartesian component pairs of a shell pair of order lab with l <= 2 per shell: ss, ps, pp|ds, dp, dd
__host__ __device__ constexpr int nab_max(int lab) { return lab == 0 ? 1 : lab == 1 ? 3 : lab == 2 ? 9 : lab == 3 ? 18 : 36; }
__host__ __device__ constexpr int cube_edge(int lab, int lcd) { return lab + lcd + 1; }
__host__ __device__ constexpr int cube_doubles(int lab, int lcd) { return cube_edge(lab, lcd) * cube_edge(lab, lcd) * cube_edge(lab, lcd); }
__host__ __device__ constexpr int blk_doubles(int lab, int lcd) { return nab_max(lab) * nab_max(lcd); }
// LDS of one wavefront: two R cubes + w[c][k_ab] while the primitives run, then the two buffers of the spherical
// transform in the same bytes; the sign and index tables behind them
__host__ __device__ constexpr int work_doubles(int lab, int lcd) {
    const int loop = 2 * cube_doubles(lab, lcd) + nab_max(lcd) * nherm_c(lab), tail = 2 * blk_doubles(lab, lcd);
    return loop > tail ? loop : tail;
}
// the static LDS of a class's kernel: what nbx_eri_plan reports is the size of the object the kernel declares
template <int LAB, int LCD>
struct EriLds {
    double buf[work_doubles(LAB, LCD)];
    double sgn[nherm_c(LCD)];                                        // (-1)^(tau + nu + phi) of the ket's Hermite index
    int offa[nherm_c(LAB)], offc[nherm_c(LCD)], rl[nherm_c(LAB + LCD)];  // cube offsets; packed (t, u, v) by order
};
#define ERI_ROW(A) sizeof(EriLds<A, 0>), sizeof(EriLds<A, 1>), sizeof(EriLds<A, 2>), sizeof(EriLds<A, 3>), sizeof(EriLds<A, 4>)
constexpr size_t LDS_BYTES[NCLASS] = {ERI_ROW(0), ERI_ROW(1), ERI_ROW(2), ERI_ROW(3), ERI_ROW(4)};
#undef ERI_ROW
inline int lds_bytes_of(int lab, int lcd) { return int(LDS_BYTES[lab * NLP + lcd]); }
inline int wg_per_cu(int lab, int lcd) { return std::min(ERI_MAX_WG_PER_CU, ERI_LDS_PER_CU / lds_bytes_of(lab, lcd)); }
inline int64_t grid_of(int lab, int lcd, int64_t count) { return std::min<int64_t>(count, int64_t(ERI_CUS) * wg_per_cu(lab, lcd)); }

// The sinks of eri_class_kernel: where the spherical block of a quartet goes.
constexpr int SINK_DENSE = 0;   // eight images into the (nao)^4 tensor
constexpr int SINK_DIAG = 1;    // quartets (ij, ij): d[p][q] = d[q][p] = (pq|pq)
constexpr int SINK_COLUMN = 2;  // col[m][p][q] = col[m][q][p] = (pq|m), m a function pair (r >= s) of a selected shell pair

// column of the function pair (x, y) of a selected shell pair whose first column is m0: (r, s) row-major, r >= s
__device__ __forceinline__ size_t column_of(unsigned m0, bool same, int x, int y, int ny) {
    if (!same) return size_t(m0) + x * ny + y;
    const int hi = x > y ? x : y, lo = x > y ? y : x;
    return size_t(m0) + hi * (hi + 1) / 2 + lo;
}

template <int LAB, int LCD, int SINK>
__global__ __launch_bounds__(ERI_BLOCK) void eri_class_kernel(EriArgs a, const uint2* __restrict__ quartets,
                                                              const uint2* __restrict__ aux, long long nq) {
    constexpr int L = LAB + LCD, E = cube_edge(LAB, LCD), CUBE = cube_doubles(LAB, LCD);
    constexpr int NHAB = nherm_c(LAB), NHCD = nherm_c(LCD), NR = nherm_c(L);
    constexpr int BLK = blk_doubles(LAB, LCD), MAXR = (BLK + ERI_BLOCK - 1) / ERI_BLOCK;
    __shared__ EriLds<LAB, LCD> lds;
    double* const s_buf = lds.buf;
    double* const s_sgn = lds.sgn;
    int* const s_offa = lds.offa;
    int* const s_offc = lds.offc;
    int* const s_rl = lds.rl;
    const int lane = threadIdx.x;

    for (int k = lane; k < NHAB; k += ERI_BLOCK) {
        const int p = a.tabs[LAB * NH_MAX + k];
        s_offa[k] = ((p & 255) * E + ((p >> 8) & 255)) * E + (p >> 16);
    }
    for (int k = lane; k < NHCD; k += ERI_BLOCK) {
        const int p = a.tabs[LCD * NH_MAX + k];
        s_offc[k] = ((p & 255) * E + ((p >> 8) & 255)) * E + (p >> 16);
        s_sgn[k] = (((p & 255) + ((p >> 8) & 255) + (p >> 16)) & 1) ? -1.0 : 1.0;
    }
    for (int k = lane; k < NR; k += ERI_BLOCK) s_rl[k] = a.tabs[NLP * NH_MAX + k];
    __syncthreads();

    double* const w = s_buf + 2 * CUBE;
    for (long long qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const uint2 ql = quartets[qi];
        const DevPair ab = a.pairs[ql.x], cd = a.pairs[ql.y];
        const int nab = ab.nab, ncd = cd.nab, nout = nab * ncd;
        double acc[MAXR];
        int aoff[MAXR], coff[MAXR];
#pragma unroll
        for (int r = 0; r < MAXR; ++r) {
            const int idx = lane + ERI_BLOCK * r, aa = idx / ncd;
            acc[r] = 0.0;
            aoff[r] = aa * NHAB;
            coff[r] = (idx - aa * ncd) * NHAB;
        }
        for (int i = 0; i < ab.nprim; ++i) {
            const double* pp = a.prim + 4 * (ab.prim_off + i);
            const double p = pp[0], px = pp[1], py = pp[2], pz = pp[3];
            const double* hab = a.h + ab.h_off + size_t(i) * nab * NHAB;
            for (int j = 0; j < cd.nprim; ++j) {
                const double* qq = a.prim + 4 * (cd.prim_off + j);
                const double q = qq[0];
                // erf(omega r12) / r12: p + q + p q / omega^2 in the place of p + q (Engine::inv_w2); p + q itself for 1 / r12
                const double pq_w = p + q + p * q * a.inv_w2;
                const double alpha = p * q / pq_w;
                const double x = px - qq[1], y = py - qq[2], z = pz - qq[3];
                // hermite_r: F_n(alpha |PQ|^2), then R^n_tuv for n = L .. 0, each pass from the one before
                double f[L + 1], pw[L + 1];
                boys_eval<L>(a.boys, alpha * (x * x + y * y + z * z), f);
                pw[0] = 1.0;
#pragma unroll
                for (int n = 1; n <= L; ++n) pw[n] = pw[n - 1] * (-2.0 * alpha);
                double* cur = s_buf;
                double* old = s_buf + CUBE;
#pragma unroll
                for (int n = L; n >= 0; --n) {
                    const int cnt = nherm_c(L - n);
                    for (int k = lane; k < cnt; k += ERI_BLOCK) {
                        const int pk = s_rl[k], t = pk & 255, u = (pk >> 8) & 255, v = pk >> 16;
                        double val;
                        if (k == 0) {
                            val = pw[n] * f[n];
                        } else if (t > 0) {
                            val = x * old[((t - 1) * E + u) * E + v];
                            if (t > 1) val += (t - 1) * old[((t - 2) * E + u) * E + v];
                        } else if (u > 0) {
                            val = y * old[(t * E + u - 1) * E + v];
                            if (u > 1) val += (u - 1) * old[(t * E + u - 2) * E + v];
                        } else {
                            val = z * old[(t * E + u) * E + v - 1];
                            if (v > 1) val += (v - 1) * old[(t * E + u) * E + v - 2];
                        }
                        cur[(t * E + u) * E + v] = val;
                    }
                    __syncthreads();
                    double* s = cur; cur = old; old = s;
                }
                const double* rb = old;  // the last pass
                const double pref = a.pref0 / (p * q * sqrt(pq_w));
                const double* hcd = a.h + cd.h_off + size_t(j) * ncd * NHCD;
                // w[c][k_ab] = pref sum_k_cd (-1)^(tau+nu+phi) H_cd[c][k_cd] R[k_ab + k_cd]
                for (int idx = lane; idx < ncd * NHAB; idx += ERI_BLOCK) {
                    const int c = idx / NHAB, ka = idx - c * NHAB;
                    const double* hc = hcd + c * NHCD;
                    const int oa = s_offa[ka];
                    double s = 0.0;
#pragma unroll
                    for (int kc = 0; kc < NHCD; ++kc) s += s_sgn[kc] * hc[kc] * rb[oa + s_offc[kc]];
                    w[idx] = s * pref;
                }
                __syncthreads();
                // blk[a][c] += sum_k_ab H_ab[a][k_ab] w[c][k_ab]
#pragma unroll
                for (int r = 0; r < MAXR; ++r)
                    if (lane + ERI_BLOCK * r < nout) {
                        const double* ha = hab + aoff[r];
                        const double* wc = w + coff[r];
                        double s = 0.0;
#pragma unroll
                        for (int ka = 0; ka < NHAB; ++ka) s += ha[ka] * wc[ka];
                        acc[r] += s;
                    }
                __syncthreads();  // w and the cubes are rewritten by the next primitive pair
            }
        }

        // Cartesian block into LDS, then the spherical transform axis by axis (Engine::to_spherical)
        const DevShell sh[4] = {a.shells[ab.ia], a.shells[ab.ib], a.shells[cd.ia], a.shells[cd.ib]};
        double* src = s_buf;
        double* dst = s_buf + BLK;
#pragma unroll
        for (int r = 0; r < MAXR; ++r)
            if (lane + ERI_BLOCK * r < nout) src[lane + ERI_BLOCK * r] = acc[r];
        __syncthreads();
        int dims[4] = {sh[0].ncart, sh[1].ncart, sh[2].ncart, sh[3].ncart};
#pragma unroll
        for (int ax = 0; ax < 4; ++ax) {
            if (sh[ax].l < 2) continue;  // identity for s and p
            const int nc = dims[ax], ns = sh[ax].nsph;
            int outer = 1, inner = 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < ax) outer *= dims[k];
                if (k > ax) inner *= dims[k];
            }
            const double* sm = a.sph + sh[ax].sph_off;
            const int total = outer * ns * inner;
            for (int idx = lane; idx < total; idx += ERI_BLOCK) {
                const int o = idx / (ns * inner), rem = idx - o * ns * inner, m = rem / inner, in = rem - m * inner;
                double s = 0.0;
                for (int c = 0; c < nc; ++c) s += sm[m * nc + c] * src[(o * nc + c) * inner + in];
                dst[idx] = s;
            }
            dims[ax] = ns;
            __syncthreads();
            double* s = src; src = dst; dst = s;
        }

        // Where shells coincide (ia == ib, ic == id, ij == kl) several (a, b, c, d) of this block name the same integral;
        // the host engine's loops leave the value of the last of them in (a, b, c, d) order in all their images, so only
        // that one is stored, by every sink: to the eight images of the tensor, or to those of them the sink keeps.
        const int na = dims[0], nb = dims[1], nc = dims[2], nd = dims[3];
        const bool same_ab = ab.ia == ab.ib, same_cd = cd.ia == cd.ib, same_q = ql.x == ql.y;
        const size_t n = size_t(a.nao), n2 = n * n, n3 = n2 * n;
        uint2 col = make_uint2(0u, 0u);
        if constexpr (SINK == SINK_COLUMN) col = aux[qi];
        for (int idx = lane; idx < na * nb * nc * nd; idx += ERI_BLOCK) {
            int t = idx;
            const int d = t % nd; t /= nd;
            const int c = t % nc; t /= nc;
            const int b = t % nb;
            const int aa = t / nb;
            bool last = true;
            for (int sq = 0; sq <= (same_q ? 1 : 0); ++sq) {
                const int a1 = sq ? c : aa, b1 = sq ? d : b, c1 = sq ? aa : c, d1 = sq ? b : d;
                for (int s1 = 0; s1 <= (same_ab ? 1 : 0); ++s1)
                    for (int s2 = 0; s2 <= (same_cd ? 1 : 0); ++s2) {
                        const int a2 = s1 ? b1 : a1, b2 = s1 ? a1 : b1, c2 = s2 ? d1 : c1, d2 = s2 ? c1 : d1;
                        if (((a2 * nb + b2) * nc + c2) * nd + d2 > idx) last = false;
                    }
            }
            if (!last) continue;
            const double val = src[idx];
            const size_t p = sh[0].ao0 + aa, q = sh[1].ao0 + b, r = sh[2].ao0 + c, s = sh[3].ao0 + d;
            double* out = a.out;
            if constexpr (SINK == SINK_DENSE) {
                out[p * n3 + q * n2 + r * n + s] = val;
                out[q * n3 + p * n2 + r * n + s] = val;
                out[p * n3 + q * n2 + s * n + r] = val;
                out[q * n3 + p * n2 + s * n + r] = val;
                out[r * n3 + s * n2 + p * n + q] = val;
                out[s * n3 + r * n2 + p * n + q] = val;
                out[r * n3 + s * n2 + q * n + p] = val;
                out[s * n3 + r * n2 + q * n + p] = val;
            } else if constexpr (SINK == SINK_DIAG) {
                // (ij, ij): the block's element (a, b, a, b) names (pq|pq).  Within one shell (b, a, a, b) names it too,
                // but the last of the orbit in (a, b, c, d) order is (hi, lo, hi, lo), which has this form itself.
                if (aa == c && b == d) {
                    out[p * n + q] = val;
                    out[q * n + p] = val;
                }
            } else {
                // the selected pair is the ket (col.y == 0), the bra (1), or both (ij == kl)
                if (col.y == 0u) {
                    double* slice = out + column_of(col.x, same_cd, c, d, nd) * n2;
                    slice[p * n + q] = val;
                    slice[q * n + p] = val;
                }
                if (col.y != 0u || same_q) {
                    double* slice = out + column_of(col.x, same_ab, aa, b, nb) * n2;
                    slice[r * n + s] = val;
                    slice[s * n + r] = val;
                }
            }
        }
        __syncthreads();  // the next quartet reuses the buffers
    }
}

template <int LAB, int LCD, int SINK>
void launch_class(hipStream_t stream, const EriArgs& args, const uint2* d_quartets, const uint2* d_aux, int64_t count) {
    hipLaunchKernelGGL((eri_class_kernel<LAB, LCD, SINK>), dim3((unsigned)grid_of(LAB, LCD, count)), dim3(ERI_BLOCK), 0, stream, args,
                       d_quartets, d_aux, (long long)count);
}

using launch_fn = void (*)(hipStream_t, const EriArgs&, const uint2*, const uint2*, int64_t);
#define ERI_ROW(A, S) launch_class<A, 0, S>, launch_class<A, 1, S>, launch_class<A, 2, S>, launch_class<A, 3, S>, launch_class<A, 4, S>
const launch_fn LAUNCH[NCLASS] = {ERI_ROW(0, SINK_DENSE), ERI_ROW(1, SINK_DENSE), ERI_ROW(2, SINK_DENSE), ERI_ROW(3, SINK_DENSE),
                                  ERI_ROW(4, SINK_DENSE)};
const launch_fn LAUNCH_COLUMN[NCLASS] = {ERI_ROW(0, SINK_COLUMN), ERI_ROW(1, SINK_COLUMN), ERI_ROW(2, SINK_COLUMN),
                                         ERI_ROW(3, SINK_COLUMN), ERI_ROW(4, SINK_COLUMN)};
#undef ERI_ROW
// a diagonal quartet is (ij, ij): only the classes l_ab == l_cd exist
const launch_fn LAUNCH_DIAG[NLP] = {launch_class<0, 0, SINK_DIAG>, launch_class<1, 1, SINK_DIAG>, launch_class<2, 2, SINK_DIAG>,
                                    launch_class<3, 3, SINK_DIAG>, launch_class<4, 4, SINK_DIAG>};

// ------------------------------------------------------------------------------------------ host side
struct Plan {
    Engine eng;
    int64_t counts[NCLASS] = {};
    std::vector<uint2> quartets;  // class after class (want_lists)
};

// Shells, index tables and pair data; NBX_E_INVALID where nbx_host_eri refuses the shells, and for l > 2.
int make_engine(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres, const double* exps,
                const double* coefs, const double* sph, double cutoff, double inv_w2, Engine& eng) {
    if (nshell <= 0 || !ang || !nprim || !nfunc || !centres || !exps || !coefs || !sph) return NBX_E_INVALID;
    eng.cutoff = cutoff;
    eng.inv_w2 = inv_w2;
    if (engine_shells(eng, nshell, ang, nprim, nfunc, centres, exps, coefs, sph, DEV_LMAX) != NBX_OK) return NBX_E_INVALID;
    engine_tables(eng);
    engine_pairs(eng, std::min(pool_size(0), 16));
    return NBX_OK;
}

// What nbx_eri_plan and nbx_eri_device start from: the engine and the canonical quartets of the dense tensor.  The lists
// do not depend on inv_w2 (the Schwarz bounds are those of 1 / r12), so nbx_eri_plan answers for every omega.
int make_plan(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres, const double* exps,
              const double* coefs, const double* sph, double cutoff, double inv_w2, bool want_lists, Plan& pl) {
    Engine& eng = pl.eng;
    if (make_engine(nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, inv_w2, eng) != NBX_OK) return NBX_E_INVALID;
    const int64_t npair = int64_t(eng.pairs.size());
    auto each = [&](auto&& fn) {
        for (int64_t ij = npair - 1; ij >= 0; --ij) {
            const Pair& ab = eng.pairs[ij];
            if (ab.nprim == 0) continue;
            for (int64_t kl = 0; kl <= ij; ++kl) {
                const Pair& cd = eng.pairs[kl];
                if (quartet_survives(ab, cd, cutoff)) fn(ab.lab * NLP + cd.lab, ij, kl);
            }
        }
    };
    each([&](int cls, int64_t, int64_t) { ++pl.counts[cls]; });
    if (want_lists) {
        int64_t fill[NCLASS], total = 0;
        for (int c = 0; c < NCLASS; ++c) { fill[c] = total; total += pl.counts[c]; }
        pl.quartets.resize(size_t(total));
        each([&](int cls, int64_t ij, int64_t kl) { pl.quartets[size_t(fill[cls]++)] = make_uint2(unsigned(ij), unsigned(kl)); });
    }
    return NBX_OK;
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// One host image of everything but the lists: shells, pairs, primitives, H, sph, Boys table, index tables.
struct Image {
    std::vector<char> bytes;
    size_t o_shell, o_pair, o_prim, o_h, o_sph, o_boys, o_tabs;
};

void build_image(const Engine& eng, Image& im) {
    const size_t nshells = eng.shells.size(), npairs = eng.pairs.size();
    size_t nprims = 0, nh = 0, nsph = 0;
    for (const Pair& pr : eng.pairs) { nprims += size_t(pr.nprim); nh += pr.h.size(); }
    for (const Shell& s : eng.shells) nsph += size_t(s.nsph) * s.ncart_;
    im.o_shell = 0;
    im.o_pair = align256(im.o_shell + nshells * sizeof(DevShell));
    im.o_prim = align256(im.o_pair + npairs * sizeof(DevPair));
    im.o_h = align256(im.o_prim + nprims * 4 * sizeof(double));
    im.o_sph = align256(im.o_h + nh * sizeof(double));
    im.o_boys = align256(im.o_sph + nsph * sizeof(double));
    im.o_tabs = align256(im.o_boys + eng.boys.f.size() * sizeof(double));
    im.bytes.assign(align256(im.o_tabs + (NLP * NH_MAX + NR_MAX) * sizeof(int)), 0);
    std::vector<char>& img = im.bytes;
    DevShell* ds = reinterpret_cast<DevShell*>(&img[im.o_shell]);
    size_t so = 0;
    double* dsph = reinterpret_cast<double*>(&img[im.o_sph]);
    for (size_t s = 0; s < nshells; ++s) {
        const Shell& sh = eng.shells[s];
        ds[s] = {sh.l, sh.ncart_, sh.nsph, sh.ao0, (long long)so};
        std::memcpy(dsph + so, sh.sph, sizeof(double) * sh.nsph * sh.ncart_);
        so += size_t(sh.nsph) * sh.ncart_;
    }
    DevPair* dp = reinterpret_cast<DevPair*>(&img[im.o_pair]);
    double* dprim = reinterpret_cast<double*>(&img[im.o_prim]);
    double* dh = reinterpret_cast<double*>(&img[im.o_h]);
    size_t po = 0, ho = 0;
    for (size_t k = 0; k < npairs; ++k) {
        const Pair& pr = eng.pairs[k];
        dp[k] = {pr.ia, pr.ib, pr.nab, pr.nprim, (long long)po, (long long)ho};
        for (int i = 0; i < pr.nprim; ++i) {
            double* q = dprim + 4 * (po + i);
            q[0] = pr.p[i]; q[1] = pr.px[i]; q[2] = pr.py[i]; q[3] = pr.pz[i];
        }
        if (!pr.h.empty()) std::memcpy(dh + ho, pr.h.data(), sizeof(double) * pr.h.size());
        po += size_t(pr.nprim);
        ho += pr.h.size();
    }
    std::memcpy(&img[im.o_boys], eng.boys.f.data(), sizeof(double) * eng.boys.f.size());
    int* tabs = reinterpret_cast<int*>(&img[im.o_tabs]);
    for (int l = 0; l < NLP; ++l)
        for (int k = 0; k < eng.hidx[l].n; ++k)
            tabs[l * NH_MAX + k] = eng.hidx[l].tuv[k][0] | (eng.hidx[l].tuv[k][1] << 8) | (eng.hidx[l].tuv[k][2] << 16);
    int k = 0;  // every (t, u, v) of order <= 8 by total order: the entries of a recursion pass are a prefix
    const HermIndex top(2 * NLP - 2);
    for (int deg = 0; deg <= 2 * NLP - 2; ++deg)
        for (int m = 0; m < top.n; ++m)
            if (top.tuv[m][0] + top.tuv[m][1] + top.tuv[m][2] == deg)
                tabs[NLP * NH_MAX + k++] = top.tuv[m][0] | (top.tuv[m][1] << 8) | (top.tuv[m][2] << 16);
}

EriArgs args_of(const char* d_img, const Image& im, const Engine& eng, double* out) {
    EriArgs args;
    args.shells = reinterpret_cast<const DevShell*>(d_img + im.o_shell);
    args.pairs = reinterpret_cast<const DevPair*>(d_img + im.o_pair);
    args.prim = reinterpret_cast<const double*>(d_img + im.o_prim);
    args.h = reinterpret_cast<const double*>(d_img + im.o_h);
    args.sph = reinterpret_cast<const double*>(d_img + im.o_sph);
    args.boys = reinterpret_cast<const double*>(d_img + im.o_boys);
    args.tabs = reinterpret_cast<const int*>(d_img + im.o_tabs);
    args.out = out;
    args.pref0 = 2.0 * std::pow(M_PI, 2.5);
    args.inv_w2 = eng.inv_w2;
    args.nao = eng.nao;
    return args;
}

std::mutex g_times_mutex;
std::vector<hipEvent_t> g_events;  // (start, stop) per class of the last bracketed nbx_eri_device call
int g_event_class[NCLASS];
int g_event_n = 0;

void drop_events() {
    for (hipEvent_t e : g_events) (void)hipEventDestroy(e);
    g_events.clear();
    g_event_n = 0;
}

}  // namespace

extern "C" int nbx_eri_plan(int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                            const double* exps, const double* coefs, const double* sph, double cutoff, int64_t* counts_out,
                            int* lds_bytes_out, int* block_out, int64_t* grid_out) {
    if (!counts_out || !lds_bytes_out || !block_out || !grid_out) return NBX_E_INVALID;
    Plan pl;
    const int rc = make_plan(nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, 0.0, false, pl);
    if (rc != NBX_OK) return rc;
    for (int lab = 0; lab < NLP; ++lab)
        for (int lcd = 0; lcd < NLP; ++lcd) {
            const int c = lab * NLP + lcd;
            counts_out[c] = pl.counts[c];
            lds_bytes_out[c] = lds_bytes_of(lab, lcd);
            block_out[c] = ERI_BLOCK;
            grid_out[c] = grid_of(lab, lcd, pl.counts[c]);
        }
    return NBX_OK;
}

namespace {

// nbx_eri_device (inv_w2 = 0) and nbx_eri_device_erf (inv_w2 = 1 / omega^2)
int eri_device(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
               const double* exps, const double* coefs, const double* sph, double cutoff, double inv_w2, double* out_device) {
    NBX_CHECK_ARG(ctx != nullptr);
    NBX_CHECK_ARG(out_device != nullptr);
    Plan pl;
    if (make_plan(nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, inv_w2, true, pl) != NBX_OK) {
        nbx_set_error("nbx_eri_device: invalid shells (angular momentum 0 .. %d, nfunc = 2l+1 or (l+1)(l+2)/2)", DEV_LMAX);
        return NBX_E_INVALID;
    }
    const Engine& eng = pl.eng;
    const size_t n = size_t(eng.nao);
    NBX_HIP(hipMemsetAsync(out_device, 0, sizeof(double) * n * n * n * n, ctx->stream));

    Image im;
    build_image(eng, im);
    const size_t bytes = im.bytes.size();
    char* d_img = nullptr;
    uint2* d_q = nullptr;
    const size_t qbytes = std::max<size_t>(pl.quartets.size() * sizeof(uint2), 8);
    NBX_HIP(hipMallocAsync(reinterpret_cast<void**>(&d_img), bytes, ctx->stream));
    if (hipMallocAsync(reinterpret_cast<void**>(&d_q), qbytes, ctx->stream) != hipSuccess) {
        (void)hipFreeAsync(d_img, ctx->stream);
        nbx_set_error("nbx_eri_device: %zu bytes of quartet lists do not fit", qbytes);
        return NBX_E_NOMEM;
    }
    int rc = NBX_OK;
    auto fail = [&](hipError_t e, const char* what) {
        nbx_set_error("nbx_eri_device: %s -> %s", what, hipGetErrorString(e));
        rc = NBX_E_HIP;
    };
    hipError_t e = hipMemcpyAsync(d_img, im.bytes.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) fail(e, "upload of the pair data");
    if (rc == NBX_OK && !pl.quartets.empty()) {
        e = hipMemcpyAsync(d_q, pl.quartets.data(), pl.quartets.size() * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) fail(e, "upload of the quartet lists");
    }
    if (rc == NBX_OK) {
        // the host images die with this call: the copies out of pageable memory must have left them
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) fail(e, "hipStreamSynchronize");
    }
    if (rc == NBX_OK) {
        const EriArgs args = args_of(d_img, im, eng, out_device);
        const bool timed = ctx->profiling && ((ctx->prof_mask >> NBX_PROF_ERI) & 1u);
        std::lock_guard<std::mutex> lock(g_times_mutex);
        if (timed) drop_events();
        int64_t off = 0;
        for (int c = 0; c < NCLASS && rc == NBX_OK; ++c) {
            const int64_t cnt = pl.counts[c];
            if (cnt == 0) continue;
            hipEvent_t ev[2] = {nullptr, nullptr};
            if (timed && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess)
                (void)hipEventRecord(ev[0], ctx->stream);
            LAUNCH[c](ctx->stream, args, d_q + off, nullptr, cnt);
            e = hipGetLastError();
            if (e != hipSuccess) fail(e, "launch");
            if (timed && ev[0] && ev[1]) {
                (void)hipEventRecord(ev[1], ctx->stream);
                g_events.push_back(ev[0]);
                g_events.push_back(ev[1]);
                g_event_class[g_event_n++] = c;
            }
            off += cnt;
        }
    }
    (void)hipFreeAsync(d_q, ctx->stream);
    (void)hipFreeAsync(d_img, ctx->stream);
    return rc;
}

}  // namespace

extern "C" int nbx_eri_device(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc,
                              const double* centres, const double* exps, const double* coefs, const double* sph,
                              double cutoff, double* out_device) {
    return eri_device(ctx, nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, 0.0, out_device);
}

extern "C" int nbx_eri_device_erf(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc,
                                  const double* centres, const double* exps, const double* coefs, const double* sph,
                                  double cutoff, double omega, double* out_device) {
    if (!(omega > 0.0) || !std::isfinite(omega)) {
        nbx_set_error("nbx_eri_device_erf: omega = %g; a finite omega > 0 is required", omega);
        return NBX_E_INVALID;
    }
    return eri_device(ctx, nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, 1.0 / (omega * omega), out_device);
}

// ------------------------------------------------------------------------------------------ diagonal and columns
namespace nbx_eri {

int session_open(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                 const double* exps, const double* coefs, const double* sph, double cutoff, Session& s) {
    if (make_engine(nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, 0.0, s.eng) != NBX_OK) return NBX_E_INVALID;
    s.stream = ctx->stream;
    s.cutoff = cutoff;
    Image im;
    build_image(s.eng, im);
    NBX_HIP(hipMallocAsync(reinterpret_cast<void**>(&s.d_img), im.bytes.size(), s.stream));
    hipError_t e = hipMemcpyAsync(s.d_img, im.bytes.data(), im.bytes.size(), hipMemcpyHostToDevice, s.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);  // the image dies with this call
    if (e != hipSuccess) {
        nbx_set_error("upload of the pair data -> %s", hipGetErrorString(e));
        session_close(s);
        return NBX_E_HIP;
    }
    s.args = args_of(s.d_img, im, s.eng, nullptr);
    return NBX_OK;
}

void session_close(Session& s) {
    if (s.d_img) (void)hipFreeAsync(s.d_img, s.stream);
    s.d_img = nullptr;
}

// memset, the lists behind it (stream-ordered scratch), one launch per non-empty class
static int run_lists(Session& s, const launch_fn* table, bool diag, const int64_t* counts, const uint2* quartets,
                     const uint2* aux, size_t total, double* out, size_t out_doubles, const int* col_pq, size_t ncols,
                     int* d_col_pq) {
    NBX_HIP(hipMemsetAsync(out, 0, sizeof(double) * out_doubles, s.stream));
    if (d_col_pq && ncols) NBX_HIP(hipMemcpyAsync(d_col_pq, col_pq, sizeof(int) * ncols, hipMemcpyHostToDevice, s.stream));
    if (total == 0) return NBX_OK;
    uint2* d_q = nullptr;
    const size_t half = align256(total * sizeof(uint2));
    if (hipMallocAsync(reinterpret_cast<void**>(&d_q), 2 * half, s.stream) != hipSuccess) {
        nbx_set_error("%zu bytes of quartet lists do not fit", 2 * half);
        return NBX_E_NOMEM;
    }
    uint2* d_aux = aux ? reinterpret_cast<uint2*>(reinterpret_cast<char*>(d_q) + half) : nullptr;
    int rc = NBX_OK;
    hipError_t e = hipMemcpyAsync(d_q, quartets, total * sizeof(uint2), hipMemcpyHostToDevice, s.stream);
    if (e == hipSuccess && aux) e = hipMemcpyAsync(d_aux, aux, total * sizeof(uint2), hipMemcpyHostToDevice, s.stream);
    EriArgs args = s.args;
    args.out = out;
    int64_t off = 0;
    for (int c = 0; c < NCLASS && e == hipSuccess; ++c) {
        if (counts[c] == 0) continue;
        (diag ? table[c / NLP] : table[c])(s.stream, args, d_q + off, d_aux ? d_aux + off : nullptr, counts[c]);
        e = hipGetLastError();
        off += counts[c];
    }
    if (e != hipSuccess) {
        nbx_set_error("diagonal / column launches -> %s", hipGetErrorString(e));
        rc = NBX_E_HIP;
    }
    (void)hipFreeAsync(d_q, s.stream);
    return rc;
}

int session_diagonal(Session& s, double* d_diag) {
    ColumnLists& l = s.lists;
    for (int64_t& c : l.counts) c = 0;
    l.quartets.clear();
    l.aux.clear();
    // class (l, l) after class: the pairs are few, two passes over them per class are nothing
    for (int lab = 0; lab < NLP; ++lab)
        for (size_t ij = 0; ij < s.eng.pairs.size(); ++ij) {
            const Pair& pr = s.eng.pairs[ij];
            if (pr.lab != lab || !quartet_survives(pr, pr, s.cutoff)) continue;
            ++l.counts[lab * NLP + lab];
            l.quartets.push_back(make_uint2(unsigned(ij), unsigned(ij)));
        }
    const size_t n = size_t(s.eng.nao);
    return run_lists(s, LAUNCH_DIAG, true, l.counts, l.quartets.data(), nullptr, l.quartets.size(), d_diag, n * n, nullptr, 0,
                     nullptr);
}

int session_columns(Session& s, int npair, const int64_t* sel, double* d_cols, int* d_col_pq) {
    build_column_lists(s.eng, npair, sel, s.cutoff, s.lists);
    const ColumnLists& l = s.lists;
    const size_t n = size_t(s.eng.nao);
    return run_lists(s, LAUNCH_COLUMN, false, l.counts, l.quartets.data(), l.aux.data(), l.quartets.size(), d_cols,
                     size_t(l.ncols) * n * n, l.col_pq.data(), size_t(l.ncols), d_col_pq);
}

}  // namespace nbx_eri

namespace {
const char* const SHELL_TEXT = "%s: invalid shells (angular momentum 0 .. %d, nfunc = 2l+1 or (l+1)(l+2)/2)";
}

extern "C" int nbx_eri_diagonal(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc,
                                const double* centres, const double* exps, const double* coefs, const double* sph,
                                double cutoff, double* d_diag) {
    NBX_CHECK_ARG(ctx != nullptr);
    NBX_CHECK_ARG(d_diag != nullptr);
    nbx_eri::Session s;
    int rc = nbx_eri::session_open(ctx, nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, s);
    if (rc == NBX_E_INVALID) nbx_set_error(SHELL_TEXT, "nbx_eri_diagonal", DEV_LMAX);
    if (rc != NBX_OK) return rc;
    rc = nbx_eri::session_diagonal(s, d_diag);
    nbx_eri::session_close(s);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == NBX_OK) rc = NBX_E_HIP;  // the lists die with this call
    return rc;
}

extern "C" int nbx_eri_columns(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc,
                               const double* centres, const double* exps, const double* coefs, const double* sph,
                               double cutoff, int npair, const int* ia, const int* ib, double* d_cols) {
    NBX_CHECK_ARG(ctx != nullptr);
    NBX_CHECK_ARG(d_cols != nullptr);
    NBX_CHECK_ARG(npair >= 0 && (npair == 0 || (ia != nullptr && ib != nullptr)));
    for (int k = 0; k < npair; ++k)
        if (ib[k] < 0 || ia[k] < ib[k] || ia[k] >= nshell) {
            nbx_set_error("nbx_eri_columns: shell pair %d is (%d, %d); %d > ia >= ib >= 0 is required", k, ia[k], ib[k], nshell);
            return NBX_E_INVALID;
        }
    nbx_eri::Session s;
    int rc = nbx_eri::session_open(ctx, nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, s);
    if (rc == NBX_E_INVALID) nbx_set_error(SHELL_TEXT, "nbx_eri_columns", DEV_LMAX);
    if (rc != NBX_OK) return rc;
    std::vector<int64_t> sel(size_t(npair > 0 ? npair : 0));
    for (int k = 0; k < npair; ++k) sel[k] = int64_t(ia[k]) * (ia[k] + 1) / 2 + ib[k];
    rc = nbx_eri::session_columns(s, npair, sel.data(), d_cols, nullptr);
    nbx_eri::session_close(s);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == NBX_OK) rc = NBX_E_HIP;  // the lists die with this call
    return rc;
}

extern "C" int nbx_eri_class_ms(nbx_ctx* ctx, double* ms_out) {
    NBX_CHECK_ARG(ctx != nullptr);
    NBX_CHECK_ARG(ms_out != nullptr);
    std::lock_guard<std::mutex> lock(g_times_mutex);
    for (int c = 0; c < NCLASS; ++c) ms_out[c] = 0.0;
    for (int k = 0; k < g_event_n; ++k) {
        float ms = 0.0f;
        NBX_HIP(hipEventSynchronize(g_events[2 * k + 1]));
        NBX_HIP(hipEventElapsedTime(&ms, g_events[2 * k], g_events[2 * k + 1]));
        ms_out[g_event_class[k]] = double(ms);
    }
    drop_events();
    return NBX_OK;
}
