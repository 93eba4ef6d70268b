// McMurchie-Davidson pieces shared by the host engine (ints_host.cpp) and the device engine (eri.hip): shells,
// the Boys table, Hermite densities of a shell pair, R_tuv, the Cartesian block of one quartet, and the set-up
// both engines start from (shell checks, index tables, pair data with their Schwarz bounds).  One copy, so
// the two engines index pairs, screen primitives and skip quartets identically.
#pragma once

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/nbx.h"

namespace nbx_md {

constexpr int LMAX = 3;               // per shell (s, p, d, f)
constexpr int LTOT = 4 * LMAX;        // highest Hermite order of a quartet
constexpr int NCUBE = LTOT + 1;

inline int ncart(int l) { return (l + 1) * (l + 2) / 2; }
inline int nherm(int l) { return (l + 1) * (l + 2) * (l + 3) / 6; }

// Cartesian components in the order of integrals.py's _CART: xx xy xz yy yz zz for d, xxx xxy xxz xyy .. zzz for f
inline void cart_list(int l, int (*out)[3]) {
    int k = 0;
    for (int lx = l; lx >= 0; --lx)
        for (int ly = l - lx; ly >= 0; --ly) {
            out[k][0] = lx; out[k][1] = ly; out[k][2] = l - lx - ly;
            ++k;
        }
}

// ------------------------------------------------------------------------------------------ Boys function
struct BoysTable {
    static constexpr double STEP = 0.1, TMAX = 42.0;
    static constexpr int NT = 421, NORD = LTOT + 10;
    std::vector<double> f;  // [NT][NORD + 1]
    BoysTable() : f(size_t(NT) * (NORD + 1)) {
        for (int i = 0; i < NT; ++i) {
            const double t = i * STEP;
            // F_top by its convergent series e^-T sum_k (2T)^k / ((2n+1)(2n+3)...(2n+2k+1)), then downwards
            const int n = NORD;
            double term = 1.0 / (2 * n + 1), sum = term;
            for (int k = 1; k < 400; ++k) {
                term *= 2.0 * t / (2 * n + 2 * k + 1);
                sum += term;
                if (term < 1e-18 * sum) break;
            }
            const double et = std::exp(-t);
            double* row = &f[size_t(i) * (NORD + 1)];
            row[n] = et * sum;
            for (int m = n; m > 0; --m) row[m - 1] = (2.0 * t * row[m] + et) / (2 * m - 1);
        }
    }
    // F_0 .. F_l at T
    void eval(int l, double t, double* out) const {
        if (t >= TMAX - 1.0) {  // asymptotic F_0, upward recursion (stable for large T)
            const double et = std::exp(-t);
            out[0] = 0.5 * std::sqrt(M_PI / t);
            for (int m = 0; m < l; ++m) out[m + 1] = ((2 * m + 1) * out[m] - et) / (2.0 * t);
            return;
        }
        const int i = int(t / STEP + 0.5);
        const double d = i * STEP - t;  // |d| <= STEP / 2
        const double* row = &f[size_t(i) * (NORD + 1)];
        double acc = 0.0, pw = 1.0;
        for (int k = 0; k < 9; ++k) {  // F_l(T) = sum_k F_{l+k}(T0) (T0 - T)^k / k!
            acc += row[l + k] * pw;
            pw *= d / (k + 1);
        }
        out[l] = acc;
        const double et = std::exp(-t);
        for (int m = l; m > 0; --m) out[m - 1] = (2.0 * t * out[m] + et) / (2 * m - 1);
    }
};

// ------------------------------------------------------------------------------------------ shell pairs
struct Shell {
    int l, nprim, ncart_, nsph, ao0;
    const double *exps, *coefs, *sph;
    double c[3];
};

struct Pair {
    int ia, ib, lab, nab, nh, nprim;
    std::vector<double> p, px, py, pz;  // per surviving primitive pair
    std::vector<double> h;              // [prim][nab][nh]
    double schwarz = 0.0;
};

struct HermIndex {  // compact list of (t, u, v), t + u + v <= l
    int n;
    int tuv[165][3];
    explicit HermIndex(int l = 0) {
        n = 0;
        for (int t = 0; t <= l; ++t)
            for (int u = 0; u <= l - t; ++u)
                for (int v = 0; v <= l - t - u; ++v) {
                    tuv[n][0] = t; tuv[n][1] = u; tuv[n][2] = v;
                    ++n;
                }
    }
};

inline void hermite_e(int la, int lb, double a, double b, double xab, double e[LMAX + 1][LMAX + 1][2 * LMAX + 1]) {
    const double p = a + b, mu = a * b / p;
    const double xpa = -b / p * xab, xpb = a / p * xab, half = 0.5 / p;
    for (int i = 0; i <= LMAX; ++i)
        for (int j = 0; j <= LMAX; ++j)
            for (int t = 0; t <= 2 * LMAX; ++t) e[i][j][t] = 0.0;
    e[0][0][0] = std::exp(-mu * xab * xab);
    for (int i = 0; i < la; ++i)
        for (int t = 0; t <= i + 1; ++t) {
            double v = xpa * e[i][0][t];
            if (t > 0) v += half * e[i][0][t - 1];
            if (t + 1 <= i) v += (t + 1) * e[i][0][t + 1];
            e[i + 1][0][t] = v;
        }
    for (int i = 0; i <= la; ++i)
        for (int j = 0; j < lb; ++j)
            for (int t = 0; t <= i + j + 1; ++t) {
                double v = xpb * e[i][j][t];
                if (t > 0) v += half * e[i][j][t - 1];
                if (t + 1 <= i + j) v += (t + 1) * e[i][j][t + 1];
                e[i][j + 1][t] = v;
            }
}

inline void build_pair(const Shell& sa, const Shell& sb, int ia, int ib, double prim_cutoff, const HermIndex* hidx, Pair& pr) {
    pr.ia = ia; pr.ib = ib;
    pr.lab = sa.l + sb.l;
    pr.nab = sa.ncart_ * sb.ncart_;
    pr.nh = nherm(pr.lab);
    int ca[10][3], cb[10][3];
    cart_list(sa.l, ca);
    cart_list(sb.l, cb);
    const HermIndex& hi = hidx[pr.lab];
    double r2 = 0.0, ab[3];
    for (int d = 0; d < 3; ++d) { ab[d] = sa.c[d] - sb.c[d]; r2 += ab[d] * ab[d]; }
    for (int i = 0; i < sa.nprim; ++i)
        for (int j = 0; j < sb.nprim; ++j) {
            const double a = sa.exps[i], b = sb.exps[j], p = a + b;
            const double w = sa.coefs[i] * sb.coefs[j];
            if (std::fabs(w) * std::exp(-a * b / p * r2) < prim_cutoff) continue;
            double ex[LMAX + 1][LMAX + 1][2 * LMAX + 1], ey[LMAX + 1][LMAX + 1][2 * LMAX + 1], ez[LMAX + 1][LMAX + 1][2 * LMAX + 1];
            hermite_e(sa.l, sb.l, a, b, ab[0], ex);
            hermite_e(sa.l, sb.l, a, b, ab[1], ey);
            hermite_e(sa.l, sb.l, a, b, ab[2], ez);
            pr.p.push_back(p);
            pr.px.push_back((a * sa.c[0] + b * sb.c[0]) / p);
            pr.py.push_back((a * sa.c[1] + b * sb.c[1]) / p);
            pr.pz.push_back((a * sa.c[2] + b * sb.c[2]) / p);
            const size_t base = pr.h.size();
            pr.h.resize(base + size_t(pr.nab) * pr.nh);
            double* h = &pr.h[base];
            for (int x = 0; x < sa.ncart_; ++x)
                for (int y = 0; y < sb.ncart_; ++y) {
                    double* row = h + size_t(x * sb.ncart_ + y) * pr.nh;
                    for (int k = 0; k < hi.n; ++k) {
                        const int t = hi.tuv[k][0], u = hi.tuv[k][1], v = hi.tuv[k][2];
                        double val = 0.0;
                        if (t <= ca[x][0] + cb[y][0] && u <= ca[x][1] + cb[y][1] && v <= ca[x][2] + cb[y][2])
                            val = w * ex[ca[x][0]][cb[y][0]][t] * ey[ca[x][1]][cb[y][1]][u] * ez[ca[x][2]][cb[y][2]][v];
                        row[k] = val;
                    }
                }
        }
    pr.nprim = int(pr.p.size());
}

// R_tuv^0 for t + u + v <= l into a cube of edge NCUBE
inline void hermite_r(int l, double alpha, double x, double y, double z, const BoysTable& boys, double* r /* NCUBE^3 */, double* tmp) {
    double f[LTOT + 1];
    boys.eval(l, alpha * (x * x + y * y + z * z), f);
    double* cur = r;
    double* old = tmp;
    // the final result must land in r: choose the starting buffer by the parity of the number of passes
    if (l % 2 == 1) { cur = tmp; old = r; }
    double pw[LTOT + 1];
    pw[0] = 1.0;
    for (int n = 1; n <= l; ++n) pw[n] = pw[n - 1] * (-2.0 * alpha);
    for (int n = l; n >= 0; --n) {
        const int top = l - n;
        cur[0] = pw[n] * f[n];
        for (int t = 0; t <= top; ++t)
            for (int u = 0; u <= top - t; ++u)
                for (int v = 0; v <= top - t - u; ++v) {
                    if (t + u + v == 0) continue;
                    double val;
                    if (t > 0) {
                        val = x * old[((t - 1) * NCUBE + u) * NCUBE + v];
                        if (t > 1) val += (t - 1) * old[((t - 2) * NCUBE + u) * NCUBE + v];
                    } else if (u > 0) {
                        val = y * old[(t * NCUBE + u - 1) * NCUBE + v];
                        if (u > 1) val += (u - 1) * old[(t * NCUBE + u - 2) * NCUBE + v];
                    } else {
                        val = z * old[(t * NCUBE + u) * NCUBE + v - 1];
                        if (v > 1) val += (v - 1) * old[(t * NCUBE + u) * NCUBE + v - 2];
                    }
                    cur[(t * NCUBE + u) * NCUBE + v] = val;
                }
        double* s = cur; cur = old; old = s;
    }
}

struct Engine {
    std::vector<Shell> shells;
    std::vector<Pair> pairs;  // ia >= ib, index ia (ia + 1) / 2 + ib
    HermIndex hidx[2 * LMAX + 1];
    // ridx[lab][lcd][k_ab * n_cd + k_cd] = cube offset of (t + tau, u + nu, v + phi); sign of the ket index
    std::vector<int> ridx[2 * LMAX + 1][2 * LMAX + 1];
    double sgn[2 * LMAX + 1][165];
    BoysTable boys;
    int nao = 0;
    double cutoff = 0.0;
    // 1 / omega^2 of the operator erf(omega r12) / r12; 0 is 1 / r12 (omega = infinity).  Per primitive quartet the
    // attenuated integral is the plain one at alpha_w = alpha / (1 + alpha / omega^2) times (1 + alpha / omega^2)^(-1/2)
    // (DESIGN.md section 17).  Both are had by putting p + q + p q / omega^2 where the plain formulas have p + q:
    // alpha_w = p q / that, and the prefactor's sqrt(p + q) becomes its root.  One multiply-add more per primitive
    // quartet, and with 0 the sum is p + q itself: the plain arithmetic is unchanged bit for bit.
    double inv_w2 = 0.0;

    // Cartesian block (nab x ncd) of the quartet (pairs ab, cd)
    void quartet_cart(const Pair& ab, const Pair& cd, double* blk, double* rbuf, double* rtmp, double* w) const {
        const int nab = ab.nab, ncd = cd.nab, nhab = ab.nh, nhcd = cd.nh, l = ab.lab + cd.lab;
        std::memset(blk, 0, sizeof(double) * nab * ncd);
        const int* ri = ridx[ab.lab][cd.lab].data();
        const double* sg = sgn[cd.lab];
        for (int i = 0; i < ab.nprim; ++i) {
            const double p = ab.p[i];
            const double* hab = &ab.h[size_t(i) * nab * nhab];
            for (int j = 0; j < cd.nprim; ++j) {
                const double q = cd.p[j];
                const double pq_w = p + q + p * q * inv_w2;  // (p + q) (1 + alpha / omega^2); p + q exactly for 1 / r12
                const double alpha = p * q / pq_w;
                hermite_r(l, alpha, ab.px[i] - cd.px[j], ab.py[i] - cd.py[j], ab.pz[i] - cd.pz[j], boys, rbuf, rtmp);
                const double pref = 2.0 * std::pow(M_PI, 2.5) / (p * q * std::sqrt(pq_w));
                const double* hcd = &cd.h[size_t(j) * ncd * nhcd];
                // w[c][k_ab] = sum_k_cd (-1)^(tau+nu+phi) H_cd[c][k_cd] R[k_ab + k_cd]
                for (int c = 0; c < ncd; ++c) {
                    const double* hc = hcd + size_t(c) * nhcd;
                    double* wc = w + size_t(c) * nhab;
                    for (int ka = 0; ka < nhab; ++ka) {
                        const int* rk = ri + size_t(ka) * nhcd;
                        double acc = 0.0;
                        for (int kc = 0; kc < nhcd; ++kc) acc += sg[kc] * hc[kc] * rbuf[rk[kc]];
                        wc[ka] = acc * pref;
                    }
                }
                for (int a = 0; a < nab; ++a) {
                    const double* ha = hab + size_t(a) * nhab;
                    double* out = blk + size_t(a) * ncd;
                    for (int c = 0; c < ncd; ++c) {
                        const double* wc = w + size_t(c) * nhab;
                        double acc = 0.0;
                        for (int ka = 0; ka < nhab; ++ka) acc += ha[ka] * wc[ka];
                        out[c] += acc;
                    }
                }
            }
        }
    }

    // Cartesian (na nb nc nd) -> spherical, in place through a scratch buffer; returns the result pointer
    const double* to_spherical(const Pair& ab, const Pair& cd, double* blk, double* scr) const {
        const Shell* sh[4] = {&shells[ab.ia], &shells[ab.ib], &shells[cd.ia], &shells[cd.ib]};
        int dims[4] = {sh[0]->ncart_, sh[1]->ncart_, sh[2]->ncart_, sh[3]->ncart_};
        double* src = blk;
        double* dst = scr;
        for (int ax = 0; ax < 4; ++ax) {
            if (sh[ax]->l < 2) continue;  // identity for s and p (their normalisation sits in the coefficients)
            const int nc = dims[ax], ns = sh[ax]->nsph;
            int outer = 1, inner = 1;
            for (int k = 0; k < ax; ++k) outer *= dims[k];
            for (int k = ax + 1; k < 4; ++k) inner *= dims[k];
            for (int o = 0; o < outer; ++o)
                for (int m = 0; m < ns; ++m)
                    for (int in = 0; in < inner; ++in) {
                        double acc = 0.0;
                        for (int c = 0; c < nc; ++c) acc += sh[ax]->sph[m * nc + c] * src[(size_t(o) * nc + c) * inner + in];
                        dst[(size_t(o) * ns + m) * inner + in] = acc;
                    }
            dims[ax] = ns;
            double* s = src; src = dst; dst = s;
        }
        return src;
    }
};

template <class Body>
inline void run_pool(int nthreads, Body&& body) {
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t) pool.emplace_back(body);
    body();
    for (auto& th : pool) th.join();
}

inline int pool_size(int nthreads) {
    if (nthreads <= 0) nthreads = int(std::thread::hardware_concurrency());
    return nthreads <= 0 ? 1 : nthreads;
}

// Shells from the caller's arrays (the arguments of nbx_host_eri); lmax: highest angular momentum accepted.
inline int engine_shells(Engine& eng, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                         const double* exps, const double* coefs, const double* sph, int lmax) {
    eng.shells.resize(nshell);
    int poff = 0, soff = 0, ao = 0;
    for (int s = 0; s < nshell; ++s) {
        if (ang[s] < 0 || ang[s] > lmax || nprim[s] <= 0) return NBX_E_INVALID;
        Shell& sh = eng.shells[s];
        sh.l = ang[s];
        sh.nprim = nprim[s];
        sh.ncart_ = ncart(sh.l);
        sh.nsph = nfunc[s];  // 2 l + 1 spherical functions, or all Cartesian components (PySCF's mol.cart)
        if (sh.nsph != 2 * sh.l + 1 && sh.nsph != sh.ncart_) return NBX_E_INVALID;
        sh.exps = exps + poff;
        sh.coefs = coefs + poff;
        sh.sph = sph + soff;
        sh.ao0 = ao;
        for (int d = 0; d < 3; ++d) sh.c[d] = centres[3 * s + d];
        poff += sh.nprim;
        soff += sh.nsph * sh.ncart_;
        ao += sh.nsph;
    }
    eng.nao = ao;
    return NBX_OK;
}

inline void engine_tables(Engine& eng) {
    for (int l = 0; l <= 2 * LMAX; ++l) eng.hidx[l] = HermIndex(l);
    for (int lab = 0; lab <= 2 * LMAX; ++lab)
        for (int lcd = 0; lcd <= 2 * LMAX; ++lcd) {
            const HermIndex &ha = eng.hidx[lab], &hc = eng.hidx[lcd];
            auto& tab = eng.ridx[lab][lcd];
            tab.resize(size_t(ha.n) * hc.n);
            for (int ka = 0; ka < ha.n; ++ka)
                for (int kc = 0; kc < hc.n; ++kc)
                    tab[size_t(ka) * hc.n + kc] = ((ha.tuv[ka][0] + hc.tuv[kc][0]) * NCUBE + ha.tuv[ka][1] + hc.tuv[kc][1]) * NCUBE +
                                                  ha.tuv[ka][2] + hc.tuv[kc][2];
        }
    for (int l = 0; l <= 2 * LMAX; ++l)
        for (int k = 0; k < eng.hidx[l].n; ++k)
            eng.sgn[l][k] = ((eng.hidx[l].tuv[k][0] + eng.hidx[l].tuv[k][1] + eng.hidx[l].tuv[k][2]) & 1) ? -1.0 : 1.0;
}

// pair data and Schwarz bounds sqrt(max (ab|ab)) of every shell pair ia >= ib, over nthreads threads.  The bounds are
// those of 1 / r12 whatever eng.inv_w2 is set to afterwards: (ab|ab)_omega <= (ab|ab) (the Fourier transform of
// erf(omega r) / r is that of 1 / r times exp(-k^2 / 4 omega^2) <= 1), so they bound the attenuated quartets too and
// every omega runs the same quartet lists.
inline void engine_pairs(Engine& eng, int nthreads) {
    const int nshell = int(eng.shells.size());
    const int64_t npair = int64_t(nshell) * (nshell + 1) / 2;
    eng.pairs.resize(npair);
    const double prim_cutoff = eng.cutoff * 1e-4;
    const double inv_w2 = eng.inv_w2;
    eng.inv_w2 = 0.0;
    std::atomic<int64_t> next{0};
    run_pool(nthreads, [&] {
        std::vector<double> blk(100 * 100), w(100 * 84), rbuf(NCUBE * NCUBE * NCUBE), rtmp(NCUBE * NCUBE * NCUBE);
        for (;;) {
            const int64_t ij = next.fetch_add(1);
            if (ij >= npair) break;
            int ia = int((std::sqrt(8.0 * double(ij) + 1.0) - 1.0) / 2.0);
            while (int64_t(ia) * (ia + 1) / 2 > ij) --ia;
            while (int64_t(ia + 1) * (ia + 2) / 2 <= ij) ++ia;
            const int ib = int(ij - int64_t(ia) * (ia + 1) / 2);
            Pair& pr = eng.pairs[ij];
            build_pair(eng.shells[ia], eng.shells[ib], ia, ib, prim_cutoff, eng.hidx, pr);
            if (pr.nprim == 0) continue;
            eng.quartet_cart(pr, pr, blk.data(), rbuf.data(), rtmp.data(), w.data());
            double mx = 0.0;
            for (int a = 0; a < pr.nab; ++a) mx = std::fmax(mx, std::fabs(blk[size_t(a) * pr.nab + a]));
            pr.schwarz = std::sqrt(mx);
        }
    });
    eng.inv_w2 = inv_w2;
}

// the test both engines apply to a canonical quartet (kl <= ij)
inline bool quartet_survives(const Pair& ab, const Pair& cd, double cutoff) {
    return ab.nprim != 0 && cd.nprim != 0 && !(ab.schwarz * cd.schwarz < cutoff);
}

}  // namespace nbx_md
