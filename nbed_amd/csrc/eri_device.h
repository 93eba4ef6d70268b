// What eri.hip (the class kernel and its three sinks) offers to eri_cd.hip (the pivoted Cholesky decomposition): one
// molecule's pair data, Boys table and index tables uploaded once, then any number of diagonal / column launches on it.
// mm_potential.hip (the potential of MM charges) runs its own kernels on the same session and Boys evaluation.
#pragma once

#include "ints_md.h"
#include "nbx_common.h"

namespace nbx_eri {

struct DevShell { int l, ncart, nsph, ao0; long long sph_off; };
struct DevPair { int ia, ib, nab, nprim; long long prim_off, h_off; };

// Function pairs (r >= s) of the shell pair (ia >= ib): the columns the column sink writes for it, (r, s) row-major.
inline int pair_columns(const nbx_md::Engine& eng, const nbx_md::Pair& pr) {
    const int na = eng.shells[pr.ia].nsph, nb = eng.shells[pr.ib].nsph;
    return pr.ia == pr.ib ? na * (na + 1) / 2 : na * nb;
}

// The host bookkeeping of one column call (no device, no HIP: tests/native/eri_cd_lists_check.hip runs it under the
// sanitizers).  For every selected shell pair kl and every bra pair ij, the canonical quartet (max, min) that passes the
// dense engine's Schwarz test, sorted into the classes (l_hi, l_lo); aux = (first column of kl, 1 if kl is the bra).
struct ColumnLists {
    int64_t counts[25] = {};
    std::vector<uint2> quartets, aux;  // class after class
    std::vector<int> col_pq;           // p * nao + q (q <= p) of every column
    int64_t ncols = 0;
};
inline void build_column_lists(const nbx_md::Engine& eng, int npair, const int64_t* sel, double cutoff, ColumnLists& out) {
    constexpr int NLP = 5;
    const int64_t np = int64_t(eng.pairs.size());
    std::vector<int64_t> m0(size_t(npair > 0 ? npair : 0));
    for (int64_t& c : out.counts) c = 0;
    out.col_pq.clear();
    out.ncols = 0;
    for (int k = 0; k < npair; ++k) {
        const nbx_md::Pair& pr = eng.pairs[size_t(sel[k])];
        const nbx_md::Shell &sa = eng.shells[pr.ia], &sb = eng.shells[pr.ib];
        m0[k] = out.ncols;
        for (int a = 0; a < sa.nsph; ++a)
            for (int b = 0; b < (pr.ia == pr.ib ? a + 1 : sb.nsph); ++b) out.col_pq.push_back((sa.ao0 + a) * eng.nao + sb.ao0 + b);
        out.ncols += pair_columns(eng, pr);
    }
    auto each = [&](auto&& fn) {
        for (int k = 0; k < npair; ++k)
            for (int64_t ij = 0; ij < np; ++ij) {
                const int64_t hi = ij > sel[k] ? ij : sel[k], lo = ij > sel[k] ? sel[k] : ij;
                const nbx_md::Pair &ab = eng.pairs[size_t(hi)], &cd = eng.pairs[size_t(lo)];
                if (nbx_md::quartet_survives(ab, cd, cutoff)) fn(ab.lab * NLP + cd.lab, hi, lo, m0[k], ij < sel[k] ? 1u : 0u);
            }
    };
    each([&](int cls, int64_t, int64_t, int64_t, unsigned) { ++out.counts[cls]; });
    int64_t fill[25], total = 0;
    for (int c = 0; c < 25; ++c) { fill[c] = total; total += out.counts[c]; }
    out.quartets.resize(size_t(total));
    out.aux.resize(size_t(total));
    each([&](int cls, int64_t hi, int64_t lo, int64_t first, unsigned bra) {
        out.quartets[size_t(fill[cls])] = make_uint2(unsigned(hi), unsigned(lo));
        out.aux[size_t(fill[cls]++)] = make_uint2(unsigned(first), bra);
    });
}

struct EriArgs {
    const DevShell* shells;
    const DevPair* pairs;
    const double* prim;   // (p, Px, Py, Pz) per surviving primitive pair
    const double* h;      // Hermite densities [prim][nab][nh]
    const double* sph;
    const double* boys;   // BoysTable::f
    const int* tabs;      // NLP x NH_MAX packed (t, u, v) in HermIndex order, then NR_MAX sorted by t + u + v
    double* out;          // the sink's buffer: (nao)^4 tensor, (nao, nao) diagonal or (ncols, nao, nao) columns
    double pref0;         // 2 pi^(5/2)
    double inv_w2;        // Engine::inv_w2: 1 / omega^2 of erf(omega r12) / r12, 0 for 1 / r12
    int nao;
};

// BoysTable::eval on the device (tab = BoysTable::f): F_0 .. F_L at t.  Shared by eri.hip and mm_potential.hip.
template <int L>
__device__ __forceinline__ void boys_eval(const double* __restrict__ tab, double t, double* out) {
    using nbx_md::BoysTable;
    if (t >= BoysTable::TMAX - 1.0) {
        const double et = exp(-t);
        out[0] = 0.5 * sqrt(M_PI / t);
#pragma unroll
        for (int m = 0; m < L; ++m) out[m + 1] = ((2 * m + 1) * out[m] - et) / (2.0 * t);
        return;
    }
    const int i = int(t / BoysTable::STEP + 0.5);
    const double d = i * BoysTable::STEP - t;
    const double* row = tab + size_t(i) * (BoysTable::NORD + 1);
    double acc = 0.0, pw = 1.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        acc += row[L + k] * pw;
        pw *= d / (k + 1);
    }
    out[L] = acc;
    const double et = exp(-t);
#pragma unroll
    for (int m = L; m > 0; --m) out[m - 1] = (2.0 * t * out[m] + et) / (2 * m - 1);
}

struct Session {
    nbx_md::Engine eng;
    hipStream_t stream = nullptr;
    double cutoff = 0.0;
    char* d_img = nullptr;
    EriArgs args = {};  // (out is set per launch)
    ColumnLists lists;  // host image of the last column call's lists: alive until the stream has copied them
};

// NBX_E_INVALID where nbx_eri_device refuses the shells (no message set); returns once the upload has left host memory
int session_open(nbx_ctx* ctx, int nshell, const int* ang, const int* nprim, const int* nfunc, const double* centres,
                 const double* exps, const double* coefs, const double* sph, double cutoff, Session& s);
void session_close(Session& s);
// d_diag (nao, nao): zeroed, then d[p][q] = d[q][p] = (pq|pq) of every surviving shell pair
int session_diagonal(Session& s, double* d_diag);
// d_cols (ncols, nao, nao): zeroed, then the columns of the shell pairs sel[0 .. npair).  If d_col_pq is given, ncols ints
// p * nao + q of the columns are left there.  The lists are copied from s.lists asynchronously: synchronise the stream
// before the next session_columns or session_close.
int session_columns(Session& s, int npair, const int64_t* sel, double* d_cols, int* d_col_pq);

}  // namespace nbx_eri
