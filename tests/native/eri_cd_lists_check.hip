// Host bookkeeping of the column sink's launches (nbx_eri::build_column_lists, csrc/eri_device.h) on its own: no device,
// no HIP call.  Built with -fsanitize=address,undefined it checks the list construction for out-of-bounds writes; the
// invariants below hold for every selection of shell pairs:
//   * the class counts add up to the list length, and every entry sits in the class (l_hi, l_lo) of its pairs;
//   * an entry is canonical (hi >= lo), names one selected pair (as the ket, or as the bra when flagged) and passes the
//     dense engine's Schwarz test; every (selected pair, bra pair) that passes is listed exactly once;
//   * aux.x is the first column of the selected pair, the columns are (r >= s) row-major, p * nao + q with q <= p.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Inbed_amd/csrc \
//       tests/native/eri_cd_lists_check.hip -pthread -o eri_cd_lists_check
#include <cstdio>
#include <map>
#include <set>

#include "eri_device.h"

using namespace nbx_md;

void nbx_set_error(const char*, ...) {}

static int check(const Engine& eng, const std::vector<int64_t>& sel, double cutoff) {
    nbx_eri::ColumnLists l;
    nbx_eri::build_column_lists(eng, int(sel.size()), sel.data(), cutoff, l);
    int bad = 0;
    int64_t total = 0;
    for (int64_t c : l.counts) total += c;
    bad += total != int64_t(l.quartets.size()) || l.aux.size() != l.quartets.size();
    std::vector<int64_t> first(sel.size());
    int64_t ncols = 0;
    for (size_t k = 0; k < sel.size(); ++k) {
        first[k] = ncols;
        ncols += nbx_eri::pair_columns(eng, eng.pairs[size_t(sel[k])]);
    }
    bad += ncols != l.ncols || int64_t(l.col_pq.size()) != ncols;
    for (int pq : l.col_pq) bad += pq < 0 || pq >= eng.nao * eng.nao || pq % eng.nao > pq / eng.nao;
    std::map<std::pair<int64_t, int64_t>, int> seen;  // (slot of the selected pair, other pair) -> times listed
    int64_t at = 0;
    for (int cls = 0; cls < 25; ++cls)
        for (int64_t i = 0; i < l.counts[cls]; ++i, ++at) {
            const uint2 q = l.quartets[size_t(at)], a = l.aux[size_t(at)];
            bad += q.x < q.y || q.x >= eng.pairs.size();
            const Pair &hi = eng.pairs[q.x], &lo = eng.pairs[q.y];
            bad += hi.lab * 5 + lo.lab != cls || !quartet_survives(hi, lo, cutoff);
            const int64_t mine = a.y ? q.x : q.y, other = a.y ? q.y : q.x;
            bad += a.y && q.x == q.y;  // the diagonal quartet is listed once, as the ket
            int hit = 0;
            for (size_t k = 0; k < sel.size(); ++k)
                if (sel[k] == mine && first[k] == int64_t(a.x)) { ++seen[{int64_t(k), other}]; ++hit; }
            bad += hit != 1;
        }
    for (size_t k = 0; k < sel.size(); ++k)
        for (int64_t ij = 0; ij < int64_t(eng.pairs.size()); ++ij) {
            const int64_t hi = std::max(ij, sel[k]), lo = std::min(ij, sel[k]);
            const int want = quartet_survives(eng.pairs[size_t(hi)], eng.pairs[size_t(lo)], cutoff) ? 1 : 0;
            const auto it = seen.find({int64_t(k), ij});
            bad += (it == seen.end() ? 0 : it->second) != want;
        }
    std::printf("pairs selected %zu: %lld quartets, %lld columns, bad=%d\n", sel.size(), (long long)total, (long long)ncols, bad);
    return bad;
}

int main() {
    // two centres 12 bohr apart (pairs across them are screened out), s, p and d shells, a Cartesian d among them
    const int nshell = 6;
    const int ang[nshell] = {0, 1, 2, 0, 2, 1}, nprim[nshell] = {2, 1, 1, 1, 1, 1}, nfunc[nshell] = {1, 3, 5, 1, 6, 3};
    const double centres[3 * nshell] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 12, 0, 0, 12, 0, 0, 12};
    const double exps[7] = {3.4, 0.6, 0.9, 1.1, 0.5, 1.3, 0.8}, coefs[7] = {0.4, 0.7, 1.0, 1.0, 1.0, 1.0, 1.0};
    std::vector<double> sph;
    for (int s = 0; s < nshell; ++s)
        for (int i = 0; i < nfunc[s] * ncart(ang[s]); ++i) sph.push_back(i % (ncart(ang[s]) + 1) == 0 ? 1.0 : 0.25);
    Engine eng;
    eng.cutoff = 1e-16;
    if (engine_shells(eng, nshell, ang, nprim, nfunc, centres, exps, coefs, sph.data(), 2) != NBX_OK) return 2;
    engine_tables(eng);
    engine_pairs(eng, 2);
    const int64_t np = int64_t(eng.pairs.size());
    int bad = 0;
    std::vector<int64_t> all;
    for (int64_t k = 0; k < np; ++k) all.push_back(k);
    bad += check(eng, all, 1e-16);
    bad += check(eng, {}, 1e-16);
    bad += check(eng, {np - 1}, 1e-16);
    bad += check(eng, {5, 0, 5, 17, 2}, 1e-16);  // scrambled, one pair twice
    bad += check(eng, {20, 9, 14}, 1e-6);
    std::printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
