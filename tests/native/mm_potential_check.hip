// The host engine's MM potential (nbx_host_mm_potential, csrc/ints_host.cpp) on its own: no device, no HIP call, no
// Python.  Built with -fsanitize=address,undefined it checks the pair loop, the Hermite cubes and the thread pool for
// out-of-bounds accesses on a hand-made table of one s, p, d and f shell (two contracted, four centres); the values are
// compared with - q (mu nu | g g), g the normalised s primitive whose square is the Gaussian charge, taken from the
// two-electron engine as tests/test_host_mm_potential.py does for water.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Inbed_amd/csrc \
//         tests/native/mm_potential_check.hip -pthread -o mm_potential_check && ./mm_potential_check
#include <cmath>
#include <cstdio>
#include <vector>

#include "ints_host.cpp"

namespace {

const int ang[] = {0, 1, 2, 3};
const int nprim[] = {2, 2, 1, 1};
const int nfunc[] = {1, 3, 5, 7};
const double centres[] = {0.0, 0.0, 0.0, 0.0, 1.1, -0.3, 0.8, -0.4, 0.6, -0.7, 0.2, 1.2};
const double exps[] = {1.3, 0.4, 0.9, 0.25, 1.1, 0.76};
// contraction coefficients times the radial normalisation (nbed_amd.integrals.Shell of the shells above)
const double coefs[] = {0.5012336067353579, 0.17256249647593527, 0.8763588624785462, 0.1009870784632302, 1.181509448508336,
                        0.5393002015957681};
// s (1 x 1), p (3 x 3), d (5 x 6 over xx xy xz yy yz zz), f (7 x 10 over xxx xxy xxz xyy xyz xzz yyy yyz yzz zzz), normalised
const double sph[] = {
    1.0,
    1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0,
    0.0, 2.8508218814199604, 0.0, 0.0, 0.0, 0.0,
    0.0, 0.0, 0.0, 0.0, 2.8508218814199604, 0.0,
    -0.8229613903247448, 0.0, 0.0, -0.8229613903247448, 0.0, 1.6459227806494896,
    0.0, 0.0, 2.8508218814199604, 0.0, 0.0, 0.0,
    1.4254109407099802, 0.0, 0.0, -1.4254109407099802, 0.0, 0.0,
    0.0, 3.4915294785200173, 0.0, 0.0, 0.0, 0.0, -1.1638431595066725, 0.0, 0.0, 0.0,
    0.0, 0.0, 0.0, 0.0, 5.70164376283992, 0.0, 0.0, 0.0, 0.0, 0.0,
    0.0, -0.9015090348733529, 0.0, 0.0, 0.0, 0.0, -0.9015090348733529, 0.0, 3.6060361394934115, 0.0,
    0.0, 0.0, -2.2082371339486406, 0.0, 0.0, 0.0, 0.0, -2.2082371339486406, 0.0, 1.4721580892990935,
    -0.9015090348733529, 0.0, 0.0, -0.9015090348733529, 0.0, 3.6060361394934115, 0.0, 0.0, 0.0, 0.0,
    0.0, 0.0, 2.8508218814199604, 0.0, 0.0, 0.0, 0.0, -2.8508218814199604, 0.0, 0.0,
    1.1638431595066725, 0.0, 0.0, -3.4915294785200173, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
constexpr int NAO = 16, NSHELL = 4;

// a charge on the s shell's centre (T = 0 on its one-centre pair), one at 60 bohr (asymptotic Boys branch), one general
const double q[] = {0.7, -0.9, 0.4};
const double xyz[] = {0.0, 0.0, 0.0, 0.3, 0.2, 60.0, 1.3, -2.1, 0.7};
const double radii[] = {0.5, 1.0, 0.8};

struct Ref { int i, j; double v; };
// sum over the three charges of - q (i j | g g) from nbx_host_eri with cutoff 0
const Ref REF[] = {{0, 0, -0.9956572916873747},   {2, 0, 0.6059447072116055},      {5, 3, -0.02193792424892907},
                   {7, 1, 0.036441674041028875},  {12, 6, 0.13868016740744016},    {15, 9, -0.0005270547218621096},
                   {10, 10, -0.5141829141445486}};
// ten times the largest difference between the host engine and this oracle on water / cc-pVDZ (1.4e-15,
// tests/test_host_mm_potential.py); on this table the difference is 2.3e-16
constexpr double TOL = 1.4e-14;

int call(int ncharge, const double* zeta, int nthreads, std::vector<double>& v) {
    v.assign(size_t(NAO) * NAO, std::nan(""));
    return nbx_host_mm_potential(NSHELL, ang, nprim, nfunc, centres, exps, coefs, sph, ncharge, q, xyz, zeta, nthreads, v.data());
}

}  // namespace

int main() {
    double zeta[3];
    for (int c = 0; c < 3; ++c) zeta[c] = 1.0 / (radii[c] * radii[c]);
    std::vector<double> v, w;
    int bad = call(3, zeta, 3, v) != NBX_OK;
    for (const Ref& r : REF)
        if (!(std::fabs(v[size_t(r.i) * NAO + r.j] - r.v) <= TOL)) {
            std::printf("V[%d][%d] = %.17g, expected %.17g\n", r.i, r.j, v[size_t(r.i) * NAO + r.j], r.v);
            ++bad;
        }
    std::printf("values bad=%d\n", bad);

    bad = 0;  // exactly symmetric, every element written, the same bits on one thread
    for (int i = 0; i < NAO; ++i)
        for (int j = 0; j < NAO; ++j) bad += !(v[size_t(i) * NAO + j] == v[size_t(j) * NAO + i]);
    bad += call(3, zeta, 1, w) != NBX_OK;
    for (size_t k = 0; k < v.size(); ++k) bad += !(v[k] == w[k]);
    std::printf("symmetry and threads bad=%d\n", bad);

    bad = call(0, nullptr, 2, w) != NBX_OK;  // no charges: exact zeros
    for (double x : w) bad += !(x == 0.0);
    std::printf("no charges bad=%d\n", bad);

    bad = call(3, nullptr, 2, w) != NBX_OK;  // point charges: the limit of small radii
    double tiny[3] = {1e12, 1e12, 1e12};
    bad += call(3, tiny, 2, v) != NBX_OK;
    for (size_t k = 0; k < v.size(); ++k) bad += !(std::fabs(v[k] - w[k]) <= 1e-9);
    std::printf("point charges bad=%d\n", bad);

    bad = 0;  // refusals write nothing
    double neg[3] = {4.0, -1.0, 1.0};
    bad += call(3, neg, 1, w) != NBX_E_INVALID;
    bad += call(-1, nullptr, 1, w) != NBX_E_INVALID;
    const int ang_g[] = {0, 1, 2, 4};
    w.assign(size_t(NAO) * NAO, 0.0);
    bad += nbx_host_mm_potential(NSHELL, ang_g, nprim, nfunc, centres, exps, coefs, sph, 3, q, xyz, zeta, 1, w.data()) != NBX_E_INVALID;
    std::printf("refusals bad=%d\n", bad);
    return 0;
}
