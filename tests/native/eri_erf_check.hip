// The host engine's attenuated two-electron integrals (nbx_host_eri_erf, csrc/ints_host.cpp) on their own: no device, no
// HIP call, no Python.  Built with -fsanitize=address,undefined it checks the quartet loop, the Hermite cubes and the
// thread pool for out-of-bounds accesses on the hand-made table of tests/native/mm_potential_check.hip (one s, p, d and f
// shell, two contracted, four centres).  The values are checked through an identity: the ket (ss| of the contracted s
// shell is a sum of Gaussian charges c_i c_j (pi / zeta_ij)^(3/2), zeta_ij = a_i + a_j, on the shell's centre, and under
// erf(omega r12) / r12 each acts like a Gaussian charge of radius sqrt(1 / omega^2 + 1 / zeta_ij) under 1 / r12 -- what
// nbx_host_mm_potential computes without the quartet code.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Inbed_amd/csrc \
//         tests/native/eri_erf_check.hip -pthread -o eri_erf_check && ./eri_erf_check
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
constexpr size_t N2 = size_t(NAO) * NAO, N4 = N2 * N2;
// the bound tests/test_host_mm_potential.py holds between two engines, per unit of charge
constexpr double TOL = 1.4e-14;

int call(double omega, int nthreads, double cutoff, std::vector<double>& v) {
    v.assign(N4, std::nan(""));
    return nbx_host_eri_erf(NSHELL, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff, omega, nthreads, v.data());
}

}  // namespace

int main() {
    std::vector<double> v, w, plain(N4), pot(N2);
    int bad = nbx_host_eri(NSHELL, ang, nprim, nfunc, centres, exps, coefs, sph, 0.0, 3, plain.data()) != NBX_OK;
    double top = 0.0;
    for (double x : plain) top = std::fmax(top, std::fabs(x));

    for (double omega : {1e-3, 0.33, 1e3}) {  // (ab|ss)_omega against the potential of the ket's Gaussian charges
        bad += call(omega, 3, 0.0, v) != NBX_OK;
        double q[4], xyz[12], zeta[4], qsum = 0.0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                const int c = 2 * i + j;
                const double z = exps[i] + exps[j];
                q[c] = coefs[i] * coefs[j] * std::pow(M_PI / z, 1.5);
                zeta[c] = 1.0 / (1.0 / (omega * omega) + 1.0 / z);
                for (int d = 0; d < 3; ++d) xyz[3 * c + d] = centres[d];
                qsum += std::fabs(q[c]);
            }
        bad += nbx_host_mm_potential(NSHELL, ang, nprim, nfunc, centres, exps, coefs, sph, 4, q, xyz, zeta, 2, pot.data()) != NBX_OK;
        for (int a = 0; a < NAO; ++a)
            for (int b = 0; b < NAO; ++b) {
                const double got = v[(size_t(a) * NAO + b) * N2], want = -pot[size_t(a) * NAO + b];
                if (!(std::fabs(got - want) <= TOL * qsum)) {
                    std::printf("omega %g: (%d %d|0 0) = %.17g, expected %.17g\n", omega, a, b, got, want);
                    ++bad;
                }
            }
        for (int a = 0; a < NAO; ++a)  // 0 <= (ab|ab)_omega <= (ab|ab), to rounding: the plain Schwarz bounds hold
            for (int b = 0; b < NAO; ++b) {
                const size_t k = (size_t(a) * NAO + b) * N2 + size_t(a) * NAO + b;
                bad += !(v[k] >= -1e-15 * top && v[k] <= plain[k] + 1e-15 * top);
            }
    }
    std::printf("values bad=%d\n", bad);

    bad = call(0.33, 3, 1e-16, v) != NBX_OK;  // the eight images are one double, every element written, threads change nothing
    for (int a = 0; a < NAO; ++a)
        for (int b = 0; b < NAO; ++b)
            for (int c = 0; c < NAO; ++c)
                for (int d = 0; d < NAO; ++d) {
                    const double x = v[((size_t(a) * NAO + b) * NAO + c) * NAO + d];
                    bad += !(x == v[((size_t(b) * NAO + a) * NAO + c) * NAO + d]);
                    bad += !(x == v[((size_t(a) * NAO + b) * NAO + d) * NAO + c]);
                    bad += !(x == v[((size_t(c) * NAO + d) * NAO + a) * NAO + b]);
                }
    bad += call(0.33, 1, 1e-16, w) != NBX_OK;
    for (size_t k = 0; k < N4; ++k) bad += !(v[k] == w[k]);
    std::printf("symmetry and threads bad=%d\n", bad);

    bad = call(1e6, 2, 0.0, v) != NBX_OK;  // omega -> infinity: the plain tensor (exponents <= 1.3: 1e-12 relative)
    for (size_t k = 0; k < N4; ++k) bad += !(std::fabs(v[k] - plain[k]) <= 1e-8 * top);
    std::printf("large omega bad=%d\n", bad);

    // a coarse cutoff: the quartets the plain tensor skips (zero there, not zero without the cutoff) are skipped here too
    // and left as exact zeros; every element is written
    bad = call(0.33, 2, 0.1, v) != NBX_OK;
    bad += nbx_host_eri(NSHELL, ang, nprim, nfunc, centres, exps, coefs, sph, 0.1, 2, w.data()) != NBX_OK;
    size_t skipped = 0;
    for (size_t k = 0; k < N4; ++k) {
        bad += !std::isfinite(v[k]);
        if (w[k] == 0.0 && plain[k] != 0.0) {
            bad += !(v[k] == 0.0);
            ++skipped;
        }
    }
    bad += skipped == 0;
    std::printf("screening bad=%d\n", bad);

    bad = 0;  // refusals write nothing
    w.assign(N4, 3.0);
    for (double omega : {0.0, -0.33, double(INFINITY), double(NAN)})
        bad += nbx_host_eri_erf(NSHELL, ang, nprim, nfunc, centres, exps, coefs, sph, 1e-16, omega, 1, w.data()) != NBX_E_INVALID;
    const int ang_g[] = {0, 1, 2, 4};
    bad += nbx_host_eri_erf(NSHELL, ang_g, nprim, nfunc, centres, exps, coefs, sph, 1e-16, 0.33, 1, w.data()) != NBX_E_INVALID;
    for (double x : w) bad += !(x == 3.0);
    std::printf("refusals bad=%d\n", bad);
    return 0;
}
