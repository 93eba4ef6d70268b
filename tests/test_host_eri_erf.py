"""The attenuated two-electron integrals (pq| erf(omega r12) / r12 |rs) of the host engine (nbx_host_eri_erf,
csrc/ints_host.cpp on csrc/ints_md.h) -- the long-range integrals of a range-separated hybrid -- against
tests/eri_erf_reference.py (the oracle's scalar recursions with the substitution derived there, and the s-type closed form
in mpmath at 50 digits), against the MM-potential engine through an identity that shares no code with either, in the limit
omega -> infinity, and in a stand-alone program under the sanitizers.  No GPU."""

import ctypes
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import eri_erf_reference as er
from nbed_amd import _nbx, integrals

OMEGAS = (1e-3, 0.33, 1e3)
# s, p, d and f shells on two centres, the p shell contracted: the table of
# tests/test_host_integrals.py::test_f_shell_integrals_match_the_oracle_engine, and its bound between the host engine and
# the oracle engine
SPDF_TABLE = {"C": [(1, (0.38, 0.9), (0.7, 0.4)), (2, (1.097,), (1.0,)), (3, (0.761,), (1.0,))],
              "H": [(0, (0.3,), (1.0,)), (2, (1.057,), (1.0,)), (3, (0.9,), (1.0,))]}
SPDF_XYZ = "2\n\nC 0.1 -0.2 0.3\nH 0.9 0.5 -0.4"
ORACLE_ATOL = 1e-13
# the bound of tests/test_host_mm_potential.py between two engines, per unit of charge
MM_TOL = 1.4e-14


def _spdf():
    bs = integrals.Basis(integrals.parse_geometry(SPDF_XYZ), SPDF_TABLE)
    ob = er.SphericalBasis(er.parse_xyz(SPDF_XYZ), SPDF_TABLE)
    assert bs.nao == ob.nao == 28 and integrals.max_ang(bs) == 3
    return bs, ob


@pytest.fixture(scope="module")
def spdf_plain():
    return integrals.two_electron_native(_spdf()[0])


def test_the_omega_keyword_exists_and_is_checked():
    bs = integrals.Basis(integrals.parse_geometry("2\n\nH 0 0 0\nH 0 0 0.74"), "sto-3g")
    got = integrals.eri_native(bs, omega=0.33)
    assert got.shape == (2, 2, 2, 2) and 0.0 < got[0, 0, 0, 0] < integrals.eri_native(bs)[0, 0, 0, 0]
    np.testing.assert_array_equal(got, integrals.two_electron_native(bs, omega=0.33))
    for bad in (0.0, -0.33, math.inf, math.nan):
        with pytest.raises(ValueError, match="omega"):
            integrals.two_electron_native(bs, omega=bad)
    # the C entry point refuses them too, and writes nothing
    lib = _nbx.load_library()
    arrays = integrals._shell_arrays(bs)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = np.full((2,) * 4, 7.0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert lib.nbx_host_eri_erf(len(bs.shells), *(ptr(a) for a in arrays), 1e-16, bad, 1, ptr(out)) == _nbx.NBX_E_INVALID
    assert np.all(out == 7.0)


def test_s_closed_form_quadrature_and_engine_agree():
    """Four s primitives on four centres.  The closed form (alpha_w in F_0, the factor omega / sqrt(alpha + omega^2)) against
    the u integral it was derived from, both at 50 digits: they must agree to ~45; then the reference's primitive and the
    host engine (normalised s shells, N = (2 a / pi)^(3/4)) against the closed form."""
    import mpmath as mp

    exps = (0.7, 1.3, 0.4, 2.1)
    xyz = "4\n\nH 0 0 0\nC 0.5 0.2 -0.3\nN 1.0 -0.7 0.4\nO -0.2 0.9 0.6"
    atoms = integrals.parse_geometry(xyz)
    centres = [pos for _, pos in atoms]
    table = {sym: [(0, (a,), (1.0,))] for (sym, _), a in zip(atoms, exps)}
    bs = integrals.Basis(atoms, table)
    norm = math.prod((2.0 * a / math.pi) ** 0.75 for a in exps)
    zero = (0, 0, 0)
    for omega in OMEGAS + (1e6,):
        exact = er.ssss_closed_form(exps, centres, omega)
        assert abs(er.ssss_quadrature(exps, centres, omega) - exact) <= mp.mpf("1e-45") * exact
        prim = er.eri_erf_prim(exps[0], zero, centres[0], exps[1], zero, centres[1], exps[2], zero, centres[2], exps[3], zero,
                               centres[3], omega)
        got = integrals.two_electron_native(bs, omega=omega, cutoff=0.0)[0, 1, 2, 3]
        rel_ref, rel_got = (float(abs(mp.mpf(v) - w) / w) for v, w in ((prim, exact), (got, norm * exact)))
        print(f"omega = {omega:g}: closed form {float(exact):.6e}; reference {rel_ref:.1e}, host engine {rel_got:.1e} relative")
        assert rel_ref <= 8 * 2.0**-52 and rel_got <= 16 * 2.0**-52
    # omega -> infinity: the value no longer moves
    assert abs(er.ssss_closed_form(exps, centres, 1e30) / er.ssss_closed_form(exps, centres, 1e29) - 1) < mp.mpf("1e-40")


@pytest.mark.parametrize("omega", OMEGAS)
def test_host_engine_against_the_reference_on_s_p_d_f_shells(omega, spdf_plain):
    """Sampled elements of the 28-function s-p-d-f table (the reference is scalar Python: 45 elements are what a few
    seconds buy, as in test_f_shell_integrals_match_the_oracle_engine), every shell type in the sample, at the absolute
    bound that test holds for the plain tensor (1e-13, tensor scale 0.81).

    At omega = 1e-3 the whole tensor is 1.1e-3, so 1e-13 would be a loose test: there the bound is scaled with the tensor,
    1e-13 * max|eri_omega| / max|eri| = 1.4e-16.  The reference's own 53-bit error on values of that size, measured against
    the 50-digit closed form in test_s_closed_form_quadrature_and_engine_agree, is 4.8e-16 relative = 5e-19 absolute;
    measured host-engine differences: 1.6e-21 (omega = 1e-3), 5.4e-19 (0.33), 5.9e-18 (1e3)."""
    bs, ob = _spdf()
    eri = integrals.two_electron_native(bs, omega=omega)
    np.testing.assert_array_equal(eri, eri.transpose(1, 0, 3, 2))
    np.testing.assert_array_equal(eri, eri.transpose(2, 3, 0, 1))
    atol = ORACLE_ATOL * min(1.0, np.abs(eri).max() / np.abs(spdf_plain).max())
    rng = np.random.default_rng(1)
    picks = [(0, 0, 0, 0), (3, 3, 8, 8), (8, 0, 8, 0), (9, 2, 20, 5), (27, 27, 27, 27), (21, 1, 14, 9), (16, 16, 3, 3)]
    picks += [tuple(int(x) for x in rng.integers(0, bs.nao, 4)) for _ in range(38)]
    worst, nonzero = 0.0, 0
    for p, q, r, s in picks:
        ref = er.eri_erf_element(ob, p, q, r, s, omega)
        worst = max(worst, abs(ref - eri[p, q, r, s]))
        nonzero += abs(ref) > 1e-6 * np.abs(eri).max()
    print(f"omega = {omega:g}: worst |host - reference| {worst:.2e} of {len(picks)} elements, bound {atol:.2e}")
    # (at omega = 1e-3 only the charge-charge term ~ omega S_pq S_rs is not suppressed by powers of omega: fewer elements count)
    assert nonzero >= 12 and worst <= atol


@pytest.mark.parametrize("omega", OMEGAS)
def test_ket_of_two_s_primitives_is_a_gaussian_mm_charge(omega):
    """For a ket of two s primitives on one centre C with exponents summing to zeta, the ket density is a Gaussian charge
    S_cd (zeta / pi)^(3/2) exp(-zeta r^2), and its potential under erf(omega r12) / r12 is that of a unit Gaussian charge of
    radius sqrt(1 / omega^2 + 1 / zeta) under 1 / r12: (ab|cd)_omega = - S_cd V_mm[a, b].  nbx_host_mm_potential shares the
    Boys table and R recursion with the two-electron engine, not the quartet code; bra shells up to d on two centres."""
    table = {"O": [(0, (1.1,), (1.0,)), (1, (0.8, 0.3), (0.6, 0.5)), (2, (0.9,), (1.0,))],
             "C": [(0, (0.45,), (1.0,)), (1, (1.4,), (1.0,)), (2, (0.6, 1.8), (0.7, 0.4))],
             "H": [(0, (0.7,), (1.0,)), (0, (1.9,), (1.0,))]}
    bs = integrals.Basis(integrals.parse_geometry("3\n\nO 0.1 -0.2 0.3\nC 1.0 0.6 -0.5\nH -0.4 0.9 1.1"), table)
    n = bs.nao
    assert n == 20 and [sh.ang for sh in bs.shells] == [0, 1, 2, 0, 1, 2, 0, 0]
    eri = integrals.two_electron_native(bs, omega=omega, cutoff=0.0)
    s_mat = integrals.one_electron_native(bs)[0]
    centre = bs.shells[-1].centre
    for c, d in ((n - 2, n - 2), (n - 1, n - 2), (n - 1, n - 1)):
        zeta = float(bs.shells[c - n].exps[0] + bs.shells[d - n].exps[0])
        v = integrals.mm_potential_native(bs, [centre], [1.0], [math.sqrt(1.0 / omega**2 + 1.0 / zeta)])
        diff = np.abs(eri[:, :, c, d] + s_mat[c, d] * v).max()
        print(f"omega = {omega:g}, ket ({c}, {d}): {diff:.2e} (max |(ab|cd)| {np.abs(eri[:, :, c, d]).max():.3e})")
        assert diff <= MM_TOL


def test_large_omega_is_the_plain_tensor(spdf_plain):
    """alpha_w = alpha / (1 + alpha / omega^2): at omega = 1e6 and exponents <= 1e3 the change is below 1e-9 relative."""
    bs, _ = _spdf()
    got = integrals.two_electron_native(bs, omega=1e6)
    assert np.abs(got - spdf_plain).max() <= 1e-8 * np.abs(spdf_plain).max()
    tight = integrals.Basis(integrals.parse_geometry("2\n\nO 0 0 0\nH 0 0 0.9"),
                            {"O": [(0, (1e3, 30.0), (0.3, 0.8)), (1, (900.0, 2.0), (0.2, 0.9))], "H": [(0, (0.5,), (1.0,))]})
    plain = integrals.two_electron_native(tight)
    got = integrals.two_electron_native(tight, omega=1e6)
    rel = np.abs(got - plain).max() / np.abs(plain).max()
    print(f"exponents up to 1e3, omega = 1e6: {rel:.2e} relative")
    assert 0.0 < rel <= 1e-8


def test_screening_and_threads():
    """The attenuated tensor skips the plain tensor's quartets (its Schwarz bounds hold for erf(omega r12) / r12 too): what
    is screened at 1e-6 is an exact zero in both, everything else is written; the thread count does not change a bit."""
    bs = integrals.Basis(integrals.parse_geometry("2\n\nH 0 0 0\nH 0 0 12.0"), "cc-pvdz")
    full = integrals.two_electron_native(bs, omega=0.33, cutoff=0.0)
    cut = integrals.two_electron_native(bs, omega=0.33, cutoff=1e-6)
    plain_cut = integrals.two_electron_native(bs, cutoff=1e-6)
    assert np.array_equal(cut == 0.0, plain_cut == 0.0) and (cut == 0.0).sum() > (full == 0.0).sum()
    kept = cut != 0.0
    np.testing.assert_array_equal(cut[kept], full[kept])
    assert np.abs(full[~kept]).max() < 1e-6  # (pq|rs)_omega <= sqrt((pq|pq) (rs|rs)): the plain bound holds
    np.testing.assert_array_equal(cut, integrals.two_electron_native(bs, omega=0.33, cutoff=1e-6, nthreads=1))


def test_host_engine_under_the_sanitizers(tmp_path):
    """nbx_host_eri_erf in a stand-alone program built with AddressSanitizer and UBSan (tests/native/eri_erf_check.hip):
    s, p, d and f shells, no device, no Python, no preloaded library."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.fail("no hipcc: the library this suite tests cannot have been built without it")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "eri_erf_check"
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", f"-I{root / 'include'}", f"-I{root / 'nbed_amd' / 'csrc'}",
                    str(root / "tests" / "native" / "eri_erf_check.hip"), "-pthread", "-o", str(exe)], check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("bad=0") == 5, r.stdout
