"""The potential of an MM environment (QM/MM) on the host: ``integrals.mm_potential`` (numpy), ``mm_potential_native``
(nbx_host_mm_potential, csrc/ints_host.cpp), the nuclei-MM energy, the unit handling, and ``nbed(config)`` on the built-in
provider with ``mm_coords`` / ``mm_charges`` / ``mm_radii`` set.

The semantics -- Gaussian charges of exponent 1 / radius^2 in the core Hamiltonian, plain point charges in
``energy_nuc()``, coordinates and radii in the geometry's unit -- restate PySCF's ``qmmm.mm_charge``; no PySCF literal
pins them here.  What IS pinned: the closed form for s functions in 30 digits, and for every angular momentum the
identity V_c[mu nu] = - q (mu nu | g g), g the normalised s primitive of exponent zeta / 2 at the charge (g^2 is the
normalised Gaussian charge), with (mu nu | g g) from the two-electron engine, which shares no code path with the
one-electron sums but the Boys table."""

import ctypes
import shutil
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

from oracle_backend import OracleBackend

from nbed_amd import NbedConfig, _nbx, integrals, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.exceptions import NbedDriverError

WATER_XYZ = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
H2_XYZ = "2\n\nH 0.0 0.0 0.0\nH 0.0 0.0 0.74"

# The largest |engine - oracle| over the three charges of test_every_pair_order_against_the_two_electron_engine, as
# measured when the test was written: 1.33e-15 (host engine; numpy 5.6e-16; values up to 1.48).  The
# two sides share no summation order.  Every comparison of two engines below allows ten times that per unit of sum |q|.
ORACLE_DIFF = 1.4e-15
TOL = 10 * ORACLE_DIFF


def _basis(xyz, name):
    return integrals.Basis(integrals.parse_geometry(xyz), name)


def _oracle(bs, pos, q, radius):
    """- q (mu nu | g g) from nbx_host_eri, nothing screened."""
    g = integrals.Shell(pos, 0, [0.5 / radius**2], [1.0])
    ext = types.SimpleNamespace(shells=bs.shells + [g], nao=bs.nao + 1)
    n = bs.nao
    return -q * integrals.two_electron_native(ext, cutoff=0.0)[:n, :n, n, n]


def _host_1e_v(bs, coords, charges):
    """V of nbx_host_1e with the charges passed as its atoms."""
    lib = _nbx.load_library()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    arrays = integrals._shell_arrays(bs)
    xyz = np.ascontiguousarray(coords, dtype=np.float64)
    q = np.ascontiguousarray(charges, dtype=np.float64)
    out = [np.empty((bs.nao, bs.nao)) for _ in range(3)]
    _nbx.check(lib, lib.nbx_host_1e(len(bs.shells), *(ptr(a) for a in arrays), len(q), ptr(q), ptr(xyz), 0, *(ptr(o) for o in out)))
    return out[2]


def test_s_functions_against_the_closed_form_in_30_digits():
    """H2 / STO-3G, three charges of different radii: V = - sum_c q_c sum_ij w_i w_j (2 pi / p) sqrt(zeta / (p + zeta))
    exp(-mu R_AB^2) F_0(rho |PC|^2), F_0(x) = sqrt(pi / x) erf(sqrt x) / 2, evaluated with mpmath."""
    import mpmath as mp

    mp.mp.dps = 30
    bs = _basis(H2_XYZ, "sto-3g")
    coords = np.array([[0.9, -0.4, 0.3], [0.0, 0.0, 2.5], [-1.7, 1.1, -0.6]])
    charges, radii = np.array([0.8, -0.45, 1.1]), np.array([0.3, 1.0, 2.2])

    def f0(x):
        return mp.mpf(1) if x == 0 else mp.sqrt(mp.pi / x) * mp.erf(mp.sqrt(x)) / 2

    ref = np.zeros((2, 2))
    for i, sa in enumerate(bs.shells):
        for j, sb in enumerate(bs.shells):
            acc = mp.mpf(0)
            ra, rb = [mp.mpf(float(x)) for x in sa.centre], [mp.mpf(float(x)) for x in sb.centre]
            r2 = sum((x - y) ** 2 for x, y in zip(ra, rb))
            for a, wa in zip(sa.exps, sa.coefs[0]):
                for b, wb in zip(sb.exps, sb.coefs[0]):
                    a_, b_ = mp.mpf(float(a)), mp.mpf(float(b))
                    p = a_ + b_
                    centre = [(a_ * x + b_ * y) / p for x, y in zip(ra, rb)]
                    for pos, q, rad in zip(coords, charges, radii):
                        zeta = 1 / mp.mpf(float(rad)) ** 2
                        pc2 = sum((x - mp.mpf(float(y))) ** 2 for x, y in zip(centre, pos))
                        acc -= (mp.mpf(float(q)) * mp.mpf(float(wa)) * mp.mpf(float(wb)) * 2 * mp.pi / p * mp.sqrt(zeta / (p + zeta))
                                * mp.exp(-a_ * b_ / p * r2) * f0(p * zeta / (p + zeta) * pc2))
            ref[i, j] = float(acc)
    assert np.abs(ref).max() > 0.5  # values of order one
    for name, got in (("numpy", integrals.mm_potential(bs, coords, charges, radii)),
                      ("native", integrals.mm_potential_native(bs, coords, charges, radii))):
        diff = np.abs(got - ref).max()
        print(f"closed form, {name}: {diff:.2e}")
        assert diff <= 1e-13, (name, diff)


def _water_charges(bs):
    """One at a time: on the oxygen nucleus with radius 0.5 (T = 0 on the one-centre pairs), 60 bohr away (the asymptotic
    Boys branch), and a general position."""
    o = bs.atoms[0][1]
    return [(o, 0.7, 0.5), (o + np.array([0.0, 0.0, 60.0]), -0.9, 1.0), (np.array([1.3, -2.1, 0.7]), 0.4, 0.8)]


def test_every_pair_order_against_the_two_electron_engine():
    """water / cc-pVDZ has every pair order l_ab = 0 .. 4 across different centres."""
    bs = _basis(WATER_XYZ, "cc-pvdz")
    assert {sa.ang + sb.ang for sa in bs.shells for sb in bs.shells} == {0, 1, 2, 3, 4}
    for pos, q, rad in _water_charges(bs):
        ref = _oracle(bs, pos, q, rad)
        for name, got in (("numpy", integrals.mm_potential(bs, [pos], [q], [rad])),
                          ("native", integrals.mm_potential_native(bs, [pos], [q], [rad]))):
            diff = np.abs(got - ref).max()
            print(f"oracle, q = {q}, radius = {rad}, {name}: {diff:.2e} (max |V| {np.abs(ref).max():.3f})")
            assert diff <= TOL * abs(q), (name, q, diff)


def test_point_charge_limit():
    bs = _basis(WATER_XYZ, "cc-pvdz")
    cases = _water_charges(bs)
    coords, charges = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    v_point = integrals.mm_potential_native(bs, coords, charges)
    diff = np.abs(v_point - _host_1e_v(bs, coords, charges)).max()
    print(f"point charges against nbx_host_1e: {diff:.2e}")
    assert diff <= TOL * np.abs(charges).sum()
    assert np.abs(integrals.mm_potential(bs, coords, charges) - v_point).max() <= TOL * np.abs(charges).sum()
    # radii of 1e-6 bohr: the lost erf tail is below 1e-300; what remains is rho = p / (1 + 1e-12 p) against p
    small = np.abs(integrals.mm_potential_native(bs, coords, charges, [1e-6] * 3) - v_point).max()
    print(f"radii of 1e-6 bohr against point charges: {small:.2e}")
    assert small <= 1e-9


def test_host_engine_against_numpy_with_f_shells():
    bs = _basis(WATER_XYZ, "cc-pvtz")
    assert integrals.max_ang(bs) == 3
    rng = np.random.default_rng(7)
    coords = rng.uniform(-4.0, 4.0, (5, 3))
    charges = np.array([0.6, -0.8, 0.35, -0.2, 1.0])
    radii = np.array([0.4, 1.5, 1e-6, 5.0, 0.9])
    ref = integrals.mm_potential(bs, coords, charges, radii)
    got = integrals.mm_potential_native(bs, coords, charges, radii)
    diff = np.abs(got - ref).max()
    print(f"host engine against numpy, cc-pVTZ: {diff:.2e}")
    assert diff <= TOL * np.abs(charges).sum()
    assert np.array_equal(got, got.T)
    assert np.array_equal(got, integrals.mm_potential_native(bs, coords, charges, radii, nthreads=1))
    zero = integrals.mm_potential_native(bs, np.zeros((0, 3)), np.zeros(0), np.zeros(0))
    assert zero.shape == (bs.nao, bs.nao) and not zero.any()
    assert not integrals.mm_potential(bs, np.zeros((0, 3)), np.zeros(0)).any()


def test_nuclear_energy_units_and_validation():
    atoms = [("O", np.array([0.0, 0.0, 0.0])), ("H", np.array([0.0, 0.0, 2.0]))]
    coords, charges = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, -1.0]]), np.array([0.5, -2.0])
    # O: 8 (0.5 / 5 - 2 / 1); H: 0.5 / sqrt(9 + 16 + 4) - 2 / 3
    expected = 8 * (0.1 - 2.0) + (0.5 / np.sqrt(29.0) - 2.0 / 3.0)
    assert abs(integrals.mm_nuclear_energy(atoms, coords, charges) - expected) < 1e-14
    assert integrals.mm_nuclear_energy(atoms, np.zeros((0, 3)), []) == 0.0

    # the same environment in angstrom and in bohr: bit-identical matrices
    ang_c, ang_r, q = [[1.1, -0.7, 0.4], [-2.0, 0.3, 1.6]], [0.5, 1.2], [0.4, -0.6]
    scale = 1.0 / integrals.BOHR
    bohr_c, bohr_r = (np.array(ang_c) * scale).tolist(), (np.array(ang_r) * scale).tolist()
    env_a = integrals.mm_environment(ang_c, q, ang_r, "angstrom")
    env_b = integrals.mm_environment(bohr_c, q, bohr_r, "bohr")
    for a, b in zip(env_a, env_b):
        assert np.array_equal(a, b)
    bs_a = integrals.Basis(integrals.parse_geometry(WATER_XYZ, "angstrom"), "sto-3g")
    assert np.array_equal(integrals.mm_potential_native(bs_a, *env_a), integrals.mm_potential_native(bs_a, *env_b))
    assert abs(env_a[0][0, 0] - 1.1 / 0.52917721092) < 1e-15 and abs(env_a[2][1] - 1.2 / 0.52917721092) < 1e-15

    good = dict(mm_coords=ang_c, mm_charges=q, mm_radii=ang_r)
    for field, value in (("mm_coords", [[1.0, 2.0], [3.0, 4.0]]), ("mm_coords", [[1.0, 2.0, 3.0]]), ("mm_charges", [[0.4, -0.6]]),
                         ("mm_radii", [0.5]), ("mm_radii", [0.5, 0.0]), ("mm_radii", [0.5, -1.0]),
                         ("mm_coords", [[1.0, 2.0, float("nan")], [0.0, 0.0, 0.0]]), ("mm_charges", [0.4, float("inf")]),
                         ("mm_radii", [0.5, float("nan")]), ("mm_charges", ["a", "b"])):
        with pytest.raises(NbedDriverError, match=field):
            integrals.mm_environment(**{**good, field: value})


def _config(charges=None, **kw):
    mm = {}
    if charges is not None:
        mm = dict(mm_coords=[[3.0, 0.5, -1.0], [-2.5, 1.5, 2.0]], mm_charges=list(charges), mm_radii=[0.6, 0.8])
    return NbedConfig(geometry=WATER_XYZ, n_active_atoms=2, basis="STO-3G", xc_functional="hf", projector="huzinaga",
                      convergence=1e-11, max_hf_cycles=200, max_dft_cycles=200, virtual_localization="disable", **mm, **kw)


def test_driver_with_an_mm_field_on_the_host_route():
    """water / STO-3G, HF-in-HF, Huzinaga projector, two Gaussian charges, on the CPU oracle backend: the field reaches
    both objects the reference wraps (global Kohn-Sham, embedded HF) and nothing else."""
    q0 = np.array([0.4, -0.5])
    cfg = _config(q0)
    assert BuiltinHFProvider.supports(cfg)
    drv = nbed(cfg, backend=OracleBackend())
    assert isinstance(drv.provider, BuiltinHFProvider) and drv.run_qmmm
    res = drv.huzinaga
    atoms = integrals.parse_geometry(WATER_XYZ)
    bs = integrals.Basis(atoms, "sto-3g")
    env = integrals.mm_environment(cfg.mm_coords, cfg.mm_charges, cfg.mm_radii, "angstrom")
    v_mm = integrals.mm_potential_native(bs, *env)
    e_mm = integrals.mm_nuclear_energy(atoms, env[0], env[1])
    plain = integrals.molecule_integrals(WATER_XYZ, "sto-3g")
    scf = res["scf"]
    assert np.array_equal(type(scf).get_hcore(scf), plain["hcore"] + v_mm)  # (the instance's get_hcore carries v_emb too)
    assert np.array_equal(np.asarray(drv._global_ks.get_hcore()), plain["hcore"] + v_mm)
    assert abs(scf.energy_nuc() - drv.e_nuc) < 1e-14
    assert abs(drv.e_nuc - (plain["e_nuc"] + e_mm)) < 1e-13
    e_field = drv._global_ks.e_tot
    assert scf.converged and abs(res["e_rhf"] - e_field) < 2e-6
    # the global HF object is not wrapped, as in the reference
    assert np.array_equal(np.asarray(drv.provider.global_hf(cfg).get_hcore()), plain["hcore"])

    free = nbed(_config(), backend=OracleBackend())
    assert not free.run_qmmm
    e_free = free._global_ks.e_tot
    assert abs(e_field - e_free) > 1e-4 and abs(res["e_rhf"] - free.huzinaga["e_rhf"]) > 1e-4

    # Hellmann-Feynman: dE / d(lambda) at lambda = 0 of the charges lambda q is tr(D_0 V_unit) + e_mm,unit with the
    # field-free density, which ties the sign and the prefactor of both new terms together
    lam = 1e-4
    provider = BuiltinHFProvider(OracleBackend())
    e_pm = [provider.global_ks(_config(s * lam * q0), True).e_tot for s in (1.0, -1.0)]
    d0 = np.asarray(free._global_ks.make_rdm1())
    d0 = d0[0] + d0[1] if d0.ndim == 3 else d0
    slope = float(np.einsum("ij,ji->", d0, v_mm)) + e_mm
    print(f"Hellmann-Feynman: finite difference {(e_pm[0] - e_pm[1]) / (2 * lam):.9f}, analytic {slope:.9f}")
    assert abs((e_pm[0] - e_pm[1]) / (2 * lam) - slope) < 1e-6


def test_mm_engine_selection_without_a_device():
    cfg = _config([0.4, -0.5])
    with pytest.raises(NbedDriverError, match="NBED_MM_ENGINE"):
        BuiltinHFProvider(OracleBackend(), mm_engine="gpu")
    with pytest.raises(NbedDriverError, match="mm_engine='device': the .* backend has no device integral engine"):
        BuiltinHFProvider(OracleBackend(), mm_engine="device").global_ks(cfg, True)
    # auto: the host without a device engine; with one, the device from AUTO_MM_MIN_WORK primitive pairs x charges on
    from nbed_amd import driver as drv_mod

    class WithEngine(OracleBackend):
        def mm_potential(self, *args, **kwargs):
            raise AssertionError("mm_route computes nothing")

    def many(m, basis="cc-pvdz"):
        return NbedConfig(geometry=WATER_XYZ, n_active_atoms=2, basis=basis, xc_functional="hf",
                          mm_coords=[[9.0, 0.0, 0.0]] * m, mm_charges=[0.1] * m, mm_radii=[1.0] * m)

    assert drv_mod.AUTO_MM_ON_DEVICE and drv_mod.AUTO_MM_MIN_WORK == 1_200_000
    assert BuiltinHFProvider(OracleBackend(), mm_engine="auto").mm_route(many(2000)) == "host"
    auto = BuiltinHFProvider(WithEngine(), mm_engine="auto")
    # water / cc-pVDZ has 793 primitive pairs: 1513 charges are 1 199 809, 1514 are 1 200 602
    assert auto.mm_route(many(1513)) == "host" and auto.mm_route(many(1514)) == "device"
    assert auto.mm_route(many(5000, "cc-pvtz")) == "host"  # f shells
    assert BuiltinHFProvider(WithEngine(), mm_engine="host").mm_route(many(5000)) == "host"
    # a shape error in the configuration names the field
    bad = _config([0.4, -0.5]).model_copy(update={"mm_radii": [0.6]})
    with pytest.raises(NbedDriverError, match="mm_radii"):
        BuiltinHFProvider(OracleBackend()).global_ks(bad, True)


def test_host_engine_under_the_sanitizers(tmp_path):
    """nbx_host_mm_potential in a stand-alone program built with AddressSanitizer and UBSan
    (tests/native/mm_potential_check.hip): s, p, d and f shells, no device, no Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.fail("no hipcc: the library this suite tests cannot have been built without it")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "mm_potential_check"
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", f"-I{root / 'include'}", f"-I{root / 'nbed_amd' / 'csrc'}",
                    str(root / "tests" / "native" / "mm_potential_check.hip"), "-pthread", "-o", str(exe)], check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("bad=0") == 5, r.stdout
