"""The potential of an MM environment on the device (nbx_mm_potential, csrc/mm_potential.hip) against
the host engine (nbx_host_mm_potential), which tests/test_host_mm_potential.py ties to a closed form and to the
two-electron engine; its bookkeeping (chunks of charges, screened pairs, refusals) and ``nbed(config)`` with
``mm_engine="device"``."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

from nbed_amd import NbedConfig, _nbx, integrals, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.exceptions import NbedDriverError

pytestmark = pytest.mark.gpu

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
WATER_PAIR_FAR = ("6\n\nO 0.0 0.0 0.115\nH 0.0 0.754 -0.459\nH 0.0 -0.754 -0.459\n"
                  "O 0.0 0.0 21.281\nH 0.0 0.754 20.707\nH 0.0 -0.754 20.707")  # 40 bohr = 21.166 angstrom apart

# Per unit of sum |q|: ten times the host engine's difference from its oracle (1.4e-15, tests/test_host_mm_potential.py)
# plus the bound on what the primitive screening of the session (cutoff 1e-16) removes (1e-13).
TOL = 10 * 1.4e-15 + 1e-13


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@lru_cache(maxsize=None)
def _basis(xyz=WATER, name="cc-pvdz"):
    return integrals.Basis(integrals.parse_geometry(xyz), name)


@lru_cache(maxsize=None)
def _environment(m):
    """m charges around water: the first on the oxygen nucleus, the second 60 bohr away, the others in a box of 8 bohr;
    radii mixed, 1e-6 and 5.0 bohr among them."""
    rng = np.random.default_rng(1000 + m)
    o = _basis().atoms[0][1]
    coords = rng.uniform(-8.0, 8.0, (m, 3))
    coords[0] = o
    if m > 1:
        coords[1] = o + np.array([0.0, 0.0, 60.0])
    charges = rng.uniform(0.2, 1.0, m) * rng.choice([-1.0, 1.0], m)
    radii = rng.choice([1e-6, 0.3, 0.8, 1.7, 5.0], m)
    radii[0] = 0.5
    for a in (coords, charges, radii):
        a.setflags(write=False)
    return coords, charges, radii


@lru_cache(maxsize=None)
def _host(m, point=False):
    coords, charges, radii = _environment(m)
    ref = integrals.mm_potential_native(_basis(), coords, charges, None if point else radii, nthreads=8)
    ref.setflags(write=False)
    return ref


def _device(be, m, point=False, bs=None):
    coords, charges, radii = _environment(m)
    return be.to_host(integrals.mm_potential_device(bs or _basis(), be, coords, charges, None if point else radii))


def _sizes(be):
    return (1, 63, 64, 65, 200, be.MM_CHUNK + 1)


def test_device_against_the_host_engine(be):
    for m in _sizes(be):
        got = _device(be, m)
        diff, scale = np.abs(got - _host(m)).max(), np.abs(_environment(m)[1]).sum()
        print(f"M = {m}: max |device - host| = {diff:.2e} (sum |q| = {scale:.1f}, max |V| = {np.abs(_host(m)).max():.2f})")
        assert diff <= TOL * scale, (m, diff)


def test_point_charges_against_the_nuclear_attraction_engine(be):
    lib = _nbx.load_library()
    bs = _basis()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for m in (65, be.MM_CHUNK + 1):
        coords, charges, _ = _environment(m)
        xyz, q = np.ascontiguousarray(coords), np.ascontiguousarray(charges)
        out = [np.empty((bs.nao, bs.nao)) for _ in range(3)]
        arrays = integrals._shell_arrays(bs)
        _nbx.check(lib, lib.nbx_host_1e(len(bs.shells), *(ptr(a) for a in arrays), m, ptr(q), ptr(xyz), 8, *(ptr(o) for o in out)))
        diff = np.abs(_device(be, m, point=True) - out[2]).max()
        print(f"M = {m}, point charges: max |device - nbx_host_1e| = {diff:.2e}")
        assert diff <= TOL * np.abs(charges).sum()


def test_reproducible_symmetric_and_every_element_written(be):
    m = be.MM_CHUNK + 1
    a, b = _device(be, m), _device(be, m)
    assert np.array_equal(a, b) and np.array_equal(a, a.T)
    # two waters 40 bohr apart in STO-3G: every primitive pair between them is screened out; the output starts as NaN
    far = _basis(WATER_PAIR_FAR, "sto-3g")
    coords, charges, radii = _environment(65)
    arrays = integrals._shell_arrays(far)
    out = be.empty((far.nao, far.nao))
    out.fill_(float("nan"))
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    zetas = np.ascontiguousarray(1.0 / radii**2)
    be._call("nbx_mm_potential", len(far.shells), *(ptr(x) for x in arrays), 1e-16, 65, ptr(np.ascontiguousarray(charges)),
             ptr(np.ascontiguousarray(coords)), ptr(zetas), be._p(out))
    v = be.to_host(out)
    half = far.nao // 2
    assert not np.isnan(v).any() and np.array_equal(v, v.T)
    assert not v[half:, :half].any() and v[:half, :half].any() and v[half:, half:].any()
    ref = integrals.mm_potential_native(far, coords, charges, radii)
    assert np.abs(v - ref).max() <= TOL * np.abs(charges).sum()
    # no charges: exact zeros
    zero = be.to_host(be.mm_potential(_basis(), np.zeros((0, 3)), np.zeros(0), np.zeros(0)))
    assert zero.shape == (_basis().nao,) * 2 and not zero.any() and not np.isnan(zero).any()


def test_chunks_of_charges_add_up(be):
    m = be.MM_CHUNK + 1
    coords, charges, radii = _environment(m)
    bs = _basis()
    whole = _device(be, m)
    first = be.to_host(integrals.mm_potential_device(bs, be, coords[:-1], charges[:-1], radii[:-1]))
    last = be.to_host(integrals.mm_potential_device(bs, be, coords[-1:], charges[-1:], radii[-1:]))
    assert np.abs(last).max() > 1e-3  # the charge past the chunk's end is seen
    assert np.abs(whole - (first + last)).max() <= TOL * np.abs(charges).sum()


def test_f_shells_are_refused_on_the_device_and_served_by_the_host(be, monkeypatch):
    bs = _basis(WATER, "cc-pvtz")
    coords, charges, radii = _environment(3)
    arrays = integrals._shell_arrays(bs)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = be.empty((bs.nao, bs.nao))
    rc = be.lib.nbx_mm_potential(be.ctx, len(bs.shells), *(ptr(x) for x in arrays), 1e-16, 3, ptr(np.ascontiguousarray(charges)),
                                 ptr(np.ascontiguousarray(coords)), None, be._p(out))
    assert rc == _nbx.NBX_E_INVALID
    assert be.lib.nbx_last_error().decode().startswith("nbx_mm_potential: invalid shells (angular momentum 0 .. 2")
    with pytest.raises(_nbx.NbxError, match="l <= 2"):
        be.mm_potential(bs, coords, charges)
    monkeypatch.delenv("NBED_MM_ENGINE", raising=False)
    cfg = NbedConfig(geometry=WATER, n_active_atoms=2, basis="cc-pvtz", xc_functional="hf", unit="angstrom",
                     mm_coords=coords.tolist(), mm_charges=charges.tolist(), mm_radii=radii.tolist())
    with pytest.raises(NbedDriverError, match="l = 3"):
        BuiltinHFProvider(be, mm_engine="device").mm_route(cfg)
    auto = BuiltinHFProvider(be)
    assert auto.mm_engine == "auto" and auto.mm_route(cfg) == "host"
    v_mm, e_mm = auto._mm_terms(cfg)
    env = integrals.mm_environment(cfg.mm_coords, cfg.mm_charges, cfg.mm_radii, "angstrom")
    assert np.array_equal(v_mm, integrals.mm_potential_native(bs, *env))


def test_nbed_with_the_field_on_the_device(be, monkeypatch):
    """water / STO-3G, two charges: mm_engine="device" against "host" for both projectors, and one run on the Cholesky
    factor against the dense route."""
    import ao2mo_factor_reference as afr

    monkeypatch.delenv("NBED_MM_ENGINE", raising=False)
    monkeypatch.delenv("NBED_ERI_ENGINE", raising=False)
    cfg = NbedConfig(geometry=WATER, n_active_atoms=2, basis="STO-3G", xc_functional="hf", projector="both",
                     convergence=1e-10, max_hf_cycles=200, max_dft_cycles=200,
                     mm_coords=[[3.0, 0.5, -1.0], [-2.5, 1.5, 2.0]], mm_charges=[0.4, -0.5], mm_radii=[0.6, 0.8])
    runs = {}
    for engine in ("device", "host"):
        provider = BuiltinHFProvider(be, mm_engine=engine)
        assert provider.mm_route(cfg) == engine
        runs[engine] = nbed(cfg, provider=provider, backend=be)
    for proj in ("mu", "huzinaga"):
        d, h = getattr(runs["device"], proj), getattr(runs["host"], proj)
        assert d["scf"].converged and h["scf"].converged
        print(f"{proj}: e_rhf device {d['e_rhf']:.10f} host {h['e_rhf']:.10f}")
        assert abs(d["e_rhf"] - h["e_rhf"]) < 1e-8
    assert abs(runs["device"]._global_ks.e_tot - runs["host"]._global_ks.e_tot) < 1e-8
    assert abs(runs["device"].e_nuc - runs["host"].e_nuc) < 1e-13
    chol = nbed(cfg, provider=BuiltinHFProvider(be, eri_engine="cholesky", cholesky_tol=1e-8, mm_engine="device"), backend=be)
    for proj in ("mu", "huzinaga"):
        res = getattr(chol, proj)
        assert res["scf"].converged and res["scf"].eri_factor_device() is not None
        assert abs(res["e_rhf"] - getattr(runs["device"], proj)["e_rhf"]) <= 10 * afr.E2E_MEASURED["energy"]
