"""The device integral engine (nbx_eri_device, csrc/eri.hip; HipBackend.eri) against the host engine it shares its pair
data and screening with (integrals.two_electron_native, itself pinned to the numpy engine and to the oracle in
tests/test_host_integrals.py), element by element; its exact symmetry, zero pattern and determinism; what it refuses; and
the embedding driver on both routes of BuiltinHFProvider."""

import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from nbed_amd import NbedConfig, _nbx, integrals, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.exceptions import NbedDriverError

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
from molecules import octane_xyz  # noqa: E402

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
H2O2 = "4\n\nO   0.000  0.734  -0.052\nO   0.000  -0.734  -0.052\nH   0.839  0.881  0.419\nH   -0.839  -0.881  0.419"
H2 = "2\n\nH 0.0 0.0 0.0\nH 0.0 0.0 0.74"
H2_FAR = "2\n\nH 0 0 0\nH 0 0 12.0"

# the smallest molecules that reach every branch (the largest tensor: 32^4 doubles = 8 MB)
CASES = {
    "h2-sto3g": (H2, "sto-3g", False),                  # two shells, six quartets, one class
    "one-s-shell": ("1\n\nH 0 0 0", {"H": [(0, (0.5,), (1.0,))]}, False),  # one function
    "h2o2-sto3g": (H2O2, "sto-3g", False),              # deep s/p contractions, all s/p classes
    "water-631gs": (WATER, "6-31g*", False),            # d classes on one centre, 6-primitive core
    "water-631gs-cart": (WATER, "6-31g*", True),        # six Cartesian d functions
    "h2o2-631gs": (H2O2, "6-31g*", False),              # 32 AOs, a two-centre (dd|dd) with L = 8
    "h2-12A-ccpvdz": (H2_FAR, "cc-pvdz", False),        # asymptotic Boys branch (T ~ 1e3), screened pairs, p shells
}
F_TABLE = {"C": [(1, (0.38, 0.9), (0.7, 0.4)), (2, (1.097,), (1.0,)), (3, (0.761,), (1.0,))],
           "H": [(0, (0.3,), (1.0,)), (2, (1.057,), (1.0,)), (3, (0.9,), (1.0,))]}


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@lru_cache(maxsize=None)
def _basis(name):
    xyz, basis, cart = CASES[name]
    return integrals.Basis(integrals.parse_geometry(xyz), basis, cart)


@lru_cache(maxsize=None)
def _ref(name):
    ref = integrals.two_electron_native(_basis(name), nthreads=4)
    ref.setflags(write=False)
    return ref


_GOT = {}


def _got(be, name):
    if name not in _GOT:
        t = integrals.two_electron_device(_basis(name), be)
        assert tuple(t.shape) == (_basis(name).nao,) * 4 and t.is_cuda
        _GOT[name] = be.to_host(t)
        _GOT[name].setflags(write=False)
    return _GOT[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_engine_matches_the_host_engine_element_by_element(be, name):
    """atol = 2e-13: the bound the project holds between its two host engines, which differ in summation order as these two
    do (tests/test_host_integrals.py, test_native_eri_engine_matches_the_numpy_engine)."""
    got, ref = _got(be, name), _ref(name)
    print(f"{name}: nao = {ref.shape[0]}, max |device - host| = {np.abs(got - ref).max():.3e}, max |host| = {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-13)
    if name == "one-s-shell":
        assert got.shape == (1, 1, 1, 1) and got[0, 0, 0, 0] > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_eight_images_of_an_integral_are_the_same_double(be, name):
    got = _got(be, name)
    np.testing.assert_array_equal(got, got.transpose(1, 0, 3, 2))
    np.testing.assert_array_equal(got, got.transpose(2, 3, 0, 1))
    np.testing.assert_array_equal(got, got.transpose(1, 0, 2, 3))


def test_screened_quartets_are_exact_zeros_and_nothing_is_left_unwritten(monkeypatch):
    """Stretched H2 on a backend whose ``empty`` hands out NaN (NBED_POISON_EMPTY=1): the engine's memset and stores cover
    the whole tensor, and the quartets it skips are the ones the host engine skips."""
    from nbed_amd.backend import HipBackend

    monkeypatch.setenv("NBED_POISON_EMPTY", "1")
    poisoned = HipBackend()
    assert np.isnan(poisoned.to_host(poisoned.empty(3))).all()
    got = poisoned.to_host(poisoned.eri(_basis("h2-12A-ccpvdz")))
    ref = _ref("h2-12A-ccpvdz")
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got == 0, ref == 0)
    assert 0.2 < (got == 0).mean() < 0.99


def test_two_calls_give_the_same_bits(be):
    first = _got(be, "h2o2-631gs")
    again = be.to_host(be.eri(_basis("h2o2-631gs")))
    np.testing.assert_array_equal(first, again)


def test_cutoff_is_the_host_engines(be):
    """A coarse cutoff drops the same quartets in both engines."""
    bs = _basis("h2-12A-ccpvdz")
    got = be.to_host(be.eri(bs, cutoff=1e-6))
    ref = integrals.two_electron_native(bs, nthreads=4, cutoff=1e-6)
    np.testing.assert_array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-13)
    assert (ref == 0).sum() > (_ref("h2-12A-ccpvdz") == 0).sum()


def test_f_shells_are_refused(be):
    bs = integrals.Basis(integrals.parse_geometry("2\n\nC 0.1 -0.2 0.3\nH 0.9 0.5 -0.4"), F_TABLE)
    assert integrals.max_ang(bs) == 3
    with pytest.raises(_nbx.NbxError) as err:
        be.eri(bs)
    assert err.value.code == _nbx.NBX_E_INVALID
    # the library itself, not only the Python check in front of it
    import ctypes

    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = be.zeros(1)
    rc = be.lib.nbx_eri_device(be.ctx, len(bs.shells), *(ptr(a) for a in integrals._shell_arrays(bs)), 1e-16, be._p(out))
    assert rc == _nbx.NBX_E_INVALID and float(be.to_host(out)[0]) == 0.0


def _config(basis):
    return NbedConfig(geometry=WATER, n_active_atoms=2, basis=basis, xc_functional="b3lyp", convergence=1e-9,
                      projector="huzinaga", max_hf_cycles=100, max_dft_cycles=100, virtual_localization="cl")


def test_provider_routes_and_refusals(be, monkeypatch):
    monkeypatch.delenv("NBED_ERI_ENGINE", raising=False)
    tz, dz = _config("cc-pvtz"), _config("cc-pvdz")
    with pytest.raises(NbedDriverError, match="l = 3"):
        BuiltinHFProvider(be, eri_engine="device")._integrals(tz)
    assert BuiltinHFProvider(be, eri_engine="auto")._eri_route(tz) == "host"
    assert BuiltinHFProvider(be)._eri_route(tz) == "host"
    # auto: the device from AUTO_ERI_MIN_NAO functions on (propane / 6-31G*: 58), the host below (water / cc-pVDZ: 24)
    propane = NbedConfig(geometry=octane_xyz(3), n_active_atoms=4, basis="6-31g*", xc_functional="b3lyp", convergence=1e-8)
    assert BuiltinHFProvider(be)._eri_route(propane) == "device" and BuiltinHFProvider(be)._eri_route(dz) == "host"
    assert BuiltinHFProvider(be, eri_engine="device")._eri_route(dz) == "device"
    assert BuiltinHFProvider(be, eri_engine="host")._eri_route(dz) == "host"
    monkeypatch.setenv("NBED_ERI_ENGINE", "device")
    assert BuiltinHFProvider(be)._eri_route(dz) == "device"
    assert BuiltinHFProvider(be, eri_engine="host")._eri_route(dz) == "host"  # the argument wins
    monkeypatch.setenv("NBED_ERI_ENGINE", "gpu")
    with pytest.raises(NbedDriverError, match="NBED_ERI_ENGINE='gpu'.*'auto', 'host' or 'device'"):
        BuiltinHFProvider(be)
    assert BuiltinHFProvider(be, eri_engine="host").eri_engine == "host"

    class NoEri:
        name = "checker"

    with pytest.raises(NbedDriverError, match="no device integral engine"):
        BuiltinHFProvider(NoEri(), eri_engine="device")._integrals(dz)


def test_embedding_agrees_between_the_two_routes_and_the_device_route_keeps_no_host_tensor(be, monkeypatch):
    """configs[1] (water / cc-pVDZ, Huzinaga, B3LYP-in-HF: the configuration of test_water_ccpvdz_huzinaga_matches_checker_backend,
    with that test's bounds between two backends) once per route on the same backend."""
    monkeypatch.delenv("NBED_ERI_ENGINE", raising=False)
    cfg = _config("cc-pvdz")
    on_device = BuiltinHFProvider(be, eri_engine="device")
    got = nbed(cfg, provider=on_device, backend=be)
    on_host = BuiltinHFProvider(be, eri_engine="host")
    ref = nbed(cfg, provider=on_host, backend=be)
    print(f"e_tot device {got._global_ks.e_tot:.12f} host {ref._global_ks.e_tot:.12f}")
    assert abs(got._global_ks.e_tot - ref._global_ks.e_tot) < 1e-8
    for key in ("e_rhf", "classical_energy", "correction"):
        print(f"{key}: device {got.huzinaga[key]:.12f} host {ref.huzinaga[key]:.12f}")
        assert abs(got.huzinaga[key] - ref.huzinaga[key]) < 1e-7, key
    assert got.huzinaga["scf"].converged

    def host_tensors(cache):
        n4 = 24 ** 4
        found = []
        for key, val in cache.items():
            items = dict.items(val) if isinstance(val, dict) else [(None, val)]
            found += [(key, k) for k, v in items if isinstance(v, np.ndarray) and v.size == n4]
        return found

    ints = on_device._cache[(cfg.geometry, "cc-pvdz", str(cfg.unit))]
    assert "eri" not in ints and not host_tensors(on_device._cache)
    assert len(host_tensors(on_host._cache)) == 1  # (the probe does find the host route's tensor)
    # a caller that does ask the device route's dict gets the tensor read back from the device, and it is not kept
    lazy = ints["eri"]
    np.testing.assert_allclose(lazy, on_host._cache[(cfg.geometry, "cc-pvdz", str(cfg.unit))]["eri"], rtol=0, atol=2e-13)
    assert "eri" not in ints


def test_injected_host_tensor_is_still_honoured(be):
    """A ``_cache`` entry that already holds a host "eri" (what the real-molecule tests inject) is uploaded as before, on
    every setting of the engine."""
    cfg = NbedConfig(geometry=H2, n_active_atoms=1, basis="sto-3g", xc_functional="hf", convergence=1e-9)
    m = integrals.molecule_integrals(H2, "sto-3g")
    marked = dict(m, eri=m["eri"] * 1.0)
    marked["eri"][0, 0, 0, 0] = 123.0
    for mode in ("auto", "host", "device"):
        prov = BuiltinHFProvider(be, eri_engine=mode)
        prov._cache[(cfg.geometry, "sto-3g", str(cfg.unit))] = marked
        assert float(be.to_host(prov._eri_kwargs(cfg, be)["eri"])[0, 0, 0, 0]) == 123.0
