"""The device engine's attenuated integrals (pq| erf(omega r12) / r12 |rs) (nbx_eri_device_erf: the class kernel of
csrc/eri.hip with 1 / omega^2 in its arguments; HipBackend.eri(omega=)) against the host engine's (nbx_host_eri_erf, pinned
to an independent reference in tests/test_host_eri_erf.py), element by element at the bound tests/test_gpu_eri.py holds for
the plain tensor; exact symmetry, determinism, the zero pattern of screened quartets, and the limit omega -> infinity."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

from nbed_amd import _nbx, integrals

pytestmark = pytest.mark.gpu

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
H2_FAR = "2\n\nH 0 0 0\nH 0 0 12.0"
OMEGAS = (1e-3, 0.33, 1e3)
ATOL = 2e-13  # tests/test_gpu_eri.py, device against host for the plain tensor

# s, p and d shells on each of two centres (18 functions, one s and one d shell contracted): every pair order
# l_ab = 0 .. 4 occurs with its two shells on different centres, so all 25 classes hold two-centre pairs
ALL_CLASSES_TABLE = {"O": [(0, (1.1, 0.35), (0.6, 0.5)), (1, (0.8,), (1.0,)), (2, (0.9,), (1.0,))],
                     "C": [(0, (0.45,), (1.0,)), (1, (1.4, 0.3), (0.5, 0.6)), (2, (0.6, 1.8), (0.7, 0.4))]}
ALL_CLASSES_XYZ = "2\n\nO 0.1 -0.2 0.3\nC 0.8 0.5 -0.4"


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@lru_cache(maxsize=None)
def _basis(name):
    if name == "all-classes":
        return integrals.Basis(integrals.parse_geometry(ALL_CLASSES_XYZ), ALL_CLASSES_TABLE)
    if name == "h2-12A-ccpvdz":
        return integrals.Basis(integrals.parse_geometry(H2_FAR), "cc-pvdz")
    return integrals.Basis(integrals.parse_geometry(WATER), "cc-pvdz")


@lru_cache(maxsize=None)
def _host(name, omega, cutoff=1e-16):
    ref = integrals.two_electron_native(_basis(name), nthreads=4, omega=omega, cutoff=cutoff)
    ref.setflags(write=False)
    return ref


_GOT = {}


def _device(be, name, omega):
    if (name, omega) not in _GOT:
        t = integrals.eri_device(_basis(name), be, omega=omega)
        assert tuple(t.shape) == (_basis(name).nao,) * 4 and t.is_cuda
        _GOT[name, omega] = be.to_host(t)
        _GOT[name, omega].setflags(write=False)
    return _GOT[name, omega]


def test_every_class_is_launched_on_two_centre_pairs():
    bs = _basis("all-classes")
    assert bs.nao == 18 <= 30
    orders = {sa.ang + sb.ang for sa in bs.shells for sb in bs.shells if not np.array_equal(sa.centre, sb.centre)}
    assert orders == {0, 1, 2, 3, 4}
    lib = _nbx.load_library()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    counts, grid = (ctypes.c_int64 * 25)(), (ctypes.c_int64 * 25)()
    lds, block = (ctypes.c_int * 25)(), (ctypes.c_int * 25)()
    # (the plan does not depend on omega: the attenuated tensor runs the plain tensor's lists)
    assert lib.nbx_eri_plan(len(bs.shells), *(ptr(a) for a in integrals._shell_arrays(bs)), 1e-16, counts, lds, block,
                            grid) == _nbx.NBX_OK
    assert min(counts[:]) > 0 and min(grid[:]) > 0, counts[:]


@pytest.mark.parametrize("omega", OMEGAS)
def test_device_matches_host_in_all_25_classes(be, omega):
    """Measured max |device - host| on the 18-function table (MI355X): see the printed line; the bound is the plain
    tensor's."""
    got, ref = _device(be, "all-classes", omega), _host("all-classes", omega)
    print(f"omega = {omega:g}: max |device - host| = {np.abs(got - ref).max():.3e}, max |host| = {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    assert np.abs(ref).max() > 0


def test_device_matches_host_on_water_ccpvdz(be):
    got, ref = _device(be, "water-ccpvdz", 0.33), _host("water-ccpvdz", 0.33)
    print(f"water / cc-pVDZ, omega = 0.33: max |device - host| = {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    plain = be.to_host(be.eri(_basis("water-ccpvdz")))
    # a different tensor, below the plain one on the diagonal (pq|pq)
    n = ref.shape[0]
    diag, diag_plain = (np.einsum("pqpq->pq", t) for t in (got, plain))
    assert np.all(diag <= diag_plain + 1e-14) and np.abs(got - plain).max() > 0.1 and n == 24


@pytest.mark.parametrize("name,omega", [("all-classes", 0.33), ("all-classes", 1e-3), ("water-ccpvdz", 0.33)])
def test_eight_images_of_an_integral_are_the_same_double(be, name, omega):
    got = _device(be, name, omega)
    np.testing.assert_array_equal(got, got.transpose(1, 0, 3, 2))
    np.testing.assert_array_equal(got, got.transpose(2, 3, 0, 1))
    np.testing.assert_array_equal(got, got.transpose(1, 0, 2, 3))


def test_two_calls_give_the_same_bits(be):
    first = _device(be, "water-ccpvdz", 0.33)
    again = be.to_host(be.eri_device(_basis("water-ccpvdz"), omega=0.33))
    np.testing.assert_array_equal(first, again)


def test_screened_quartets_are_exact_zeros_and_nothing_is_left_unwritten(monkeypatch):
    """Stretched H2 at a cutoff of 1e-6 on a backend whose ``empty`` hands out NaN (NBED_POISON_EMPTY=1): memset and stores
    cover the whole tensor, and the skipped quartets are the host engine's -- the plain tensor's."""
    from nbed_amd.backend import HipBackend

    monkeypatch.setenv("NBED_POISON_EMPTY", "1")
    poisoned = HipBackend()
    assert np.isnan(poisoned.to_host(poisoned.empty(3))).all()
    bs = _basis("h2-12A-ccpvdz")
    got = poisoned.to_host(poisoned.eri(bs, cutoff=1e-6, omega=0.33))
    ref = _host("h2-12A-ccpvdz", 0.33, 1e-6)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got == 0, ref == 0)
    np.testing.assert_array_equal(got == 0, integrals.two_electron_native(bs, nthreads=4, cutoff=1e-6) == 0)
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL)
    assert (got == 0).sum() > (_host("h2-12A-ccpvdz", 0.33) == 0).sum() and 0.2 < (got == 0).mean() < 0.99


def test_large_omega_is_the_plain_device_tensor(be):
    for name in ("all-classes", "h2-12A-ccpvdz"):  # exponents up to 1.8 and up to 13
        bs = _basis(name)
        plain = be.to_host(be.eri(bs))
        got = be.to_host(be.eri(bs, omega=1e6))
        top = max(float(np.max(sh.exps)) for sh in bs.shells)
        rel = np.abs(got - plain).max() / np.abs(plain).max()
        print(f"{name}: largest exponent {top:g}, omega = 1e6: {rel:.2e} relative to the largest element")
        assert rel <= 1e-8


def test_refusals(be):
    bs = _basis("all-classes")
    for bad in (0.0, -0.33, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="omega"):
            integrals.eri_device(bs, be, omega=bad)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = be.zeros(1)
    arrays = integrals._shell_arrays(bs)
    for bad in (0.0, float("nan")):
        rc = be.lib.nbx_eri_device_erf(be.ctx, len(bs.shells), *(ptr(a) for a in arrays), 1e-16, bad, be._p(out))
        assert rc == _nbx.NBX_E_INVALID and float(be.to_host(out)[0]) == 0.0
