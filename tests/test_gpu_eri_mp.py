"""The device integral engine (csrc/eri.hip on eri_device.h and ints_md.h: 25 class kernels, 1 / r12 and
erf(omega r12) / r12; csrc/mm_potential.hip: five pair orders) against the extended-precision reference of
tests/eri_mp_reference.py, element by element, nothing screened (cutoff = 0).

The bound is relative to each element's own scale: |device - reference| <= K EPS A-bar + 1e-300 with A-bar the same
evaluation over absolute values and K = 4 max(1, r_twin) measured per case from the float64 twin of the reference
(mpmath Boys values rounded to double) -- computed at run time and printed, never a constant here.
tests/test_host_eri_mp_reference.py certifies the reference against mpmath, holds the host engines to the same bound and
shows that the bound catches a Boys evaluation that is short of Taylor terms, one that switches branches too early and a
dropped ket sign.

Cases (all 18 to 20 functions): the generic two-centre table of tests/test_gpu_eri_erf.py (spherical and Cartesian d);
the sweep of the Boys argument T of the (AA|BB) quartets over a table node, half a table step, both sides of the switch
at 41, the asymptotic branch and the underflow of the cross-centre pairs; exponents of 5e4 next to 0.02 with a
contraction of mixed sign; omega in {1e-3, 0.33, 1e3} and alpha_w R^2 on both sides of 41; eight charges around the
molecule (on a nucleus, 1e-5 Bohr from it, rho R^2 on both sides of 41 for the tightest pair) as points, as Gaussians of
mixed and of diffuse exponent, and three charges 60 Bohr away in calls of their own.

Each test prints nao, K and the worst ratio |x - reference| / (EPS A-bar) of the device and of the twin per class
(l_a + l_b, l_c + l_d) -- the classes of csrc/eri.hip -- or per pair order for the potential.  What is not repeated here:
the diagonal and column sinks (bit-identical to slices of the dense tensor, tests/test_gpu_eri_cholesky.py), screening
at the default cutoff (tests/test_gpu_eri.py), the chunking of charges (tests/test_gpu_mm_potential.py).

Measured on an MI355X, worst ratio per case in units of EPS A-bar (host: the host engine in
tests/test_host_eri_mp_reference.py).  Every one of the 25 classes and five pair orders has a non-zero device ratio.

    case                        K  device   twin   host
    generic                  11.3     3.4   2.81    3.4
    generic-cart             12.2     3.4   3.06    3.4
    extremes                 33.2    6.43    8.3   6.43
    sweep-1e-09              9.37    1.41   2.34    1.4
    sweep-0.05               10.2    1.94   2.55   1.93
    sweep-0.15               7.96    1.28   1.99   1.28
    sweep-20.05                23    7.34   5.76   7.34
    sweep-40.95              58.9    13.6   14.7   13.6
    sweep-40.9999            13.2    10.4   3.29   6.58
    sweep-41                 42.7    10.1   10.7   10.1
    sweep-41.0001              62    17.1   15.5   17.1
    sweep-45                 60.1    13.1     15   13.1
    sweep-1000                441     109    110    109
    sweep-100000             6.11    1.23   1.53   1.23
    generic-w0.001           15.8    3.15   3.94   3.15
    generic-w0.33            16.2    3.26   4.06   3.26
    generic-w1000              13    3.84   3.25   3.84
    generic-cart-w0.33       24.8    3.54    6.2   4.09
    sweep-w0.33-40.9999       105    24.7   26.2   24.7
    sweep-w0.33-41.0001       237    58.4   59.3   58.4
    near-points                 4   0.356  0.284  0.671
    near-mixed                  4   0.853   0.21  0.853
    near-0.04                   4   0.221  0.211   0.27
    far-points                  4   0.462  0.276  0.426
    far-mixed                   4   0.652  0.527  0.652

The device follows the host engine to the printed digits nearly everywhere: they share the algorithm, and the device's
exp, sqrt and FMA contraction do not show at this resolution.  The large K of the sweeps from T = 40.95 on is the twin's
own: the argument mu R^2 of the cross-centre pair factor (20 to 500) is rounded to double before exp.  The nearest
approach to the bound is sweep-40.9999, class (4, 4): 10.4 of 13.2, where the rounding of R happens to spare the twin
(3.29) and what is left is the table-based Boys evaluation just below its switch, F_8 from the top table row and eight
downward steps (host 6.58; the restated table in the twin, 6.01).
"""

import numpy as np
import pytest

import eri_mp_reference as mpr
from nbed_amd import integrals

pytestmark = pytest.mark.gpu

ALL_CLASSES = ("generic", "generic-cart", "extremes", "generic-w0.001", "generic-w0.33", "generic-w1000",
               "generic-cart-w0.33")  # every class holds two-centre pairs with no symmetry zeros among them


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


def _report(label, case, got):
    r_dev, r_twin = mpr.ratios(got, case.ref, case.scale), mpr.ratios(case.twin, case.ref, case.scale)
    print(f"{label}: nao = {case.basis.nao}, K = {case.k:.4g}, worst device = {r_dev.max():.4g}, worst twin = "
          f"{r_twin.max():.4g} (units of EPS A-bar)")
    per_class = mpr.worst_per_class(r_dev, case.shells)
    print(mpr.format_classes("device, per class", per_class))
    print(mpr.format_classes("twin, per class", mpr.worst_per_class(r_twin, case.shells)))
    return r_dev, per_class


@pytest.mark.parametrize("label", list(mpr.ERI_CASES))
def test_device_eri_within_the_bound(be, label):
    case = mpr.eri_case(label)
    assert 18 <= case.basis.nao <= 20 and case.k >= mpr.MARGIN and np.isfinite(case.k)
    t = integrals.two_electron_device(case.basis, be, cutoff=0.0, omega=case.omega)
    assert tuple(t.shape) == (case.basis.nao,) * 4 and t.is_cuda
    got = be.to_host(t)
    assert np.isfinite(got).all()
    r, per_class = _report(label, case, got)
    bad = mpr.violations(got, case.ref, case.scale, case.k)
    assert len(bad) == 0, (len(bad), [tuple(int(i) for i in e) for e in bad[:5]], float(r.max()), case.k)
    assert per_class.shape == (5, 5) and r.max() > 0  # something was compared
    if label in ALL_CLASSES:
        assert per_class.min() > 0, per_class


@pytest.mark.parametrize("label", list(mpr.MM_CASES))
def test_device_mm_potential_within_the_bound(be, label):
    case = mpr.mm_case(label)
    assert case.k >= mpr.MARGIN and np.isfinite(case.k)
    v = be.mm_potential(case.basis, case.coords, case.charges, case.zetas, cutoff=0.0)
    assert tuple(v.shape) == (case.basis.nao,) * 2 and v.is_cuda
    got = be.to_host(v)
    assert np.isfinite(got).all() and np.abs(got).max() > 1e-3
    r, per_order = _report(label, case, got)
    bad = mpr.violations(got, case.ref, case.scale, case.k)
    assert len(bad) == 0, (len(bad), [tuple(int(i) for i in e) for e in bad[:5]], float(r.max()), case.k)
    assert per_order.shape == (5,) and per_order.min() > 0, per_order  # all five pair orders were compared
