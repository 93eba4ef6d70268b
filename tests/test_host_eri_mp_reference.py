"""The extended-precision reference of the integral engines (tests/eri_mp_reference.py) and the host engines under its
bound.  Three parts:

1. the reference certifies itself: the same code on mpmath.mpf scalars at 50 digits agrees with the longdouble run to
   2^-10 of the bound's unit EPS A-bar on every (ss|ss) primitive quartet of the cases, on single-primitive two-centre
   (dd|dd) quartets and on a (dd| charges) pair; (ss|ss) agrees with the closed form of tests/eri_erf_reference.py; the
   mpmath Boys values obey F_n(0) = 1 / (2n + 1), the downward recursion and the confluent hypergeometric form; and
   sampled elements of every class agree with ``oracle.gto.eri_element_general``, an independent restatement;
2. nbx_host_eri, nbx_host_eri_erf and nbx_host_mm_potential with nothing screened stay within K EPS A-bar of the
   reference in every case, with K = 4 max(1, r_twin) measured from the float64 twin (printed, never a constant here);
3. the bound would catch a subtly wrong kernel: the table-based Boys evaluation restated in numpy passes every sweep
   case as the twin's Boys function, and fails the named case with six Taylor terms instead of nine, with the switch to
   the asymptotic branch at T >= 25 instead of 41, and the tensor fails with the ket sign dropped from one index."""

import ctypes
import itertools

import mpmath as mp
import numpy as np
import pytest

import eri_erf_reference as er
import eri_mp_reference as mpr
from nbed_amd import _nbx, integrals
from oracle import gto as oracle_gto

CERTIFY = 2.0 ** -10  # of EPS A-bar: the longdouble reference against the same code in mpmath


def _mpf_ratio(got, exact, scale):
    """max |got - exact| / (EPS A-bar) with ``exact`` an object array of mpf; inf where only A-bar vanishes."""
    worst = 0.0
    with mp.workdps(mpr.MP_DPS):
        for g, e, s in zip(np.ravel(got), np.ravel(exact), np.ravel(scale)):
            diff = abs(mpr.to_mp(g) - e)
            if diff > mpr.FLOOR:  # (the floor of the bound: exp(-5e4) is zero in longdouble and 1e-21715 in mpmath)
                worst = max(worst, float(diff / (mpr.EPS * mpr.to_mp(s))) if s > 0 else np.inf)
    return worst


def _quartet_three_ways(shells, omega):
    with mp.workdps(mpr.MP_DPS):
        return tuple(mpr.quartet_ao(mpr.Arith(mode), *shells, omega=omega) for mode in ("reference", "mpf", "magnitude"))


def _s_primitives(shells):
    """Every primitive of every s shell as a shell of its own, its contraction coefficient kept."""
    return [mpr.Shell(0, sh.centre, (a,), (c,), ((1.0,),)) for sh in shells if sh.ang == 0 for a, c in zip(sh.exps, sh.coefs)]


def test_longdouble_is_an_extended_type():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63  # what the certification below rests on


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_mpmath_boys_values():
    with mp.workdps(mpr.MP_DPS):
        tol = mp.mpf(10) ** (8 - mpr.MP_DPS)
        assert mpr.boys_mp(8, 0.0) == [mp.mpf(1) / (2 * n + 1) for n in range(9)]
        for t in (1e-300, 1e-9, 0.05, 0.15, 20.05, 40.9999, 41.0, 45.0, 1e3, 1e5):
            f = mpr.boys_mp(8, t)
            tm, et = mp.mpf(t), mp.exp(-mp.mpf(t))
            for n in range(9):
                # an independent evaluation of each order, and the recursion that ties neighbours together
                direct = mp.hyp1f1(n + mp.mpf(1) / 2, n + mp.mpf(3) / 2, -tm) / (2 * n + 1)
                assert abs(f[n] - direct) <= tol * direct, (t, n)
                if n:
                    assert abs((2 * n - 1) * f[n - 1] - (2 * tm * f[n] + et)) <= tol * f[n - 1], (t, n)
            assert abs(f[0] - mp.sqrt(mp.pi / tm) * mp.erf(mp.sqrt(tm)) / 2) <= tol * f[0]
        for n, v in enumerate(mpr.boys_mp(8, 1e-300)):
            assert abs(v - mp.mpf(1) / (2 * n + 1)) <= tol  # continuous into T = 0


def test_longdouble_agrees_with_mpmath_on_every_ssss_primitive_quartet():
    worst, count = 0.0, 0
    seen = set()
    for label, (key, omega) in mpr.ERI_CASES.items():
        prims = tuple(_s_primitives(mpr.shells_of(mpr.case_basis(key))))
        if (prims, omega) in seen:  # (the spherical and the Cartesian generic case share their s shells)
            continue
        seen.add((prims, omega))
        n = len(prims)
        case_worst = 0.0
        for quartet in itertools.product(prims, repeat=4):
            ld, exact, scale = _quartet_three_ways(quartet, omega)
            case_worst = max(case_worst, _mpf_ratio(ld, exact, scale))
            count += 1
        print(f"{label}: {n} s primitives, worst |longdouble - mpf| = {case_worst:.3g} EPS A-bar")
        worst = max(worst, case_worst)
    print(f"{count} quartets, worst {worst:.3g} against {CERTIFY:.3g}")
    assert count > 500 and worst <= CERTIFY


@pytest.mark.parametrize("t,omega", [(0.15, None), (20.05, None), (41.0001, None), (20.05, 0.33), (1e-9, 1e3)])
def test_longdouble_agrees_with_mpmath_on_two_centre_dddd(t, omega):
    """Single-primitive d shells of the sweep geometry: (d_A d_B | d_A d_B) and (d_A d_A | d_B d_B), 625 AO elements each
    through the E coefficients, the R table up to order 8 and the Cartesian-to-AO step."""
    sh = mpr.shells_of(mpr.sweep_basis(mpr.sweep_distance(t)))
    da, db = sh[2], sh[5]
    assert da.ang == db.ang == 2 and len(da.exps) == 1 and da.centre != db.centre
    for quartet in ((da, db, da, db), (da, da, db, db)):
        ld, exact, scale = _quartet_three_ways(quartet, omega)
        worst = _mpf_ratio(ld, exact, scale)
        print(f"T = {t:g}, omega = {omega}: worst |longdouble - mpf| = {worst:.3g} EPS A-bar, largest element "
              f"{float(np.abs(ld).max()):.3g}")
        assert worst <= CERTIFY and np.abs(ld).max() > 0


@pytest.mark.parametrize("label", ["near-points", "near-mixed", "far-mixed"])
def test_longdouble_agrees_with_mpmath_on_a_dd_charge_pair(label):
    q, xyz, zetas = mpr.MM_CASES[label]
    sh = mpr.shells_of(mpr.case_basis("generic"))
    da = sh[2]
    db = mpr.Shell(2, sh[5].centre, sh[5].exps[1:], sh[5].coefs[1:], sh[5].sph)  # the tight primitive of the carbon's d shell
    with mp.workdps(mpr.MP_DPS):
        ld, exact, scale = (mpr.charge_pair_ao(mpr.Arith(mode), da, db, np.array(q), np.array(xyz),
                                               None if zetas is None else np.array(zetas))
                            for mode in ("reference", "mpf", "magnitude"))
    worst = _mpf_ratio(ld, exact, scale)
    print(f"{label}: worst |longdouble - mpf| = {worst:.3g} EPS A-bar")
    assert worst <= CERTIFY and np.abs(ld).max() > 0


def test_ssss_is_the_closed_form():
    """(s_A s_A | s_B s_B) (T = alpha_w R^2) and (s_A s_B | s_A s_B) of unnormalised primitives over the T list at
    omega = 1e3, and over 1 / r12 as the limit omega = 1e30 of the closed form (1 / omega^2 below 1e-59 of p + q)."""
    worst = 0.0
    for t in mpr.SWEEP_T:
        r = mpr.sweep_distance(t)
        a = mpr.Shell(0, (0.0, 0.0, 0.0), (1.0,), (1.0,), ((1.0,),))
        b = mpr.Shell(0, (0.0, 0.0, r), (1.0,), (1.0,), ((1.0,),))
        for quartet in ((a, a, b, b), (a, b, a, b), (a, a, a, b)):
            for omega, omega_closed in ((1e3, 1e3), (None, 1e30)):
                ld, _, scale = _quartet_three_ways(quartet, omega)
                with mp.workdps(mpr.MP_DPS):
                    exact = er.ssss_closed_form([s.exps[0] for s in quartet], [s.centre for s in quartet], omega_closed,
                                                dps=mpr.MP_DPS)
                    if exact < mp.mpf(10) ** -4900:  # below the longdouble range: both are zero
                        assert float(ld.ravel()[0]) == 0.0
                        continue
                    worst = max(worst, _mpf_ratio(ld, np.array([exact], dtype=object), scale))
    print(f"worst |longdouble - closed form| = {worst:.3g} EPS A-bar")
    assert worst <= CERTIFY


def test_sampled_elements_of_every_class_agree_with_the_oracle():
    """``oracle.gto`` normalises the functions itself and evaluates E and R by scalar recursions with scipy's hyp1f1:
    nothing shared with the reference but the formulas' source.  Its own tolerance, 1e-12."""
    case = mpr.eri_case("generic")
    ob = oracle_gto.SphericalBasis(oracle_gto.parse_xyz(mpr.GENERIC_XYZ), mpr.GENERIC_TABLE)
    assert ob.nao == case.basis.nao
    l = mpr.ao_ang(case.shells)
    lab = l[:, None] + l[None, :]
    rng = np.random.default_rng(20261021)
    picks = []
    for x in range(5):
        for y in range(5):  # one two-centre element of each class, the largest of eight drawn
            bra, ket = np.argwhere(lab == x), np.argwhere(lab == y)
            drawn = [(*bra[rng.integers(len(bra))], *ket[rng.integers(len(ket))]) for _ in range(8)]
            picks.append(max(drawn, key=lambda e: abs(float(case.ref[e]))))
    picks += [tuple(rng.integers(0, case.basis.nao, 4)) for _ in range(15)]
    ref = np.asarray(case.ref, dtype=np.float64)
    worst = 0.0
    for p, q, r, s in picks:
        want = oracle_gto.eri_element_general(ob, int(p), int(q), int(r), int(s))
        worst = max(worst, abs(ref[p, q, r, s] - want))
        assert abs(ref[p, q, r, s] - want) <= 1e-12, (p, q, r, s)
    assert len(picks) == 40 and max(abs(ref[e]) for e in picks[:25]) > 1e-3
    print(f"40 elements: max |reference - oracle| = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 2. the host engines
def _host_mm(case):
    lib = _nbx.load_library()
    arrays = integrals._shell_arrays(case.basis)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    q, xyz = np.ascontiguousarray(case.charges), np.ascontiguousarray(case.coords)
    zetas = None if case.zetas is None else np.ascontiguousarray(case.zetas)
    out = np.empty((case.basis.nao,) * 2)
    _nbx.check(lib, lib.nbx_host_mm_potential(len(case.basis.shells), *(ptr(a) for a in arrays), len(q), ptr(q), ptr(xyz),
                                              ptr(zetas), 2, ptr(out)))
    return out


def _report(label, case, got, what):
    r_got, r_twin = mpr.ratios(got, case.ref, case.scale), mpr.ratios(case.twin, case.ref, case.scale)
    print(f"{label}: nao = {case.basis.nao}, K = {case.k:.3g}, worst {what} = {r_got.max():.3g}, worst twin = "
          f"{r_twin.max():.3g} (units of EPS A-bar)")
    print(mpr.format_classes(f"{what}, per class", mpr.worst_per_class(r_got, case.shells)))
    print(mpr.format_classes("twin, per class", mpr.worst_per_class(r_twin, case.shells)))
    return r_got


@pytest.mark.parametrize("label", list(mpr.ERI_CASES))
def test_host_eri_within_the_bound(label):
    case = mpr.eri_case(label)
    assert 18 <= case.basis.nao <= 20 and case.k >= mpr.MARGIN and np.isfinite(case.k)
    got = integrals.two_electron_native(case.basis, nthreads=4, cutoff=0.0, omega=case.omega)
    r = _report(label, case, got, "host")
    bad = mpr.violations(got, case.ref, case.scale, case.k)
    assert len(bad) == 0, (len(bad), bad[:5], r.max())
    assert r.max() > 0  # something was compared


@pytest.mark.parametrize("label", list(mpr.MM_CASES))
def test_host_mm_potential_within_the_bound(label):
    case = mpr.mm_case(label)
    assert case.k >= mpr.MARGIN and np.isfinite(case.k)
    got = _host_mm(case)
    r = _report(label, case, got, "host")
    bad = mpr.violations(got, case.ref, case.scale, case.k)
    assert len(bad) == 0, (len(bad), bad[:5], r.max())
    assert r.max() > 0 and np.abs(got).max() > 1e-3


def test_the_charges_of_the_near_set_are_where_the_issue_puts_them():
    q, xyz, _ = mpr.MM_CASES["near-points"]
    atoms = integrals.parse_geometry(mpr.GENERIC_XYZ)
    o, c = atoms[0][1], atoms[1][1]
    xyz = np.array(xyz)
    assert np.array_equal(xyz[0], o) and abs(np.linalg.norm(xyz[1] - o) - 1e-5) < 1e-12
    assert np.allclose(3.6 * np.sum((xyz[2:4] - c) ** 2, axis=1), [40.9999, 41.0001], rtol=1e-14, atol=0)
    assert all(np.linalg.norm(p - o) < 4.0 or np.linalg.norm(p - c) < 4.0 for p in xyz)
    assert min(q) < 0 < max(q) and len(q) == 8
    assert all(np.linalg.norm(p) >= 60.0 for p in mpr.MM_CASES["far-points"][1])
    top = max(a + b for sh in mpr.shells_of(mpr.case_basis("generic")) for a in sh.exps for b in sh.exps)
    assert top == 3.6


# ------------------------------------------------------------------------------------------------ 3. sensitivity
class TableBoys:
    """The engines' Boys evaluation restated from its description: a table of F_0 .. F_22 at T = 0, 0.1, .. 42 (the top
    order from the series exp(-T) sum_k (2T)^k / ((2n+1)(2n+3) .. (2n+2k+1)), the others by downward recursion); F_L(T)
    from ``terms`` Taylor terms about the nearest node, F_L(T) = sum_k F_(L+k)(T0) (T0 - T)^k / k!, and downward recursion
    below it; from T >= ``switch`` on F_0 = sqrt(pi / T) / 2 and the upward recursion."""

    STEP, NT, NORD = 0.1, 421, 22

    def __init__(self, terms=9, switch=41.0):
        self.terms, self.switch = terms, switch
        t = np.arange(self.NT) * self.STEP
        n = self.NORD
        term = np.full_like(t, 1.0 / (2 * n + 1))
        top = term.copy()
        for k in range(1, 400):
            term = term * (2.0 * t / (2 * n + 2 * k + 1))
            top = top + term
        et = np.exp(-t)
        self.table = np.empty((self.NT, n + 1))
        self.table[:, n] = et * top
        for m in range(n, 0, -1):
            self.table[:, m - 1] = (2.0 * t * self.table[:, m] + et) / (2 * m - 1)

    def __call__(self, big_l, t):
        t = np.asarray(t, dtype=np.float64)
        out = np.empty((big_l + 1,) + t.shape)
        far = t >= self.switch
        et = np.exp(-t)
        tf = np.where(far, t, 1.0)
        up = [0.5 * np.sqrt(np.pi / tf)]
        for m in range(big_l):
            up.append(((2 * m + 1) * up[m] - et) / (2.0 * tf))
        tn = np.where(far, 0.0, t)
        node = np.floor(tn / self.STEP + 0.5).astype(np.int64)
        d = node * self.STEP - tn
        acc, pw = np.zeros_like(t), np.ones_like(t)
        for k in range(self.terms):
            acc = acc + self.table[node, big_l + k] * pw
            pw = pw * d / (k + 1)
        down = [None] * (big_l + 1)
        down[big_l] = acc
        for m in range(big_l, 0, -1):
            down[m - 1] = (2.0 * tn * down[m] + np.exp(-tn)) / (2 * m - 1)
        for m in range(big_l + 1):
            out[m] = np.where(far, up[m], down[m])
        return out


SENSITIVITY_T = mpr.SWEEP_T + (30.0,)  # 30: between a switch moved to 25 and the one at 41


def _sweep_with(t, **twin_args):
    case = mpr.eri_case((("sweep", mpr.sweep_distance(t)), None))
    got = mpr.eri_tensor_with(case.shells, None, **twin_args)
    return mpr.ratios(got, case.ref, case.scale).max(), case.k


def test_the_restated_table_boys_passes_every_sweep_case():
    for t in SENSITIVITY_T:
        worst, k = _sweep_with(t, boys=TableBoys())
        print(f"T = {t:g}: table-based Boys in the twin: {worst:.3g} of K = {k:.3g}")
        assert 0 < worst <= k


def test_six_taylor_terms_fail_at_half_a_table_step():
    worst, k = _sweep_with(0.05, boys=TableBoys(terms=6))
    print(f"T = 0.05, six Taylor terms: {worst:.3g} against K = {k:.3g}")
    assert worst > k


def test_a_switch_at_25_fails_at_30():
    worst, k = _sweep_with(30.0, boys=TableBoys(switch=25.0))
    print(f"T = 30, asymptotic branch from 25: {worst:.3g} against K = {k:.3g}")
    assert worst > k


def test_a_ket_sign_dropped_from_one_index_fails_the_generic_case():
    case = mpr.eri_case("generic")
    got = mpr.eri_tensor_with(case.shells, None, ket_sign_axes=(0, 1))  # (-1)^(tau + nu), phi forgotten
    r = mpr.ratios(got, case.ref, case.scale)
    print(f"generic, sign of phi dropped: {r.max():.3g} against K = {case.k:.3g}; {int((r > case.k).sum())} elements outside")
    assert r.max() > case.k
    same = mpr.eri_tensor_with(case.shells, None)
    np.testing.assert_array_equal(same, case.twin)  # the variant run is the twin when nothing is changed
