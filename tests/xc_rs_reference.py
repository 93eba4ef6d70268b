"""Extended-precision reference for the range-separated hybrids ``cam-b3lyp`` and ``lc-blyp`` (their semi-local parts): the
companion of tests/xc_reference.py and tests/xc_gga_reference.py, whose pieces, regimes, conventions and error measure
are reused.  Nothing here is imported from ``nbed_amd``.

  B88^sr       per spin channel (Iikura, Tsuneda, Yanai and Hirao, J. Chem. Phys. 115, 3540 (2001)): with the whole B88
               exchange of the channel, e = -cx rho^(4/3) - beta rho^(4/3) g(x) = -1/2 rho^(4/3) K,
                   k = sqrt(9 pi / K) rho^(1/3),   a = omega / (2 k),   e_sr = e F(a),
                   F(a) = 1 - (8/3) a [sqrt(pi) erf(1 / (2a)) + 2a (b - c)],  b = exp(-1 / (4 a^2)) - 1,  c = 2 a^2 b + 1/2
  cam-b3lyp    (1 - alpha - beta) (Slater + B88) + beta B88^sr(omega) + 0.81 LYP + 0.19 VWN5, alpha = 0.19, beta = 0.46,
               omega = 0.33 (Yanai, Tew and Handy, Chem. Phys. Lett. 393, 51 (2004))
  lc-blyp      B88^sr(omega) + LYP, omega = 0.33

F enters the sympy expressions as an opaque function ``ityh_F`` (derivative ``ityh_dF``).  At 50 digits both are the
closed form, evaluated with 64 + 4 log2(a) more bits because the closed form cancels (its bracket tends to 3/8 while F
falls like 1 / (36 a^2): 36 a^4 ulp are lost, 58 bits at a = 1e4).  The reference's own 53-bit evaluation -- the figure the loose
regimes are bounded by -- uses the branch rule a float64 evaluation needs: the closed form below ``SWITCH``, the series

    F = sum_{m >= 1} c_m t^m,  t = 1 / (4 a^2),  c_m = -(8/3) (-1)^m [1 / (m! (2m + 1)) - 1 / (2 (m + 1)!) - 1 / (4 (m + 2)!)]

from there on.  ``series_coefficient`` is that formula; ``series_coefficients_from_the_closed_form`` derives the same
numbers from the closed form alone (sympy's expansion in t), and ``branch_errors`` measures both branches in 53 bits
against the 50-digit value, which is how the switch point was chosen.
"""

from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import mpmath as mp
import numpy as np
import sympy as sp

import xc_gga_reference as xg
import xc_reference as xr

RA, RB, SAA, SAB, SBB = VARS = xr.VARS
FUNCTIONALS = ("cam-b3lyp", "lc-blyp")
OMEGA = sp.Rational(33, 100)
ALPHA, BETA = sp.Rational(19, 100), sp.Rational(46, 100)
POINTS_PER_REGIME = 64
SWITCH = 0.5      # a from which a float64 evaluation sums the series
SERIES_TERMS = 16
ENTRY_BOUND, SUM_BOUND = xr.ENTRY_BOUND, xr.SUM_BOUND
LOOSE_REGIMES = xg.LOOSE_REGIMES
_THIRD = sp.Rational(1, 3)


# ------------------------------------------------------------------------------------------ the attenuation factor
def _closed_f(a):
    b = mp.expm1(-1 / (4 * a * a))
    c = 2 * a * a * b + mp.mpf(1) / 2
    return 1 - mp.mpf(8) / 3 * a * (mp.sqrt(mp.pi) * mp.erf(1 / (2 * a)) + 2 * a * (b - c))


def _closed_df(a):
    """dF/da of the closed form, term by term: -(8/3) [sqrt(pi) erf(1 / (2a)) + 2 a b - 16 a^3 b - 4 a]."""
    b = mp.expm1(-1 / (4 * a * a))
    return -mp.mpf(8) / 3 * (mp.sqrt(mp.pi) * mp.erf(1 / (2 * a)) + 2 * a * b - 16 * a ** 3 * b - 4 * a)


def series_coefficient(m: int) -> Fraction:
    f = math.factorial
    return Fraction(-8, 3) * (-1) ** m * (Fraction(1, f(m) * (2 * m + 1)) - Fraction(1, 2 * f(m + 1)) - Fraction(1, 4 * f(m + 2)))


def series_coefficients_from_the_closed_form(n: int):
    """c_0 .. c_n of F as a power series in t = 1 / (4 a^2), from sympy's expansion of the closed form (a = 1 / (2 sqrt t))."""
    t = sp.Symbol("t", positive=True)
    a = 1 / (2 * sp.sqrt(t))
    b = sp.exp(-t) - 1
    c = 2 * a * a * b + sp.Rational(1, 2)
    f = 1 - sp.Rational(8, 3) * a * (sp.sqrt(sp.pi) * sp.erf(sp.sqrt(t)) + 2 * a * (b - c))
    ser = sp.series(sp.expand(f), t, 0, n + 1).removeO()
    return [sp.nsimplify(sp.simplify(ser.coeff(t, m))) for m in range(n + 1)]


def _series_f(a):
    t = 1 / (4 * a * a)
    s = mp.mpf(0)
    for m in range(SERIES_TERMS, 0, -1):
        c = series_coefficient(m)
        s = (s + mp.mpf(c.numerator) / c.denominator) * t
    return s


def _series_df(a):
    t = 1 / (4 * a * a)
    s = mp.mpf(0)
    for m in range(SERIES_TERMS, 0, -1):
        c = series_coefficient(m)
        s = (s + m * mp.mpf(c.numerator) / c.denominator) * t
    return -2 * s / a


def _guarded(fn, a):
    """The closed form ``fn`` at ``a`` to the working precision: 36 a^4 ulp are lost, so 64 + 4 log2(a) guard bits."""
    a = mp.mpf(a)
    extra = 64 + max(0, 4 * int(mp.ceil(mp.log(a, 2))) + 8)
    with mp.workprec(mp.mp.prec + extra):
        out = fn(a)
    return +out


def f_exact(a):
    """F(a) to the working precision."""
    return mp.mpf(1) if a == 0 else _guarded(_closed_f, a)


def df_exact(a):
    return -mp.mpf(8) / 3 * mp.sqrt(mp.pi) if a == 0 else _guarded(_closed_df, a)


def f_branched(a):
    """F(a) in the working precision with the branch rule of a float64 evaluation."""
    return _series_f(a) if a >= SWITCH else (_closed_f(a) if a > 0 else mp.mpf(1))


def df_branched(a):
    return _series_df(a) if a >= SWITCH else (_closed_df(a) if a > 0 else -mp.mpf(8) / 3 * mp.sqrt(mp.pi))


def branch_errors(a: float):
    """(closed F, closed a F', series F, series a F'): relative errors of the two branches in 53-bit arithmetic."""
    with mp.workdps(xr.DPS):
        f, h = f_exact(mp.mpf(a)), mp.mpf(a) * df_exact(mp.mpf(a))
    with mp.workprec(53):
        am = mp.mpf(a)
        got = (_closed_f(am), am * _closed_df(am), _series_f(am), am * _series_df(am))
    with mp.workdps(xr.DPS):
        return tuple(float(abs(g - w) / abs(w)) for g, w in zip(got, (f, h, f, h)))


class ityh_dF(sp.Function):
    """dF/da, opaque (first derivatives of the energy are all that is asked for)."""


class ityh_F(sp.Function):
    def fdiff(self, argindex=1):
        return ityh_dF(self.args[0])


# ------------------------------------------------------------------------------------------ energy densities
def b88_total_enhancement(x):
    """G(x) of the whole B88 exchange of a channel, e = -rho^(4/3) G: the Slater constant plus beta g(x)."""
    cx = sp.Rational(3, 2) * (3 / (4 * sp.pi)) ** _THIRD
    return cx + xr._q("0.0042") * xr.b88_enhancement(x)


def ityh_a(r, s, omega):
    """a = omega / (2 k), k = sqrt(9 pi / K) rho^(1/3), K = 2 G."""
    k_big = 2 * b88_total_enhancement(sp.sqrt(s) / r ** (4 * _THIRD))
    return omega / (2 * sp.sqrt(9 * sp.pi / k_big) * r ** _THIRD)


def b88_sr_channel_expr(r, s, omega):
    r43 = r ** (4 * _THIRD)
    return -r43 * b88_total_enhancement(sp.sqrt(s) / r43) * ityh_F(ityh_a(r, s, omega))


def _rational(omega) -> sp.Rational:
    return omega if isinstance(omega, sp.Rational) else sp.Rational(*Fraction(float(omega)).as_integer_ratio())


@lru_cache(maxsize=None)
def _piece_expr(label: str, omega: sp.Rational):
    if label == "b88sr_a":
        return b88_sr_channel_expr(RA, SAA, omega)
    if label == "b88sr_b":
        return b88_sr_channel_expr(RB, SBB, omega)
    return xg._piece_expr(label)


def pieces(name: str):
    """[(coefficient, label)] of the semi-local part of ``name``."""
    one = sp.Integer(1)
    if name == "lc-blyp":
        return [(one, "b88sr_a"), (one, "b88sr_b"), (one, "lyp")]
    if name == "cam-b3lyp":
        full = 1 - ALPHA - BETA
        return [(full, "slater_a"), (full, "slater_b"), (full, "b88_a"), (full, "b88_b"), (BETA, "b88sr_a"), (BETA, "b88sr_b"),
                (sp.Rational(19, 100), "vwn5"), (sp.Rational(81, 100), "lyp")]
    raise ValueError(name)


@lru_cache(maxsize=None)
def _compiled(label: str, stable: bool, omega: sp.Rational):
    if not label.startswith("b88sr"):
        return xg._compiled(label, stable)
    e = _piece_expr(label, omega)
    outs = [e] + [sp.diff(e, v) for v in VARS]
    fns = {"ityh_F": f_branched, "ityh_dF": df_branched} if stable else {"ityh_F": f_exact, "ityh_dF": df_exact}
    return sp.lambdify(VARS, outs, modules=[fns, "mpmath"], cse=True)


def point(name: str, ra, rb, saa, sab, sbb, omega=OMEGA):
    """(e, de/dra, de/drb, de/dsaa, de/dsab, de/dsbb) of a functional at one point, mpf at 50 digits."""
    omega = _rational(omega)
    with mp.workdps(xr.DPS):
        args = [mp.mpf(v) for v in (ra, rb, saa, sab, sbb)]
        out = [mp.mpf(0)] * 6
        for c, label in pieces(name):
            cm = mp.mpf(c.p) / mp.mpf(c.q)
            out = [o + cm * mp.mpf(v) for o, v in zip(out, _compiled(label, False, omega)(*args))]
        return tuple(out)


# ------------------------------------------------------------------------------------------ the product's conventions
def _evaluate(name, rho, grad, w, floor, stable, omega):
    """xg._evaluate for the names of FUNCTIONALS: totals and, per entry, the sum of the magnitudes of the pieces."""
    npts = rho.shape[1]
    zero = mp.mpf(0)
    vr, vec = np.full((2, npts), zero, dtype=object), np.full((2, 3, npts), zero, dtype=object)
    mvr, mvec = np.full((2, npts), zero, dtype=object), np.full((2, 3, npts), zero, dtype=object)
    keep = np.zeros(npts, dtype=bool)
    half, tiny, fl = mp.mpf(float(floor)) / 2, mp.mpf(1e-40), mp.mpf(float(floor))
    exc = mexc = nelec = zero
    parts = [(mp.mpf(c.p) / mp.mpf(c.q), _compiled(label, stable, omega)) for c, label in pieces(name)]
    for g in range(npts):
        r0, r1, wg = mp.mpf(float(rho[0, g])), mp.mpf(float(rho[1, g])), mp.mpf(float(w[g]))
        ga = [mp.mpf(float(grad[0, a, g])) for a in range(3)]
        gb = [mp.mpf(float(grad[1, a, g])) for a in range(3)]
        nelec += wg * (r0 + r1)
        if not r0 + r1 > fl:
            continue
        keep[g] = True
        saa = sum(x * x for x in ga) + tiny
        sbb = sum(x * x for x in gb) + tiny
        sab = sum(x * y for x, y in zip(ga, gb))
        args = (max(r0, half), max(r1, half), saa, sab, sbb)
        for c, fn in parts:
            e, va, vb, vaa, vab, vbb = (wg * c * mp.mpf(v) for v in fn(*args))
            exc += e
            mexc += abs(e)
            vr[0, g] += va
            vr[1, g] += vb
            mvr[0, g] += abs(va)
            mvr[1, g] += abs(vb)
            for a in range(3):
                ea, eb = 2 * vaa * ga[a] + vab * gb[a], 2 * vbb * gb[a] + vab * ga[a]
                vec[0, a, g] += ea
                vec[1, a, g] += eb
                mvec[0, a, g] += abs(ea)
                mvec[1, a, g] += abs(eb)
    return vr, vec, exc, nelec, keep, (mvr, mvec, mexc)


def functional_reference(name: str, rho, grad, w, floor: float, omega=OMEGA):
    """``xg.functional_reference`` for ``cam-b3lyp`` and ``lc-blyp`` at the range separation ``omega``: the same tuple
    ``(vr, vec, exc, nelec, keep, mag, own)``, so xg.check_functional, xg.own_error and xg.entry_bound apply to it."""
    rho, grad, w = (np.asarray(x, dtype=np.float64) for x in (rho, grad, w))
    omega = _rational(omega)
    with mp.workdps(xr.DPS):
        vr, vec, exc, nelec, keep, mag = _evaluate(name, rho, grad, w, floor, False, omega)
    with mp.workprec(53):
        vr53, vec53, exc53, _, keep53, _ = _evaluate(name, rho, grad, w, floor, True, omega)
    assert np.array_equal(keep, keep53)
    with mp.workdps(xr.DPS):
        e_exc = float(abs(exc53 - exc) / max(mag[2], mp.mpf(1e-150)))
    own = (xg.scaled_err(vr53, vr, mag[0]), xg.scaled_err(vec53, vec, mag[1]), e_exc)
    return vr, vec, exc, nelec, keep, mag, own


def regime_inputs(regime: str, floor: float):
    return xr.regime_inputs(regime, floor, n=POINTS_PER_REGIME)


@lru_cache(maxsize=None)
def regime_reference(name: str, regime: str, floor: float):
    return functional_reference(name, *regime_inputs(regime, floor), floor)


# ------------------------------------------------------------------------------------------ points at chosen a
# (label, omega, a of the alpha channel): either side of the switch at the functionals' own omega, and the two ends a
# user's omega can reach -- a = 1e-6 (F = 1 - 3e-6) and a = 1e4 (F = 2.8e-10, where the closed form is noise)
A_CASES = (("below_switch", 0.33, SWITCH * (1 - 2.0 ** -20)), ("above_switch", 0.33, SWITCH * (1 + 2.0 ** -20)),
           ("a_1e-6", 1e-5, 1e-6), ("a_1e4", 1e3, 1e4))
POINTS_PER_A_CASE = 16


def a_case_inputs(label: str):
    """``(omega, rho, grad, w)``: points whose alpha channel has the case's a (to rounding) at reduced gradients over
    1e-2 .. 1e2, the beta channel within a factor of two of it: rho = (omega sqrt(2 G(x)) / (6 sqrt(pi) a))^3."""
    idx = [c[0] for c in A_CASES].index(label)
    _, omega, a_t = A_CASES[idx]
    rng = np.random.default_rng(4000 + idx)
    n = POINTS_PER_A_CASE
    rho, grad = np.empty((2, n)), np.empty((2, 3, n))
    for ch, target in enumerate((np.full(n, a_t), a_t * 2.0 ** rng.uniform(-1, 1, n))):
        x = 10 ** rng.uniform(-2, 2, n)
        big_g = 0.9305257363491 + 0.0042 * x * x / (1 + 6 * 0.0042 * x * np.arcsinh(x))
        rho[ch] = (omega * np.sqrt(2 * big_g) / (6 * math.sqrt(math.pi) * target)) ** 3
        d = rng.normal(size=(3, n))
        grad[ch] = d / np.linalg.norm(d, axis=0) * x * rho[ch] ** (4 / 3)
    return omega, rho, grad, rng.uniform(0.1, 2.0, n)


@lru_cache(maxsize=None)
def a_case_reference(name: str, label: str, floor: float):
    omega, rho, grad, w = a_case_inputs(label)
    return functional_reference(name, rho, grad, w, floor, omega)


def channel_a(rho, grad, omega):
    """a of both channels at 50 digits -> float (2, G): what the tests assert the cases reach."""
    out = np.empty(rho.shape)
    fn = sp.lambdify((RA, SAA), ityh_a(RA, SAA, _rational(omega)), modules="mpmath")
    with mp.workdps(xr.DPS):
        for ch in range(2):
            for g in range(rho.shape[1]):
                s = sum(mp.mpf(float(v)) ** 2 for v in grad[ch, :, g]) + mp.mpf(1e-40)
                out[ch, g] = float(fn(mp.mpf(float(rho[ch, g])), s))
    return out
