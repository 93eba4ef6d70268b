"""Extended-precision references for the functionals built on PBE exchange, PW92 and PBE correlation, and for the
recombinations of the older pieces (``blyp``, ``b3lyp5``) -- the companion of tests/xc_reference.py, whose pieces,
regimes and conventions are reused.  Nothing here is imported from ``nbed_amd``.

  PBE exchange   per spin channel e_s = -cx rho_s^(4/3) F(s^2),  s^2 = sigma_ss / (4 (6 pi^2)^(2/3) rho_s^(8/3)),
                 F = 1 + kappa - kappa / (1 + mu s^2 / kappa),  kappa = 0.804,  mu = beta pi^2 / 3,
                 beta = 0.06672455060314922  (Perdew, Burke and Ernzerhof, Phys. Rev. Lett. 77, 3865 (1996), eqs. 10-14,
                 spin-scaled; libxc GGA_X_PBE)
  PW92           e = n eps(r_s, zeta),  eps = eps_0 + alpha_c f(zeta) / f''(0) (1 - zeta^4) + (eps_1 - eps_0) f(zeta) zeta^4,
                 G = -2A (1 + a1 r_s) ln(1 + 1 / (2A (b1 r_s^(1/2) + b2 r_s + b3 r_s^(3/2) + b4 r_s^2)))  (Perdew and Wang,
                 Phys. Rev. B 45, 13244 (1992), eqs. 8-10 and table I, with f''(0) = 4 / (9 (2^(1/3) - 1)) exact and A to
                 seven digits: libxc LDA_C_PW_MOD)
  PBE correlation  e = n (eps + H),  H = gamma phi^3 ln(1 + (beta / gamma) t^2 (1 + y) / (1 + y + y^2)),  y = A t^2,
                 A = (beta / gamma) / (exp(-eps / (gamma phi^3)) - 1),  gamma = (1 - ln 2) / pi^2,
                 phi = ((1 + zeta)^(2/3) + (1 - zeta)^(2/3)) / 2,  t^2 = sigma / (4 phi^2 k_s^2 n^2),  k_s^2 = 4 k_F / pi,
                 k_F = (3 pi^2 n)^(1/3)  (PBE eqs. 3, 7, 8; libxc GGA_C_PBE)

  lda,pw_mod = Slater + PW92;  pbe = PBE_X + PBE_C;  pbeh = 0.75 PBE_X + PBE_C;  blyp = Slater + B88 + LYP;
  b3lyp5 = 0.8 Slater + 0.72 B88 + 0.19 VWN5 + 0.81 LYP  (the semi-local parts)

A potential is a sum of pieces of either sign (at a large reduced gradient eps and H cancel to 1e-5 of their size), so
errors are measured against the sum of the MAGNITUDES of the pieces' exact contributions to an entry -- each exchange
channel, the eps part, the H part, B88 per channel, LYP, VWN.  ``functional_reference`` returns those sums, and the
error of its own expressions evaluated in 53-bit arithmetic (with expm1 / log1p where the formulas above have
exp(.) - 1 and ln(1 + .)): what a float64 evaluation of the textbook formulas can be asked to deliver.
"""

from __future__ import annotations

import math
from functools import lru_cache

import mpmath as mp
import numpy as np
import sympy as sp

import xc_reference as xr

RA, RB, SAA, SAB, SBB = VARS = xr.VARS
FUNCTIONALS = ("lda,pw_mod", "pbe", "pbeh", "blyp", "b3lyp5")
POINTS_PER_REGIME = 64
LOOSE_REGIMES = ("tails", "at_floor")  # the two whose bound follows the reference's own 53-bit evaluation
ENTRY_BOUND, SUM_BOUND = xr.ENTRY_BOUND, xr.SUM_BOUND

_q = xr._q
_THIRD = sp.Rational(1, 3)
KAPPA = _q("0.804")
BETA = _q("0.06672455060314922")
MU = BETA * sp.pi ** 2 / 3
GAMMA = (1 - sp.log(2)) / sp.pi ** 2


class xexpm1(sp.Function):
    """exp(x) - 1, kept as one function so that the 53-bit evaluation can call mpmath.expm1."""

    @classmethod
    def eval(cls, x):
        if x.is_zero:
            return sp.Integer(0)

    def fdiff(self, argindex=1):
        return sp.exp(self.args[0])


class xlog1p(sp.Function):
    """ln(1 + x), kept as one function so that the 53-bit evaluation can call mpmath.log1p."""

    @classmethod
    def eval(cls, x):
        if x.is_zero:
            return sp.Integer(0)

    def fdiff(self, argindex=1):
        return 1 / (1 + self.args[0])


def _expm1(x, stable):
    return xexpm1(x) if stable else sp.exp(x) - 1


def _log1p(x, stable):
    return xlog1p(x) if stable else sp.log(1 + x)


# ------------------------------------------------------------------------------------------ energy densities
def pbe_enhancement(s2):
    """F(s^2) of e_s = -cx rho_s^(4/3) F."""
    return 1 + KAPPA - KAPPA / (1 + MU * s2 / KAPPA)


def pbe_x_channel_expr(r, s):
    cx = sp.Rational(3, 2) * (3 / (4 * sp.pi)) ** _THIRD
    s2 = s / (4 * (6 * sp.pi ** 2) ** (2 * _THIRD) * r ** (8 * _THIRD))
    return -cx * r ** (4 * _THIRD) * pbe_enhancement(s2)


def pbe_x_expr(ra=RA, rb=RB, saa=SAA, sbb=SBB):
    return pbe_x_channel_expr(ra, saa) + pbe_x_channel_expr(rb, sbb)


def _pw_g(rs, a, a1, b1, b2, b3, b4, stable):
    a, a1, b1, b2, b3, b4 = (_q(v) for v in (a, a1, b1, b2, b3, b4))
    q1 = 2 * a * (b1 * sp.sqrt(rs) + b2 * rs + b3 * rs ** sp.Rational(3, 2) + b4 * rs ** 2)
    return -2 * a * (1 + a1 * rs) * _log1p(1 / q1, stable)


def pw_eps_expr(ra=RA, rb=RB, stable=False):
    """eps(r_s, zeta); 1 +- zeta formed as 2 rho_s / rho and 1 - zeta^4 as the product of its factors."""
    rho = ra + rb
    rs = (3 / (4 * sp.pi * rho)) ** _THIRD
    up, dn = 2 * ra / rho, 2 * rb / rho
    zeta = (ra - rb) / rho
    fz = (up ** (4 * _THIRD) + dn ** (4 * _THIRD) - 2) / (2 ** (4 * _THIRD) - 2)
    fpp0 = sp.Rational(4, 9) / (2 ** _THIRD - 1)
    e0 = _pw_g(rs, "0.0310907", "0.21370", "7.5957", "3.5876", "1.6382", "0.49294", stable)
    e1 = _pw_g(rs, "0.01554535", "0.20548", "14.1189", "6.1977", "3.3662", "0.62517", stable)
    alpha_c = -_pw_g(rs, "0.0168869", "0.11125", "10.357", "3.6231", "0.88026", "0.49671", stable)
    return e0 + alpha_c * fz / fpp0 * (up * dn * (1 + zeta ** 2)) + (e1 - e0) * fz * zeta ** 4


def pw_mod_expr(ra=RA, rb=RB, stable=False):
    return (ra + rb) * pw_eps_expr(ra, rb, stable)


def pbe_h_expr(ra=RA, rb=RB, saa=SAA, sab=SAB, sbb=SBB, stable=False):
    """H(r_s, zeta, t) per electron."""
    rho = ra + rb
    up, dn = 2 * ra / rho, 2 * rb / rho
    phi = (up ** (2 * _THIRD) + dn ** (2 * _THIRD)) / 2
    kf = (3 * sp.pi ** 2 * rho) ** _THIRD
    t2 = (saa + 2 * sab + sbb) / (4 * phi ** 2 * (4 * kf / sp.pi) * rho ** 2)
    a = (BETA / GAMMA) / _expm1(-pw_eps_expr(ra, rb, stable) / (GAMMA * phi ** 3), stable)
    y = a * t2
    return GAMMA * phi ** 3 * _log1p(BETA / GAMMA * t2 * (1 + y) / (1 + y + y * y), stable)


def pbe_c_expr(ra=RA, rb=RB, saa=SAA, sab=SAB, sbb=SBB, stable=False):
    return (ra + rb) * (pw_eps_expr(ra, rb, stable) + pbe_h_expr(ra, rb, saa, sab, sbb, stable))


def _b88_channel_expr(r, s):
    r43 = r ** (4 * _THIRD)
    return -_q("0.0042") * r43 * xr.b88_enhancement(sp.sqrt(s) / r43)


@lru_cache(maxsize=None)
def _piece_expr(label: str, stable: bool = False):
    """One piece of a potential: an expression in xr.VARS."""
    if label == "slater_a":
        return xr.slater_expr(RA, 0)
    if label == "slater_b":
        return xr.slater_expr(0, RB)
    if label == "b88_a":
        return _b88_channel_expr(RA, SAA)
    if label == "b88_b":
        return _b88_channel_expr(RB, SBB)
    if label == "lyp":
        return xr.lyp_expr()
    if label == "vwn5":
        return xr.vwn5_expr()
    if label == "vwn_rpa":
        return xr.vwn_rpa_expr()
    if label == "pbe_x_a":
        return pbe_x_channel_expr(RA, SAA)
    if label == "pbe_x_b":
        return pbe_x_channel_expr(RB, SBB)
    if label == "pw_mod":
        return pw_mod_expr(stable=stable)
    if label == "pbe_h":
        return (RA + RB) * pbe_h_expr(stable=stable)
    raise ValueError(label)


def pieces(name: str):
    """[(coefficient, label)] of the semi-local part of ``name``."""
    one = sp.Integer(1)
    if name == "lda,pw_mod":
        return [(one, "slater_a"), (one, "slater_b"), (one, "pw_mod")]
    if name in ("pbe", "pbeh"):
        cx = one if name == "pbe" else sp.Rational(3, 4)
        return [(cx, "pbe_x_a"), (cx, "pbe_x_b"), (one, "pw_mod"), (one, "pbe_h")]
    if name == "blyp":
        return [(one, "slater_a"), (one, "slater_b"), (one, "b88_a"), (one, "b88_b"), (one, "lyp")]
    if name in ("b3lyp5", "b3lyp"):
        s, b, v, c = sp.Rational(8, 10), sp.Rational(72, 100), sp.Rational(19, 100), sp.Rational(81, 100)
        return [(s, "slater_a"), (s, "slater_b"), (b, "b88_a"), (b, "b88_b"),
                (v, "vwn5" if name == "b3lyp5" else "vwn_rpa"), (c, "lyp")]
    raise ValueError(name)


def energy_density_expr(name: str, stable: bool = False):
    return sum(c * _piece_expr(label, stable) for c, label in pieces(name))


@lru_cache(maxsize=None)
def _compiled(label: str, stable: bool = False):
    """(e, de/dra, de/drb, de/dsaa, de/dsab, de/dsbb) of one piece as an mpmath function, as xr._compiled builds it."""
    e = _piece_expr(label, stable)
    outs = [e] + [sp.diff(e, v) for v in VARS]
    return sp.lambdify(VARS, outs, modules=[{"xexpm1": mp.expm1, "xlog1p": mp.log1p}, "mpmath"], cse=True)


def point(name: str, ra, rb, saa, sab, sbb):
    """(e, de/dra, de/drb, de/dsaa, de/dsab, de/dsbb) of a functional at one point, mpf at 50 digits."""
    with mp.workdps(xr.DPS):
        args = [mp.mpf(v) for v in (ra, rb, saa, sab, sbb)]
        out = [mp.mpf(0)] * 6
        for c, label in pieces(name):
            cm = mp.mpf(c.p) / mp.mpf(c.q)
            out = [o + cm * mp.mpf(v) for o, v in zip(out, _compiled(label)(*args))]
        return tuple(out)


# ------------------------------------------------------------------------------------------ the product's conventions
_POINT_CACHE: dict = {}


def _piece_at(label, stable, args):
    """One piece at one point in the working precision; remembered, because the functionals share their pieces and
    the tests share their points."""
    key = (label, stable, mp.mp.prec, args)
    hit = _POINT_CACHE.get(key)
    if hit is None:
        hit = _POINT_CACHE[key] = tuple(mp.mpf(v) for v in _compiled(label, stable)(*args))
    return hit


def _evaluate(name, rho, grad, w, floor, stable):
    """The sums and entries of functional_reference in the working precision of mpmath: totals and, per entry, the
    sum of the magnitudes of the pieces' contributions."""
    npts = rho.shape[1]
    zero = mp.mpf(0)
    vr, vec = np.full((2, npts), zero, dtype=object), np.full((2, 3, npts), zero, dtype=object)
    mvr, mvec = np.full((2, npts), zero, dtype=object), np.full((2, 3, npts), zero, dtype=object)
    keep = np.zeros(npts, dtype=bool)
    half, tiny, fl = mp.mpf(float(floor)) / 2, mp.mpf(1e-40), mp.mpf(float(floor))
    exc = mexc = nelec = zero
    parts = [(mp.mpf(c.p) / mp.mpf(c.q), label) for c, label in pieces(name)]
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
        for c, label in parts:
            e, va, vb, vaa, vab, vbb = _piece_at(label, stable, args)
            e, va, vb, vaa, vab, vbb = wg * c * e, wg * c * va, wg * c * vb, wg * c * vaa, wg * c * vab, wg * c * vbb
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


def scaled_err(got, want, mag, absolute=1e-150):
    """|got - want| / max(mag, absolute) per entry (float64 array), formed at 50 digits; ``got``: floats or mpf."""
    got, want, mag = np.asarray(got), np.asarray(want), np.asarray(mag)
    out = np.empty(got.shape)
    with mp.workdps(xr.DPS):
        lo = mp.mpf(absolute)
        for idx in np.ndindex(got.shape):
            gv = got[idx]
            if not isinstance(gv, mp.mpf):
                gv = float(gv)
                if not math.isfinite(gv):
                    out[idx] = math.inf
                    continue
            out[idx] = float(abs(mp.mpf(gv) - mp.mpf(want[idx])) / max(mp.mpf(mag[idx]), lo))
    return out


def functional_reference(name: str, rho, grad, w, floor: float, own_error: bool = True):
    """``xr.functional_reference`` for the names of FUNCTIONALS, with its conventions (sigma from the gradients in
    extended precision, +1e-40 on saa and sbb, densities clamped at floor / 2, points with rho_a + rho_b <= floor
    dropped): ``(vr (2, G), vec (2, 3, G), exc, nelec, keep (G,), mag, own)``.

    ``mag = (mag_vr, mag_vec, mag_exc)``: per entry the sum of the magnitudes of the pieces' exact contributions
    (mag_exc = sum_g w |piece|).  ``own = (err_vr, err_vec, err_exc)``: the error, on that scale, of the same
    expressions evaluated with mp.prec = 53 and expm1 / log1p (None when ``own_error`` is False)."""
    rho, grad, w = (np.asarray(x, dtype=np.float64) for x in (rho, grad, w))
    with mp.workdps(xr.DPS):
        vr, vec, exc, nelec, keep, mag = _evaluate(name, rho, grad, w, floor, False)
    own = None
    if own_error:
        with mp.workprec(53):
            vr53, vec53, exc53, _, keep53, _ = _evaluate(name, rho, grad, w, floor, True)
        assert np.array_equal(keep, keep53)
        with mp.workdps(xr.DPS):
            e_exc = float(abs(exc53 - exc) / max(mag[2], mp.mpf(1e-150)))
        own = (scaled_err(vr53, vr, mag[0]), scaled_err(vec53, vec, mag[1]), e_exc)
    return vr, vec, exc, nelec, keep, mag, own


def regime_inputs(regime: str, floor: float):
    return xr.regime_inputs(regime, floor, n=POINTS_PER_REGIME)


@lru_cache(maxsize=None)
def regime_reference(name: str, regime: str, floor: float):
    return functional_reference(name, *regime_inputs(regime, floor), floor)


def own_error(ref) -> float:
    """The worst entry error of the reference's own 53-bit evaluation."""
    return float(max(ref[6][0].max(initial=0.0), ref[6][1].max(initial=0.0)))


def entry_bound(regime: str, ref) -> float:
    """5e-11 -- and, in the two regimes of LOOSE_REGIMES, at least four times the error of the reference's own 53-bit
    evaluation (the 4: a device libm good to 1-2 ulp and another order of operations)."""
    return max(ENTRY_BOUND, 4.0 * own_error(ref)) if regime in LOOSE_REGIMES else ENTRY_BOUND


def check_functional(label: str, got, ref, bound):
    """``got`` = (vr, vec, E_xc, electron count) in float64 against ``ref`` = functional_reference(...): prints the
    worst figure of each output, then asserts ``bound`` (a number, or an array per grid point) per entry on the scale
    of the pieces, 1e-12 on E_xc (relative to sum w |piece|) and the electron count, and exact zeros -- never NaN -- at
    the dropped points."""
    vr, vec, exc, nelec = got
    want_vr, want_vec, want_exc, want_nelec, keep, (mag_vr, mag_vec, mag_exc), _ = ref
    err_r, err_v = scaled_err(vr, want_vr, mag_vr), scaled_err(vec, want_vec, mag_vec)
    with mp.workdps(xr.DPS):
        e_exc = float(abs(mp.mpf(float(exc)) - want_exc) / max(mag_exc, mp.mpf(1e-150))) if math.isfinite(exc) else math.inf
        if mag_exc == 0:
            e_exc = 0.0 if exc == 0.0 else math.inf
    e_n = xr.rel_err_scalar(nelec, want_nelec)
    print(f"XCREF {label} vr_a {err_r[0].max():.2e} vr_b {err_r[1].max():.2e} vec_a {err_v[0].max():.2e} "
          f"vec_b {err_v[1].max():.2e} exc {e_exc:.2e} nelec {e_n:.2e} bound {np.max(bound):.2e}")
    assert np.isfinite(vr).all() and np.isfinite(vec).all()
    dropped = ~keep
    assert np.all(vr[:, dropped] == 0.0) and np.all(vec[:, :, dropped] == 0.0)  # exact zeros, never NaN
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), keep.shape)
    assert np.all(err_r < bound[None, :]) and np.all(err_v < bound[None, None, :]), (
        label, err_r.max(axis=1), err_v.max(axis=(1, 2)))
    assert e_exc < SUM_BOUND and e_n < SUM_BOUND, (label, e_exc, e_n)
    return max(err_r.max(initial=0.0), err_v.max(initial=0.0))
