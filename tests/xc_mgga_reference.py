"""Extended-precision reference for the meta-GGAs ``tpss`` and ``tpssh`` -- the companion of tests/xc_reference.py and
tests/xc_gga_reference.py, whose regimes and conventions are reused.  Written from the published formulas with mpmath at
50 digits; nothing here is imported from ``nbed_amd``.

  TPSS exchange (Tao, Perdew, Staroverov and Scuseria, Phys. Rev. Lett. 91, 146401 (2003), eqs. 5-10), spin-scaled:
    E_x[n_a, n_b] = 1/2 E_x[2 n_a] + 1/2 E_x[2 n_b] (tau doubled too),  E_x[n] = int e_x^unif(n) F_x(p, z),
    p = |grad n|^2 / (4 (3 pi^2)^(2/3) n^(8/3)),  z = tau_W / tau,  tau_W = |grad n|^2 / (8 n),
    alpha = (5p/3)(1/z - 1) = (tau - tau_W) / tau_unif,  tau_unif = (3/10)(3 pi^2)^(2/3) n^(5/3),
    q_b = (9/20)(alpha - 1) / sqrt(1 + b alpha (alpha - 1)) + 2p/3,
    x = {[10/81 + c z^2 / (1 + z^2)^2] p + (146/2025) q_b^2 - (73/405) q_b sqrt((1/2)(3z/5)^2 + p^2/2)
         + (1/kappa)(10/81)^2 p^2 + 2 sqrt(e)(10/81)(3z/5)^2 + e mu p^3} / (1 + sqrt(e) p)^2,
    F_x = 1 + kappa - kappa / (1 + x / kappa);  kappa = 0.804, b = 0.40, c = 1.59096, e = 1.537, mu = 0.21951
  TPSS correlation (eqs. 11-14):  z of the totals,
    eps_revPKZB = eps_PBE(n_a, n_b, grad n_a, grad n_b) [1 + C z^2] - (1 + C) z^2 sum_s (n_s / n) eps~_s,
    eps~_s = the larger of eps_PBE(n_s, 0, grad n_s, 0) and eps_PBE of the full density,
    C = (0.53 + 0.87 zeta^2 + 0.50 zeta^4 + 2.26 zeta^6) / {1 + xi^2 [(1 + zeta)^(-4/3) + (1 - zeta)^(-4/3)] / 2}^4,
    xi = |grad zeta| / (2 (3 pi^2 n)^(1/3)),  |grad zeta|^2 = 4 (n_b^2 s_aa - 2 n_a n_b s_ab + n_a^2 s_bb) / n^4,
    eps_TPSS = eps_revPKZB [1 + d eps_revPKZB z^3],  d = 2.8,  e_c = n eps_TPSS;
    eps_PBE: PBE correlation on PW92 with libxc's LDA_C_PW_MOD constants and beta = 0.06672455060314922
  tpss = exchange + correlation;  tpssh = 0.9 exchange + correlation  (the semi-local parts)

Conventions of the product (copied, not imported): densities clamped at floor / 2, sigma_aa and sigma_bb lifted by 1e-40,
points with rho_a + rho_b <= floor dropped; wherever z is formed tau is clamped from below at the tau_W of the same
clamped quantities -- each channel's own in the exchange, the totals in the correlation -- by the test
``tau >= sigma / (8 n) * (1 - 1e-10)`` CARRIED OUT IN FLOAT64 (so that the branch of the reference is the branch of the
code under test), and where it fails z = 1 and alpha = 0 are constants (the margin keeps a one-orbital density, which has
tau = tau_W at every point, on one side of the kink that the potential has at the clamp: z <= 1 + 1e-10); "the larger of" a and b is a where
a >= b.

First derivatives are central differences of the 50-digit energy (relative step 1e-20, carried at 90 digits), with the branches -- the three clamps and the two "larger of" -- frozen at their values at the point.

The energy density is split into seven pieces that add up to it exactly: the two exchange channels, n eps_PW (1 + C z^2),
n H (1 + C z^2), the eps_PW part and the H part of -(1 + C) z^2 sum_s n_s eps~_s, and the remainder
d n z^3 eps_revPKZB^2.  eps_PW and H cancel at a large reduced gradient (in eps~_s as well) and the third and fourth
cancel the fifth and sixth for a one-electron density, so errors are measured against the
sum of the MAGNITUDES of the pieces' contributions to an entry, as tests/xc_gga_reference.py does.
"""

from __future__ import annotations

import math
from functools import lru_cache

import mpmath as mp
import numpy as np

import xc_gga_reference as gr
import xc_reference as xr

NAMES = ("tpss", "tpssh")
EXCHANGE_SCALE = {"tpss": "1", "tpssh": "0.9"}
POINTS_PER_REGIME = 64
NEW_REGIMES = ("z_one", "z_one_plus_1e-12", "tau_below_tau_w", "z_1e-6", "zero_gradient_tau_unif", "polarised_tau_empty")
REGIMES = xr.REGIMES + NEW_REGIMES
ENTRY_BOUND, SUM_BOUND = xr.ENTRY_BOUND, xr.SUM_BOUND
WORK_DPS = 90
STEP = "1e-20"
NPIECE = 7
CLAMP = np.float64(1.0) - np.float64(1e-10)


def _c(s):
    return mp.mpf(s)


class Dual:
    """A value with its seven first derivatives, in the working precision of mpmath (forward mode): what lets the same
    expressions be evaluated with their derivatives in 53-bit arithmetic, where differences are of no use."""

    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def lift(x):
        return x if isinstance(x, Dual) else Dual(mp.mpf(x), [mp.mpf(0)] * 7)

    def _chain(self, v, dv):  # f(self) with f' = dv
        return Dual(v, [dv * x for x in self.d])

    def __add__(self, o):
        o = Dual.lift(o)
        return Dual(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])

    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, [-a for a in self.d])

    def __sub__(self, o):
        return self + (-Dual.lift(o))

    def __rsub__(self, o):
        return Dual.lift(o) + (-self)

    def __mul__(self, o):
        o = Dual.lift(o)
        return Dual(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o)
        q = self.v / o.v
        return Dual(q, [(a - q * b) / o.v for a, b in zip(self.d, o.d)])

    def __rtruediv__(self, o):
        return Dual.lift(o) / self

    def __pow__(self, e):
        if self.v == 0:  # (an empty channel's 1 - zeta: every power taken of it is positive and it is a constant)
            return Dual(mp.mpf(0), [mp.mpf(0)] * 7)
        return self._chain(self.v ** e, e * self.v ** (e - 1))

    def __ge__(self, o):
        return self.v >= Dual.lift(o).v


def _sqrt(x):
    return x._chain(mp.sqrt(x.v), 1 / (2 * mp.sqrt(x.v))) if isinstance(x, Dual) else mp.sqrt(x)


def _log1p(x):
    return x._chain(mp.log1p(x.v), 1 / (1 + x.v)) if isinstance(x, Dual) else mp.log1p(x)


def _expm1(x):
    return x._chain(mp.expm1(x.v), mp.exp(x.v)) if isinstance(x, Dual) else mp.expm1(x)


# ------------------------------------------------------------------------------------------ the pieces at one point
def _pw_g(rs, a, a1, b1, b2, b3, b4):
    a, a1, b1, b2, b3, b4 = (_c(v) for v in (a, a1, b1, b2, b3, b4))
    q1 = 2 * a * (b1 * _sqrt(rs) + b2 * rs + b3 * rs ** _c("1.5") + b4 * rs ** 2)
    return -2 * a * (1 + a1 * rs) * _log1p(1 / q1)


def _pbe_parts(ra, rb, st):
    """(eps_PW, H) per electron of PBE correlation for the spin densities (ra, rb) and the total sigma."""
    third = mp.mpf(1) / 3
    n = ra + rb
    rs = (3 / (4 * mp.pi * n)) ** third
    up, dn = 2 * ra / n, 2 * rb / n
    zeta = (ra - rb) / n
    fz = (up ** (4 * third) + dn ** (4 * third) - 2) / (2 ** (4 * third) - 2)
    fpp0 = (mp.mpf(4) / 9) / (2 ** third - 1)
    e0 = _pw_g(rs, "0.0310907", "0.21370", "7.5957", "3.5876", "1.6382", "0.49294")
    e1 = _pw_g(rs, "0.01554535", "0.20548", "14.1189", "6.1977", "3.3662", "0.62517")
    ac = -_pw_g(rs, "0.0168869", "0.11125", "10.357", "3.6231", "0.88026", "0.49671")
    eps = e0 + ac * fz / fpp0 * (1 - zeta ** 4) + (e1 - e0) * fz * zeta ** 4
    beta, gamma = _c("0.06672455060314922"), (1 - mp.log(2)) / mp.pi ** 2
    phi = (up ** (2 * third) + dn ** (2 * third)) / 2
    kf = (3 * mp.pi ** 2 * n) ** third
    t2 = st / (4 * phi ** 2 * (4 * kf / mp.pi) * n ** 2)
    a = (beta / gamma) / _expm1(-eps / (gamma * phi ** 3))
    y = a * t2
    h = gamma * phi ** 3 * _log1p(beta / gamma * t2 * (1 + y) / (1 + y + y * y))
    return eps, h


def _exchange_channel(r, s, tau, ok):
    third = mp.mpf(1) / 3
    kappa, b, c, e, mu = _c("0.804"), _c("0.40"), _c("1.59096"), _c("1.537"), _c("0.21951")
    n, sig, t = 2 * r, 4 * s, 2 * tau  # the spin-scaling relation
    p = sig / (4 * (3 * mp.pi ** 2) ** (2 * third) * n ** (8 * third))
    tw = sig / (8 * n)
    if ok:
        z = tw / t
        alpha = (t - tw) / (mp.mpf(3) / 10 * (3 * mp.pi ** 2) ** (2 * third) * n ** (5 * third))
    else:
        z, alpha = (Dual.lift(1), Dual.lift(0)) if isinstance(r, Dual) else (mp.mpf(1), mp.mpf(0))
    qb = mp.mpf(9) / 20 * (alpha - 1) / _sqrt(1 + b * alpha * (alpha - 1)) + 2 * p / 3
    c1081 = mp.mpf(10) / 81
    x = ((c1081 + c * z ** 2 / (1 + z ** 2) ** 2) * p + mp.mpf(146) / 2025 * qb ** 2
         - mp.mpf(73) / 405 * qb * _sqrt((3 * z / 5) ** 2 / 2 + p ** 2 / 2) + c1081 ** 2 / kappa * p ** 2
         + 2 * mp.sqrt(e) * c1081 * (3 * z / 5) ** 2 + e * mu * p ** 3) / (1 + mp.sqrt(e) * p) ** 2
    fx = 1 + kappa - kappa / (1 + x / kappa)
    ex_unif = -mp.mpf(3) / 4 * (3 / mp.pi) ** third * n ** (4 * third)
    return ex_unif * fx / 2


def pieces_at(args, flags):
    """The seven pieces of e_xc (exchange unscaled) at (ra, rb, saa, sab, sbb, ta, tb), all mpf, with the branches
    ``flags = (ok_a, ok_b, ok_c, sel_a, sel_b)``: the clamps pass, eps~_s is the one-spin value; sel None: decided
    here.  Returns (pieces, flags)."""
    ra, rb, saa, sab, sbb, ta, tb = args
    ok_a, ok_b, ok_c, sel_a, sel_b = flags
    third = mp.mpf(1) / 3
    xa, xb = _exchange_channel(ra, saa, ta, ok_a), _exchange_channel(rb, sbb, tb, ok_b)
    n = ra + rb
    st = saa + 2 * sab + sbb
    z = st / (8 * n) / (ta + tb) if ok_c else Dual.lift(1) if isinstance(n, Dual) else mp.mpf(1)
    eps_pw, h = _pbe_parts(ra, rb, st)
    eps = eps_pw + h
    pa, pb = _pbe_parts(ra, mp.mpf(0), saa), _pbe_parts(rb, mp.mpf(0), sbb)
    if sel_a is None:
        sel_a, sel_b = bool(pa[0] + pa[1] >= eps), bool(pb[0] + pb[1] >= eps)
    (ea_pw, ea_h), (eb_pw, eb_h) = (pa if sel_a else (eps_pw, h)), (pb if sel_b else (eps_pw, h))
    zeta = (ra - rb) / n
    gz2 = 4 * (rb ** 2 * saa - 2 * ra * rb * sab + ra ** 2 * sbb) / n ** 4
    xi2 = gz2 / (4 * (3 * mp.pi ** 2 * n) ** (2 * third))
    big_c = ((_c("0.53") + _c("0.87") * zeta ** 2 + _c("0.50") * zeta ** 4 + _c("2.26") * zeta ** 6)
             / (1 + xi2 * ((2 * ra / n) ** (-4 * third) + (2 * rb / n) ** (-4 * third)) / 2) ** 4)
    p1e = n * eps_pw * (1 + big_c * z ** 2)
    p1h = n * h * (1 + big_c * z ** 2)
    p2e = -(1 + big_c) * z ** 2 * (ra * ea_pw + rb * eb_pw)
    p2h = -(1 + big_c) * z ** 2 * (ra * ea_h + rb * eb_h)
    rev = (p1e + p1h + p2e + p2h) / n
    rest = _c("2.8") * n * z ** 3 * rev ** 2
    return (xa, xb, p1e, p1h, p2e, p2h, rest), (ok_a, ok_b, ok_c, sel_a, sel_b)


@lru_cache(maxsize=None)
def _point(args64: tuple, clamps: tuple):
    """(pieces (7,), d pieces / d variable (7, 7), flags) at one point of float64 inputs (already clamped and lifted
    sigmas given as mpf strings are avoided: ``args64`` holds the seven values as exact mpf)."""
    with mp.workdps(WORK_DPS):
        args = list(args64)
        base, flags = pieces_at(args, clamps + (None, None))
        ra, rb, saa, sab, sbb, ta, tb = args
        # the step is relative to the variable itself (an empty channel's tau is 1e-27 beside the other's); a variable
        # that is zero gets the scale of what it is added to
        scale = (ra, rb, saa, abs(sab) if sab != 0 else mp.sqrt(saa * sbb), sbb,
                 ta if ta != 0 else max(tb, mp.mpf("1e-300")), tb if tb != 0 else max(ta, mp.mpf("1e-300")))
        rel = mp.mpf(STEP)
        der = []
        for i in range(7):
            h = rel * scale[i]
            hi, lo = list(args), list(args)
            hi[i], lo[i] = args[i] + h, args[i] - h
            fp, _ = pieces_at(hi, flags)
            fm, _ = pieces_at(lo, flags)
            der.append([(a - b) / (2 * h) for a, b in zip(fp, fm)])
        return base, [[der[i][k] for i in range(7)] for k in range(NPIECE)], flags


@lru_cache(maxsize=None)
def _point_53(args64: tuple, flags: tuple):
    """d pieces / d variable (7, 7) of the same expressions evaluated in 53-bit arithmetic (forward mode, log1p and
    expm1 where the formulas have ln(1 + .) and exp(.) - 1), the branches given: the reference's own float64 error."""
    with mp.workprec(53):
        args = [Dual(+a, [mp.mpf(int(i == j)) for j in range(7)]) for i, a in enumerate(args64)]
        out, _ = pieces_at(args, flags)
        return [Dual.lift(o).d for o in out]


def clamp_flags(ra, rb, saa, sab, sbb, ta, tb):
    """The three tests ``tau >= sigma / (8 n) * CLAMP`` in float64, as the convention prescribes (float inputs)."""
    ra, rb, saa, sab, sbb, ta, tb = (np.float64(v) for v in (ra, rb, saa, sab, sbb, ta, tb))
    return (bool(ta >= saa / (8.0 * ra) * CLAMP), bool(tb >= sbb / (8.0 * rb) * CLAMP),
            bool(ta + tb >= (saa + 2.0 * sab + sbb) / (8.0 * (ra + rb)) * CLAMP))


# ------------------------------------------------------------------------------------------ the product's conventions
def functional_reference(name: str, rho, grad, tau, w, floor: float, own_error: bool = False):
    """``(vr (2, G), vec (2, 3, G), vt (2, G), exc, nelec, keep (G,), mag)`` of nbx_xc_functional_mgga's outputs at 50
    digits (weights folded in), ``mag = (mag_vr, mag_vec, mag_vt, mag_exc)`` the sums of the magnitudes of the seven
    pieces' contributions.  The float64 sigmas that decide the clamps are sum g^2 (+ 1e-40) in float64."""
    rho, grad, tau, w = (np.asarray(x, dtype=np.float64) for x in (rho, grad, tau, w))
    npts = rho.shape[1]
    with mp.workdps(WORK_DPS):
        zero = mp.mpf(0)
        ax = mp.mpf(EXCHANGE_SCALE[name])
        coef = (ax, ax) + (mp.mpf(1),) * 5
        vr, vec, vt = (np.full(s, zero, dtype=object) for s in ((2, npts), (2, 3, npts), (2, npts)))
        mvr, mvec, mvt = (np.full(s, zero, dtype=object) for s in ((2, npts), (2, 3, npts), (2, npts)))
        keep = np.zeros(npts, dtype=bool)
        half, tiny, fl = mp.mpf(float(floor)) / 2, mp.mpf(1e-40), mp.mpf(float(floor))
        exc = mexc = nelec = zero
        own = np.zeros((3, npts))  # worst error of the rho, sigma and tau derivatives at the point
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
            ra, rb = max(r0, half), max(r1, half)
            ta, tb = mp.mpf(float(tau[0, g])), mp.mpf(float(tau[1, g]))
            fa, fb = grad[0, :, g], grad[1, :, g]
            s64 = (float(fa[0] * fa[0] + fa[1] * fa[1] + fa[2] * fa[2]) + 1e-40, float(fa[0] * fb[0] + fa[1] * fb[1] + fa[2] * fb[2]),
                   float(fb[0] * fb[0] + fb[1] * fb[1] + fb[2] * fb[2]) + 1e-40)
            clamps = clamp_flags(max(float(rho[0, g]), floor / 2), max(float(rho[1, g]), floor / 2), s64[0], s64[1], s64[2],
                                 float(tau[0, g]), float(tau[1, g]))
            base, der, flags = _point((ra, rb, saa, sab, sbb, ta, tb), clamps)
            if own_error:
                # the derivatives' errors on the scale of the pieces (the entries of vr, vec and vt are these times the
                # weight and, for vec, combined with the gradient's components)
                d53 = _point_53((ra, rb, saa, sab, sbb, ta, tb), flags)
                for i in range(7):
                    got = sum(coef[k] * d53[k][i] for k in range(NPIECE))
                    want = sum(coef[k] * der[k][i] for k in range(NPIECE))
                    mag = sum(abs(coef[k] * der[k][i]) for k in range(NPIECE))
                    if mag > 0:
                        kind = (0, 0, 1, 1, 1, 2, 2)[i]
                        own[kind, g] = max(own[kind, g], float(abs(got - want) / mag))
            for k in range(NPIECE):
                c = wg * coef[k]
                e = c * base[k]
                va, vb, vaa, vab, vbb, vta, vtb = (c * d for d in der[k])
                exc += e
                mexc += abs(e)
                vr[0, g] += va
                vr[1, g] += vb
                mvr[0, g] += abs(va)
                mvr[1, g] += abs(vb)
                vt[0, g] += vta
                vt[1, g] += vtb
                mvt[0, g] += abs(vta)
                mvt[1, g] += abs(vtb)
                for a in range(3):
                    ea, eb = 2 * vaa * ga[a] + vab * gb[a], 2 * vbb * gb[a] + vab * ga[a]
                    vec[0, a, g] += ea
                    vec[1, a, g] += eb
                    mvec[0, a, g] += abs(ea)
                    mvec[1, a, g] += abs(eb)
    return vr, vec, vt, exc, nelec, keep, (mvr, mvec, mvt, mexc), (own if own_error else None)


# ------------------------------------------------------------------------------------------ input regimes
_CF = 0.3 * (6.0 * math.pi ** 2) ** (2.0 / 3.0)  # tau_unif of a spin channel = _CF rho_s^(5/3)


def _tau_w(rho, grad, floor):
    """tau_W (2, n) of each channel from the clamped densities and the lifted sigmas, float64."""
    r = np.maximum(rho, floor / 2)
    return ((grad * grad).sum(axis=1) + 1e-40) / (8.0 * r)


def regime_inputs(regime: str, floor: float, n: int = POINTS_PER_REGIME):
    """``(rho (2, n), grad (2, 3, n), tau (2, n), w (n))`` of one regime -- float64, fixed seed.  The ten regimes of
    tests/xc_reference.py get tau_s = tau_W,s (1 + 10^u), u uniform in (-2, 2): z from 0.01 to 0.99."""
    rng = np.random.default_rng(5000 + REGIMES.index(regime))
    if regime in xr.REGIMES:
        rho, grad, w = xr.regime_inputs(regime, floor, n=n)
        tau = _tau_w(rho, grad, floor) * (1.0 + 10 ** rng.uniform(-2, 2, (2, n)))
        return rho, grad, tau, w
    if regime == "z_one":
        # tau = tau_W to the bit: gradients of small integers times a power of two and densities that are powers of two,
        # so that sigma (the 1e-40 is absorbed) and sigma / (8 rho) are exact in float64 in any order of operations.
        # First half: one electron (beta empty, tau_b = 0); second half: closed shell (the total z is 1 too).
        ra = 2.0 ** rng.integers(-20, 7, n)
        ga = rng.integers(-31, 32, (3, n)) * 2.0 ** rng.integers(-12, 3, n)[None, :]
        ga[0, ga[0] == 0] = 1.0
        ta = (ga * ga).sum(axis=0) / (8.0 * ra)
        closed = np.arange(n) >= n // 2
        rho = np.stack([ra, np.where(closed, ra, 0.0)])
        grad = np.stack([ga, np.where(closed[None, :], ga, 0.0)])
        tau = np.stack([ta, np.where(closed, ta, 0.0)])
        assert np.all((grad[0] ** 2).sum(axis=0) + 1e-40 == (grad[0] ** 2).sum(axis=0))
        return rho, grad, tau, rng.uniform(0.1, 2.0, n)
    if regime == "polarised_tau_empty":
        rho, grad, w = xr.regime_inputs("polarised_beta_empty", floor, n=n)
        tau = _tau_w(rho, grad, floor) * (1.0 + 10 ** rng.uniform(-2, 2, (2, n)))
        tau[1] = 0.0
        return rho, grad, tau, w
    rho, grad, w = xr.regime_inputs("existing", floor, n=n)
    if regime == "zero_gradient_tau_unif":
        grad = np.zeros_like(grad)
        tau = _CF * rho ** (5.0 / 3.0)
    elif regime == "z_one_plus_1e-12":
        tau = _tau_w(rho, grad, floor) * (1.0 + 1e-12)
    elif regime == "tau_below_tau_w":
        tw = _tau_w(rho, grad, floor)
        tau = tw * rng.uniform(0.0, 0.9, (2, n))
        tau[:, ::8] = 0.0
        tau[:, 1::8] = tw[:, 1::8] * (1.0 - 2e-10)   # just below the margin: clamped
        tau[:, 2::8] = tw[:, 2::8] * (1.0 - 5e-11)   # inside it: not clamped, z = 1 + 5e-11
    elif regime == "z_1e-6":
        tau = _tau_w(rho, grad, floor) * 1e6
    else:
        raise ValueError(regime)
    return rho, grad, tau, w


#: regimes whose bound follows the reference's own 53-bit evaluation: the two of tests/xc_gga_reference.py, and the
#: uniform gas, where alpha - 1 = (tau - tau_W - tau_unif) / tau_unif is a rounding residue of its three terms and
#: dE/dtau, proportional to it, has no correct digit in any float64 evaluation (it is 1e-16 of dE/dtau elsewhere)
LOOSE_REGIMES = gr.LOOSE_REGIMES + ("zero_gradient_tau_unif",)


@lru_cache(maxsize=None)
def regime_reference(name: str, regime: str, floor: float):
    return functional_reference(name, *regime_inputs(regime, floor), floor, own_error=regime in LOOSE_REGIMES)


def entry_bound(regime: str, ref):
    """(bound of vr, of vec, of vt): 5e-11 -- and, in the regimes of LOOSE_REGIMES, at least four times the worst error
    of the reference's own 53-bit evaluation of the derivatives of that kind in the regime (the rule of
    tests/xc_gga_reference.py; a rounding residue has no pointwise bound)."""
    if regime not in LOOSE_REGIMES:
        return (ENTRY_BOUND,) * 3
    return tuple(max(ENTRY_BOUND, 4.0 * float(ref[7][k].max(initial=0.0))) for k in range(3))


def check_functional(label: str, got, ref, bound=(ENTRY_BOUND,) * 3):
    """``got`` = (vr, vec, vt, E_xc, electron count) in float64 against ``ref`` = functional_reference(...): prints the
    worst figure of each output, then asserts ``bound`` = (of vr, of vec, of vt; numbers or arrays per grid point) per entry on the scale of the pieces, 1e-12 on E_xc (relative to
    sum w |piece|) and the electron count, and exact zeros -- never NaN -- at the dropped points.  Returns the worst
    entry."""
    vr, vec, vt, exc, nelec = got
    want_vr, want_vec, want_vt, want_exc, want_nelec, keep, (mag_vr, mag_vec, mag_vt, mag_exc), _ = ref
    err_r, err_v, err_t = (gr.scaled_err(a, b, c) for a, b, c in ((vr, want_vr, mag_vr), (vec, want_vec, mag_vec),
                                                                   (vt, want_vt, mag_vt)))
    with mp.workdps(xr.DPS):
        e_exc = float(abs(mp.mpf(float(exc)) - want_exc) / max(mag_exc, mp.mpf(1e-150))) if math.isfinite(exc) else math.inf
        if mag_exc == 0:
            e_exc = 0.0 if exc == 0.0 else math.inf
    e_n = xr.rel_err_scalar(nelec, want_nelec)
    worst = max(err_r.max(initial=0.0), err_v.max(initial=0.0), err_t.max(initial=0.0))
    print(f"XCMGGA {label} vr_a {err_r[0].max(initial=0.0):.2e} vr_b {err_r[1].max(initial=0.0):.2e} "
          f"vec_a {err_v[0].max(initial=0.0):.2e} vec_b {err_v[1].max(initial=0.0):.2e} vt_a {err_t[0].max(initial=0.0):.2e} "
          f"vt_b {err_t[1].max(initial=0.0):.2e} exc {e_exc:.2e} nelec {e_n:.2e} bound {' '.join(f'{np.max(b):.2e}' for b in bound)}")
    assert np.isfinite(vr).all() and np.isfinite(vec).all() and np.isfinite(vt).all()
    dropped = ~keep
    assert np.all(vr[:, dropped] == 0.0) and np.all(vec[:, :, dropped] == 0.0) and np.all(vt[:, dropped] == 0.0)
    b_r, b_v, b_t = (np.broadcast_to(np.asarray(b, dtype=np.float64), keep.shape) for b in bound)
    assert np.all(err_r < b_r[None, :]) and np.all(err_v < b_v[None, None, :]) and np.all(err_t < b_t[None, :]), (
        label, err_r.max(axis=1), err_v.max(axis=(1, 2)), err_t.max(axis=1))
    assert e_exc < SUM_BOUND and e_n < SUM_BOUND, (label, e_exc, e_n)
    return worst
