"""Extended-precision references for the exchange-correlation chain (csrc/grid.hip, csrc/xc.hip).

Nothing here is imported from ``nbed_amd.xc``: the energy densities are transcribed from the papers as sympy
expressions with exact rational constants, differentiated symbolically and evaluated by mpmath at 50 digits; the
contractions and the point-wise producers are restated in ``numpy.longdouble`` (64-bit mantissa, or compensated
float64 sums where the host has no 80-bit type).  tests/test_host_xc_reference.py holds the host expression to
these references, tests/test_gpu_xc.py the five kernels.

  Slater      e = -(3/2) (3 / (4 pi))^(1/3) (ra^(4/3) + rb^(4/3))
  B88         e = -beta sum_s rs^(4/3) x^2 / (1 + 6 beta x asinh x),  x = sqrt(sigma_ss) / rs^(4/3),  beta = 0.0042
              (A. D. Becke, Phys. Rev. A 38, 3098 (1988): the gradient correction alone)
  VWN         e = rho eps(x, zeta),  x = sqrt(r_s),  Vosko, Wilk and Nusair, Can. J. Phys. 58, 1200 (1980), eq. 4.4 with
              the parameters of their fits to the RPA ("VWN-RPA", interpolated with f(zeta) alone) and to the
              Ceperley-Alder data ("VWN5", interpolated through the spin stiffness)
  LYP         Lee, Yang and Parr in the gradient-only form of Miehlich, Savin, Stoll and Preuss, Chem. Phys. Lett. 157,
              200 (1989), eq. 2
  b3lyp       0.8 Slater + 0.72 B88 + 0.19 VWN-RPA + 0.81 LYP (the semi-local part)
"""

from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import mpmath as mp
import numpy as np
import sympy as sp

DPS = 50
U = 2.0 ** -53  # unit roundoff of float64
LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 2e-19)

RA, RB, SAA, SAB, SBB = VARS = (sp.Symbol("ra", positive=True), sp.Symbol("rb", positive=True),
                                sp.Symbol("saa", positive=True), sp.Symbol("sab", real=True),
                                sp.Symbol("sbb", positive=True))
FUNCTIONALS = ("b3lyp", "lda", "lda,vwn", "slater")


def _q(literal: str):
    """The exact rational a decimal literal denotes."""
    return sp.Rational(literal)


_THIRD = sp.Rational(1, 3)


# ------------------------------------------------------------------------------------------ energy densities
def slater_expr(ra=RA, rb=RB):
    cx = sp.Rational(3, 2) * (3 / (4 * sp.pi)) ** _THIRD
    return -cx * (ra ** (4 * _THIRD) + rb ** (4 * _THIRD))


def b88_enhancement(x):
    """g(x) of e = -beta rho^(4/3) g(x)."""
    beta = _q("0.0042")
    return x * x / (1 + 6 * beta * x * sp.asinh(x))


def b88_expr(ra=RA, rb=RB, saa=SAA, sbb=SBB):
    beta = _q("0.0042")
    out = 0
    for r, s in ((ra, saa), (rb, sbb)):
        r43 = r ** (4 * _THIRD)
        out = out - beta * r43 * b88_enhancement(sp.sqrt(s) / r43)
    return out


def _vwn_fit(x, a, x0, b, c):
    q = sp.sqrt(4 * c - b * b)
    big = x * x + b * x + c
    big0 = x0 * x0 + b * x0 + c
    at = sp.atan(q / (2 * x + b))
    return a * (sp.log(x * x / big) + 2 * b / q * at
                - b * x0 / big0 * (sp.log((x - x0) ** 2 / big) + 2 * (b + 2 * x0) / q * at))


def _vwn_common(ra, rb):
    rho = ra + rb
    x = (3 / (4 * sp.pi * rho)) ** sp.Rational(1, 6)
    up, dn = 2 * ra / rho, 2 * rb / rho  # 1 + zeta, 1 - zeta
    fz = (up ** (4 * _THIRD) + dn ** (4 * _THIRD) - 2) / (2 ** (4 * _THIRD) - 2)
    return rho, x, up, dn, fz


def vwn_rpa_expr(ra=RA, rb=RB):
    rho, x, _, _, fz = _vwn_common(ra, rb)
    ep = _vwn_fit(x, _q("0.0310907"), _q("-0.409286"), _q("13.0720"), _q("42.7198"))
    ef = _vwn_fit(x, _q("0.01554535"), _q("-0.743294"), _q("20.1231"), _q("101.578"))
    return rho * (ep + fz * (ef - ep))


def vwn5_expr(ra=RA, rb=RB):
    rho, x, up, dn, fz = _vwn_common(ra, rb)
    ep = _vwn_fit(x, _q("0.0310907"), _q("-0.10498"), _q("3.72744"), _q("12.9352"))
    ef = _vwn_fit(x, _q("0.01554535"), _q("-0.32500"), _q("7.06042"), _q("18.0578"))
    al = _vwn_fit(x, -1 / (6 * sp.pi ** 2), _q("-0.0047584"), _q("1.13107"), _q("13.0045"))
    fpp0 = sp.Rational(4, 9) / (2 ** _THIRD - 1)
    zeta = (ra - rb) / rho
    z4 = zeta ** 4
    one_minus_z4 = up * dn * (1 + zeta * zeta)
    return rho * (ep + al * fz / fpp0 * one_minus_z4 + (ef - ep) * fz * z4)


def lyp_expr(ra=RA, rb=RB, saa=SAA, sab=SAB, sbb=SBB):
    a, b, c, d = _q("0.04918"), _q("0.132"), _q("0.2533"), _q("0.349")
    rho = ra + rb
    r13 = rho ** (-_THIRD)
    den = 1 + d * r13
    omega = sp.exp(-c * r13) / den * rho ** sp.Rational(-11, 3)
    delta = c * r13 + d * r13 / den
    cf = sp.Rational(3, 10) * (3 * sp.pi ** 2) ** (2 * _THIRD)
    stot = saa + 2 * sab + sbb
    brace = (ra * rb * (2 ** sp.Rational(11, 3) * cf * (ra ** sp.Rational(8, 3) + rb ** sp.Rational(8, 3))
                        + (sp.Rational(47, 18) - 7 * delta / 18) * stot
                        - (sp.Rational(5, 2) - delta / 18) * (saa + sbb)
                        - (delta - 11) / 9 * (ra / rho * saa + rb / rho * sbb))
             - sp.Rational(2, 3) * rho ** 2 * stot
             + (sp.Rational(2, 3) * rho ** 2 - ra ** 2) * sbb
             + (sp.Rational(2, 3) * rho ** 2 - rb ** 2) * saa)
    return -a * 4 / den * ra * rb / rho - a * b * omega * brace


def energy_density_expr(name: str):
    if name == "slater":
        return slater_expr()
    if name == "lda":
        return slater_expr() + vwn_rpa_expr()
    if name == "lda,vwn":
        return slater_expr() + vwn5_expr()
    if name == "b3lyp":
        return (sp.Rational(8, 10) * slater_expr() + sp.Rational(72, 100) * b88_expr()
                + sp.Rational(19, 100) * vwn_rpa_expr() + sp.Rational(81, 100) * lyp_expr())
    raise ValueError(name)


def evaluate_expr(expr, ra, rb, saa=1, sab=0, sbb=1):
    """One expression at one point, 50 digits (arguments: anything sympy takes exactly -- ints, Rationals, mpf)."""
    vals = [sp.Float(str(v), DPS + 10) if isinstance(v, mp.mpf) else sp.sympify(v) for v in (ra, rb, saa, sab, sbb)]
    return mp.mpf(str(sp.N(expr.subs(dict(zip(VARS, vals))), DPS)))


@lru_cache(maxsize=None)
def _compiled(name: str):
    e = energy_density_expr(name)
    outs = [e] + [sp.diff(e, v) for v in VARS]
    return sp.lambdify(VARS, outs, modules="mpmath", cse=True)


def point(name: str, ra, rb, saa, sab, sbb):
    """(e, de/dra, de/drb, de/dsaa, de/dsab, de/dsbb) at one point, mpf at 50 digits."""
    with mp.workdps(DPS):
        return tuple(mp.mpf(v) for v in _compiled(name)(mp.mpf(ra), mp.mpf(rb), mp.mpf(saa), mp.mpf(sab), mp.mpf(sbb)))


# ------------------------------------------------------------------------------------------ the product's conventions
def functional_reference(name: str, rho, grad, w, floor: float):
    """What nbx_xc_functional / XCProvider's host expression are to return for the float64 inputs ``rho`` (2, G),
    ``grad`` (2, 3, G), ``w`` (G): sigma from the gradients in extended precision (+1e-40 on saa and sbb), densities
    clamped at floor / 2, points with rho_a + rho_b <= floor dropped.  Returns ``(vr (2, G), vec (2, 3, G), exc,
    nelec, keep (G,))`` -- object arrays of mpf, sums in extended precision."""
    rho, grad, w = (np.asarray(x, dtype=np.float64) for x in (rho, grad, w))
    npts = rho.shape[1]
    vr = np.empty((2, npts), dtype=object)
    vec = np.empty((2, 3, npts), dtype=object)
    keep = np.zeros(npts, dtype=bool)
    with mp.workdps(DPS):
        f = _compiled(name)
        zero, half, tiny, fl = mp.mpf(0), mp.mpf(float(floor)) / 2, mp.mpf(1e-40), mp.mpf(float(floor))
        exc = nelec = zero
        for g in range(npts):
            r0, r1, wg = mp.mpf(float(rho[0, g])), mp.mpf(float(rho[1, g])), mp.mpf(float(w[g]))
            ga = [mp.mpf(float(grad[0, a, g])) for a in range(3)]
            gb = [mp.mpf(float(grad[1, a, g])) for a in range(3)]
            nelec += wg * (r0 + r1)
            if not r0 + r1 > fl:
                vr[:, g] = zero
                vec[:, :, g] = zero
                continue
            keep[g] = True
            saa = sum(x * x for x in ga) + tiny
            sbb = sum(x * x for x in gb) + tiny
            sab = sum(x * y for x, y in zip(ga, gb))
            e, va, vb, vaa, vab, vbb = f(max(r0, half), max(r1, half), saa, sab, sbb)
            exc += wg * e
            vr[0, g], vr[1, g] = wg * va, wg * vb
            for a in range(3):
                vec[0, a, g] = wg * (2 * vaa * ga[a] + vab * gb[a])
                vec[1, a, g] = wg * (2 * vbb * gb[a] + vab * ga[a])
    return vr, vec, exc, nelec, keep


def rel_err(got, want, absolute=1e-150):
    """|got - want| / max(|want|, absolute) per entry (float64 array), formed at 50 digits.  ``want``: mpf entries."""
    got = np.asarray(got, dtype=np.float64)
    out = np.empty(got.shape)
    with mp.workdps(DPS):
        lo = mp.mpf(absolute)
        for idx in np.ndindex(got.shape):
            gv = float(got[idx])
            if not math.isfinite(gv):
                out[idx] = math.inf
                continue
            wv = mp.mpf(want[idx])
            out[idx] = float(abs(mp.mpf(gv) - wv) / max(abs(wv), lo))
    return out


def rel_err_scalar(got: float, want) -> float:
    """|got - want| / |want| at 50 digits (0 / 0 counts as 0: both sums are empty)."""
    with mp.workdps(DPS):
        want = mp.mpf(want)
        if want == 0:
            return 0.0 if got == 0.0 else math.inf
        return float(abs(mp.mpf(float(got)) - want) / abs(want))


ENTRY_BOUND, SUM_BOUND = 5e-11, 1e-12


def check_functional(label: str, got, ref):
    """``got`` = (vr, vec, E_xc, electron count) in float64 against ``ref`` = functional_reference(...): prints the
    worst figure of each output, then asserts 5e-11 relative per entry (entries below 1e-150 measured against
    1e-150), 1e-12 relative on the two sums, and exact zeros -- never NaN -- at the dropped points."""
    vr, vec, exc, nelec = got
    want_vr, want_vec, want_exc, want_nelec, keep = ref
    err_r, err_v = rel_err(vr, want_vr), rel_err(vec, want_vec)
    e_exc, e_n = rel_err_scalar(exc, want_exc), rel_err_scalar(nelec, want_nelec)
    print(f"XCREF {label} vr_a {err_r[0].max():.2e} vr_b {err_r[1].max():.2e} vec_a {err_v[0].max():.2e} "
          f"vec_b {err_v[1].max():.2e} exc {e_exc:.2e} nelec {e_n:.2e}")
    dropped = ~keep
    assert np.all(vr[:, dropped] == 0.0) and np.all(vec[:, :, dropped] == 0.0)  # exact zeros, never NaN
    assert err_r.max() < ENTRY_BOUND and err_v.max() < ENTRY_BOUND, (label, err_r.max(axis=1), err_v.max(axis=(1, 2)))
    assert e_exc < SUM_BOUND and e_n < SUM_BOUND, (label, e_exc, e_n)


# ------------------------------------------------------------------------------------------ input regimes
REGIMES = ("existing", "closed_shell", "polarised_beta_empty", "polarised_alpha_empty", "polarisation_1e4_1e12",
           "core", "tails", "zero_gradient", "antiparallel", "at_floor")
POINTS_PER_REGIME = 150


def _gradients(rng, r):
    """Gradients with reduced gradients x = |grad rho| / rho^(4/3) over 1e-2 .. 1e2."""
    n = r.shape[0]
    return rng.normal(size=(3, n)) * np.maximum(r, 5e-15) ** (4 / 3) * 10 ** rng.uniform(-2, 2, n)


def regime_inputs(regime: str, floor: float, n: int = POINTS_PER_REGIME):
    """``(rho (2, n), grad (2, 3, n), w (n))`` of one regime -- float64, fixed seed."""
    rng = np.random.default_rng(1000 + REGIMES.index(regime))
    ra = 10 ** rng.uniform(-9, 2, n)
    rb = ra * 10 ** rng.uniform(-3, 3, n)
    ga = gb = None
    if regime == "closed_shell":
        rb = ra.copy()
        ga = _gradients(rng, ra)
        gb = ga.copy()
    elif regime in ("polarised_beta_empty", "polarised_alpha_empty"):
        ra = 10 ** rng.uniform(-6, 2, n)
        rb = np.zeros(n)
        rb[n // 2:] = -(10 ** rng.uniform(-22, -16, n - n // 2))  # rounding residue of an empty channel: clamped too
        ga = _gradients(rng, ra)
        gb = np.zeros((3, n))
        gb[:, n // 2:] = rng.normal(size=(3, n - n // 2)) * 1e-19
        if regime == "polarised_alpha_empty":
            ra, rb, ga, gb = rb, ra, gb, ga
    elif regime == "polarisation_1e4_1e12":
        ra = 10 ** rng.uniform(-4, 2, n)
        rb = ra * 10 ** -rng.uniform(4, 12, n)
        ga, gb = _gradients(rng, ra), _gradients(rng, rb)
        swap = np.arange(n) % 2 == 1
        ra[swap], rb[swap] = rb[swap], ra[swap]
        ga[:, swap], gb[:, swap] = gb[:, swap], ga[:, swap]
    elif regime == "core":
        ra = rng.uniform(30, 1000, n)
        rb = ra * rng.uniform(0.8, 1.25, n)
    elif regime == "tails":
        ra = 10 ** rng.uniform(-13, -9, n)
        rb = ra * 10 ** rng.uniform(-1, 1, n)
    elif regime == "zero_gradient":
        ga = np.zeros((3, n))
        gb = np.zeros((3, n))
    elif regime == "antiparallel":
        ga = _gradients(rng, ra)
        gb = -ga * ((rb / ra) ** (4 / 3) * 10 ** rng.uniform(-1, 1, n))[None, :]
    elif regime == "at_floor":
        # rho_a + rho_b exactly the floor (dropped: the test is >) and exactly one ulp above it (kept); the larger
        # channel lies in [floor / 2, 3 floor / 4], so the difference and the sum are exact in float64
        big = floor * rng.uniform(0.5, 0.75, n)
        total = np.where(np.arange(n) % 2 == 0, floor, np.nextafter(floor, np.inf))
        small = total - big
        for b, s, t in zip(big, small, total):
            assert Fraction(float(b)) + Fraction(float(s)) == Fraction(float(t)) and float(b) + float(s) == float(t)
        flip = np.arange(n) % 4 >= 2
        ra, rb = np.where(flip, small, big), np.where(flip, big, small)
    elif regime != "existing":
        raise ValueError(regime)
    if ga is None:
        ga, gb = _gradients(rng, ra), _gradients(rng, rb)
    w = rng.uniform(0.1, 2.0, n)
    return np.stack([ra, rb]), np.stack([ga, gb]), w


@lru_cache(maxsize=None)
def regime_reference(name: str, regime: str, floor: float):
    return functional_reference(name, *regime_inputs(regime, floor), floor)


# ------------------------------------------------------------------------------------------ extended-precision sums
def _two_prod(x, y):
    """x y = p + e exactly (Dekker / Veltkamp), float64 arrays."""
    p = x * y
    c = 134217729.0
    xh = c * x
    xh = xh - (xh - x)
    xl = x - xh
    yh = c * y
    yh = yh - (yh - y)
    yl = y - yh
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


def matmul(a, b):
    """a @ b in extended precision: longdouble, or, where that is no wider than float64, error-free products
    summed by math.fsum (each entry then correctly rounded to float64)."""
    if HAVE_LONGDOUBLE:
        return np.asarray(a, dtype=LD) @ np.asarray(b, dtype=LD)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[1]))
    for i in range(a.shape[0]):
        p, e = _two_prod(a[i][:, None], b)
        out[i] = [math.fsum(np.concatenate([p[:, j], e[:, j]])) for j in range(b.shape[1])]
    return out


def rowdot(a, b):
    """sum_n a[..., n] b[..., n] in extended precision."""
    if HAVE_LONGDOUBLE:
        return (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)).sum(axis=-1)
    p, e = _two_prod(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    both = np.concatenate([p, e], axis=-1)
    return np.apply_along_axis(math.fsum, -1, both)


# ------------------------------------------------------------------------------------------ contractions
def rho_reference(ao, dao, dm):
    """rho (2, G) and grad rho (2, 3, G) of a symmetric two-spin density matrix, with the rounding bound of a float64
    evaluation in any order: the two nested sums (c = ao D: nao terms; c . ao: nao terms) as dot products, so
    |err| <= 2 (2 nao + 4) u sum_mn |ao_gm| |D_mn| |ao_gn| (|dao| in place of the second |ao|, and the exact factor 2,
    for the gradient); the leading 2 covers the order in which the matrix cores accumulate."""
    nao = ao.shape[1]
    rho, grad, brho, bgrad = [], [], [], []
    fac = 2.0 * (2 * nao + 4) * U
    for x in range(2):
        c = matmul(ao, dm[x])
        cabs = np.abs(ao) @ np.abs(dm[x])
        rho.append(rowdot(c, ao))
        grad.append(np.stack([2 * rowdot(c, dao[a]) for a in range(3)]))
        brho.append(fac * (cabs * np.abs(ao)).sum(axis=1))
        bgrad.append(np.stack([2.0 * fac * (cabs * np.abs(dao[a])).sum(axis=1) for a in range(3)]))
    return np.stack(rho), np.stack(grad), np.stack(brho), np.stack(bgrad)


def vmat_reference(ao, dao, vr, vec):
    """v (2, nao, nao) = ao^T half + (ao^T half)^T, half = vr / 2 ao + vec . dao, with the bound (G + 8) u (A + A^T),
    A_mn = sum_g |ao_gm| |half|_gn: a dot product over G grid points; the 8 covers the four terms of ``half`` (whose
    magnitude is taken term by term, |vr| / 2 |ao| + sum |vec| |dao|, so that it bounds the rounding of a ``half``
    that cancels), the chunk sums and the symmetrisation."""
    npts = ao.shape[0]
    out, bound = [], []
    ao_l, dao_l = np.asarray(ao, dtype=LD), np.asarray(dao, dtype=LD)
    for x in range(2):
        half = 0.5 * np.asarray(vr[x], dtype=LD)[:, None] * ao_l
        habs = 0.5 * np.abs(vr[x])[:, None] * np.abs(ao)
        for a in range(3):
            half = half + np.asarray(vec[x, a], dtype=LD)[:, None] * dao_l[a]
            habs = habs + np.abs(vec[x, a])[:, None] * np.abs(dao[a])
        if HAVE_LONGDOUBLE:
            v = ao_l.T @ half
        else:  # (half is float64 here: its own rounding, four terms, is inside the bound's 8)
            v = matmul(np.ascontiguousarray(ao.T), np.asarray(half, dtype=np.float64))
        babs = np.abs(ao).T @ habs
        out.append(v + v.T)
        bound.append((npts + 8) * U * (babs + babs.T))
    return np.stack(out), np.stack(bound)


# ------------------------------------------------------------------------------------------ point-wise producers
def becke_reference(pts, centres, aij, inv_dist, owner: int):
    """Becke's cell share of atom ``owner`` (three smoothing iterations, size adjustment a_ij) in longdouble."""
    pts, centres, aij, inv = (np.asarray(x, dtype=LD) for x in (pts, centres, aij, inv_dist))
    natm = centres.shape[0]
    rg = np.sqrt(((pts[:, None, :] - centres[None, :, :]) ** 2).sum(axis=-1))
    mu = (rg[:, :, None] - rg[:, None, :]) * inv[None]
    f = mu + aij[None] * (1 - mu * mu)
    for _ in range(3):
        f = (3 * f - f ** 3) / 2
    s = (1 - f) / 2
    s[:, np.arange(natm), np.arange(natm)] = 1
    cell = s.prod(axis=2)
    return cell[:, owner] / cell.sum(axis=1)


def ao_reference(shells, pts):
    """Contracted Cartesian Gaussians x^l y^m z^n sum_k c_k exp(-a_k r^2) and their gradients straight from shell
    data ``[(centre (3,), exps (K,), coefs (ncomp, K), lmn [(l, m, n)] * ncomp)]`` -> ``(ao (G, ncart), dao (3, G,
    ncart), bound_ao, bound_dao)``.  The bound of a float64 evaluation, per entry:
        4 u |poly| sum_k |c_k| exp(-a_k r^2) (K + 4 + a_k r^2)  +  the smallest normal float64
    K + 4 roundings in the contraction sum and the polynomial, a_k r^2 u from the rounded argument of the exponential,
    4 for an exponential good to a few ulp; results below the normal range are absolute (they may flush to zero).
    The gradient's two terms (poly x_i sum_k -2 a_k c_k e_k and l_i poly / x_i sum_k c_k e_k) are bounded alike."""
    pts = np.asarray(pts, dtype=LD)
    ncart = sum(len(lmn) for _, _, _, lmn in shells)
    npts = pts.shape[0]
    ao, dao = np.zeros((npts, ncart), dtype=LD), np.zeros((3, npts, ncart), dtype=LD)
    bao, bdao = np.zeros((npts, ncart)), np.zeros((3, npts, ncart))
    tiny = float(np.finfo(np.float64).tiny)
    col = 0
    for centre, exps, coefs, lmns in shells:
        d = pts - np.asarray(centre, dtype=LD)[None, :]
        r2 = (d * d).sum(axis=1)
        a = np.asarray(exps, dtype=LD)
        nk = a.shape[0]
        arg = r2[:, None] * a[None, :]
        ex = np.exp(-arg)                                   # (G, K)
        ops = (nk + 4 + arg).astype(np.float64)             # roundings per primitive
        exf = ex.astype(np.float64)
        for ic, lmn in enumerate(lmns):
            c = np.asarray(coefs[ic], dtype=LD)
            rad = ex @ c
            drad = ex @ (c * (-2 * a))
            rad_b = (exf * ops) @ np.abs(np.asarray(coefs[ic], dtype=np.float64))
            drad_b = (exf * ops) @ np.abs(np.asarray(coefs[ic], dtype=np.float64) * 2 * np.asarray(exps, dtype=np.float64))
            poly = np.ones(npts, dtype=LD)
            for ax in range(3):
                poly = poly * d[:, ax] ** lmn[ax]
            ao[:, col] = poly * rad
            bao[:, col] = 4 * U * np.abs(poly).astype(np.float64) * rad_b + tiny
            for ax in range(3):
                g = poly * drad * d[:, ax]
                gb = np.abs(poly * d[:, ax]).astype(np.float64) * drad_b
                if lmn[ax]:
                    lower = np.ones(npts, dtype=LD)
                    for bx in range(3):
                        lower = lower * d[:, bx] ** (lmn[bx] - (1 if bx == ax else 0))
                    g = g + lmn[ax] * lower * rad
                    gb = gb + lmn[ax] * np.abs(lower).astype(np.float64) * rad_b
                dao[ax, :, col] = g
                bdao[ax, :, col] = 4 * U * gb + tiny
            col += 1
    return ao, dao, bao, bdao
