"""Reference for the attenuated two-electron integrals (pq| erf(omega r12) / r12 |rs) of nbx_host_eri_erf /
nbx_eri_device_erf.

Derivation.  erf(omega r) / r = (2 / sqrt(pi)) int_0^omega exp(-u^2 r^2) du, and 1 / r is the same integral to infinity.
For two spherical Gaussians exp(-p |r1 - P|^2), exp(-q |r2 - Q|^2) the six-dimensional integral over the kernel
exp(-u^2 r12^2) is elementary:

    pi^3 (p q + (p + q) u^2)^(-3/2) exp(-p q u^2 |PQ|^2 / (p q + (p + q) u^2)).

With alpha = p q / (p + q) and t^2 = u^2 / (alpha + u^2) the u integral becomes
(2 pi^(5/2) / (p q sqrt(p + q))) int_0^T exp(-alpha |PQ|^2 t^2) dt with the upper limit T = omega / sqrt(alpha + omega^2)
(T = 1 for 1 / r12: the Boys function F_0(alpha |PQ|^2)).  Substituting t = T s,

    [ss|ss]_omega = (2 pi^(5/2) / (p q sqrt(p + q))) T F_0(alpha T^2 |PQ|^2),

that is the plain formula at alpha_w = alpha T^2 = alpha omega^2 / (alpha + omega^2) times omega / sqrt(alpha + omega^2).
Higher angular momenta are derivatives with respect to P and Q of this function of PQ alone, which is why the same
substitution goes into the powers (-2 alpha_w)^n of the Hermite integrals R^n_tuv, and only there: the Hermite expansion
coefficients E_t^ij describe the charge distributions and do not see the operator.

``eri_erf_prim`` / ``eri_erf_element`` restate the primitive integral with that substitution on the oracle's scalar
recursions (``oracle.gto._E`` and ``_R``, imported, not edited) -- written from the formula above, not from
csrc/ints_md.h.  ``ssss_closed_form`` is the closed form in mpmath at 50 digits and ``ssss_quadrature`` the
u integral of the first display done numerically at 50 digits: the derivation's starting point, with no Boys function
and no alpha_w in it.
"""

from __future__ import annotations

import math

import numpy as np

from oracle.gto import SphericalBasis, _E, _R, parse_xyz  # noqa: F401  (the bases are re-exported for the tests)


def eri_erf_prim(a, lmn1, A, b, lmn2, B, c, lmn3, C, d, lmn4, D, omega):
    """[ab| erf(omega r12) / r12 |cd] of four unnormalised Cartesian primitives."""
    p, q = a + b, c + d
    alpha = p * q / (p + q)
    alpha_w = alpha * omega * omega / (alpha + omega * omega)
    scale = omega / math.sqrt(alpha + omega * omega)
    P = (a * np.asarray(A) + b * np.asarray(B)) / p
    Q = (c * np.asarray(C) + d * np.asarray(D)) / q
    pq = P - Q
    r2 = float(pq @ pq)
    bra = [[_E(lmn1[k], lmn2[k], t, A[k] - B[k], a, b) for t in range(lmn1[k] + lmn2[k] + 1)] for k in range(3)]
    ket = [[_E(lmn3[k], lmn4[k], t, C[k] - D[k], c, d) for t in range(lmn3[k] + lmn4[k] + 1)] for k in range(3)]
    val = 0.0
    for t, ex in enumerate(bra[0]):
        for u, ey in enumerate(bra[1]):
            for v, ez in enumerate(bra[2]):
                for tau, fx in enumerate(ket[0]):
                    for nu, fy in enumerate(ket[1]):
                        for phi, fz in enumerate(ket[2]):
                            sign = -1.0 if (tau + nu + phi) & 1 else 1.0
                            val += sign * ex * ey * ez * fx * fy * fz * _R(t + tau, u + nu, v + phi, 0, alpha_w, pq[0], pq[1],
                                                                           pq[2], r2)
    return val * scale * 2.0 * math.pi**2.5 / (p * q * math.sqrt(p + q))


def eri_erf_element(basis: SphericalBasis, p: int, q: int, r: int, s: int, omega: float) -> float:
    """One (pq| erf(omega r12) / r12 |rs) over the AOs of an ``oracle.gto.SphericalBasis``."""
    (A, t1, e1, c1), (B, t2, e2, c2), (C, t3, e3, c3), (D, t4, e4, c4) = (basis.aos[i] for i in (p, q, r, s))
    val = 0.0
    for w1, l1 in t1:
        for w2, l2 in t2:
            for w3, l3 in t3:
                for w4, l4 in t4:
                    acc = 0.0
                    for a, ca in zip(e1, c1):
                        for b, cb in zip(e2, c2):
                            for c, cc in zip(e3, c3):
                                for d, cd in zip(e4, c4):
                                    acc += ca * cb * cc * cd * eri_erf_prim(a, l1, A, b, l2, B, c, l3, C, d, l4, D, omega)
                    val += w1 * w2 * w3 * w4 * acc
    return val


def _mp_geometry(mp, exps, centres):
    a, b, c, d = (mp.mpf(float(x)) for x in exps)
    A, B, C, D = ([mp.mpf(float(x)) for x in v] for v in centres)
    p, q = a + b, c + d
    P = [(a * x + b * y) / p for x, y in zip(A, B)]
    Q = [(c * x + d * y) / q for x, y in zip(C, D)]
    kab = mp.exp(-a * b / p * sum((x - y) ** 2 for x, y in zip(A, B)))
    kcd = mp.exp(-c * d / q * sum((x - y) ** 2 for x, y in zip(C, D)))
    return p, q, kab * kcd, sum((x - y) ** 2 for x, y in zip(P, Q))


def ssss_closed_form(exps, centres, omega, dps: int = 50):
    """[ss|ss]_omega of four unnormalised s primitives exp(-a |r - A|^2), mpmath at ``dps`` digits (an mpf)."""
    import mpmath as mp

    with mp.workdps(dps):
        p, q, k, r2 = _mp_geometry(mp, exps, centres)
        w = mp.mpf(float(omega))
        alpha = p * q / (p + q)
        x = alpha * w * w / (alpha + w * w) * r2
        f0 = mp.mpf(1) if x == 0 else mp.sqrt(mp.pi / x) * mp.erf(mp.sqrt(x)) / 2
        return +(2 * mp.pi ** mp.mpf("2.5") / (p * q * mp.sqrt(p + q)) * k * w / mp.sqrt(alpha + w * w) * f0)


def ssss_quadrature(exps, centres, omega, dps: int = 50):
    """The same number from (2 / sqrt pi) int_0^omega du of the Gaussian-kernel integral, by mpmath's quadrature."""
    import mpmath as mp

    with mp.workdps(dps):
        p, q, k, r2 = _mp_geometry(mp, exps, centres)
        w = mp.mpf(float(omega))

        def kernel(u):
            den = p * q + (p + q) * u * u
            return mp.pi**3 * den ** mp.mpf("-1.5") * mp.exp(-p * q * u * u * r2 / den)

        # the integrand varies on the scale sqrt(alpha) ~ 1: break the range there so a large omega does not hide it
        pts = sorted({mp.mpf(0), w} | {mp.mpf(x) for x in (0.25, 1, 4, 16, 64, 256) if x < w})
        return +(2 / mp.sqrt(mp.pi) * k * mp.quad(kernel, pts))
