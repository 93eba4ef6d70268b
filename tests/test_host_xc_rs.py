"""``cam-b3lyp`` and ``lc-blyp`` on the host: ``nbed_amd.xc.energy_density`` under autograd, with XCProvider's conventions,
against the 50-digit reference of tests/xc_rs_reference.py in every regime of tests/xc_reference.py and at chosen values
of the attenuation parameter a; the branch rule of F(a); anchors that do not rest on the transcription.

Bounds: those of tests/test_host_xc_gga.py -- per entry 5e-11 of the sum of the magnitudes of the pieces' exact
contributions, 1e-12 on E_xc and the electron count.  The loose rule of ``tails`` and ``at_floor`` (4 x the error of the
reference's own 53-bit evaluation) is not used: no regime needs it.

Measured (64 points per regime, 16 per chosen a; worst entry of the two names; the reference's own 53-bit evaluation
beside it):

  regime                    host                 reference at 53 bits
  existing                  1.6e-14 (lc-blyp)    2.3e-09
  closed_shell              2.1e-14 (lc-blyp)    1.1e-10
  polarised_beta_empty      2.4e-14 (lc-blyp)    5.0e-13
  polarised_alpha_empty     1.7e-14 (lc-blyp)    3.3e-13
  polarisation_1e4_1e12     1.9e-14 (lc-blyp)    1.5e-14
  core                      7.7e-15 (lc-blyp)    5.0e-15
  tails                     3.5e-14 (cam-b3lyp)  1.2e-07
  zero_gradient             2.3e-15 (cam-b3lyp)  4.5e-15
  antiparallel              2.7e-14 (lc-blyp)    5.7e-09
  at_floor                  7.5e-14 (cam-b3lyp)  1.5e-06
  a = 0.5 (1 - 2^-20)       3.4e-14 (lc-blyp)    4.5e-14
  a = 0.5 (1 + 2^-20)       6.3e-15 (lc-blyp)    6.1e-15
  a = 1e-6                  1.9e-15 (cam-b3lyp)  7.4e-16
  a = 1e4                   2.1e-15 (lc-blyp)    1.0e-14

The right-hand column is no guide here.  The reference differentiates e = -rho^(4/3) G F(a) symbolically, and the sigma
derivative comes out as G' F + G F' da/dsigma = G' (F + a F' / 2); for large a both terms are t G' / 9 with opposite
signs (t = 1 / (4 a^2)) and the sum is of order t^2: 27 a^2 ulp are lost in 53 bits, 1.5e-6 at a = 5e3.  The first version
of ``nbed_amd.xc._b88_sr`` had the same form and failed this test in ``existing`` (2.1e-10) and ``antiparallel``
(1.0e-9); it now writes the energy through a alone where F is summed as a series (see its docstring).
"""

from pathlib import Path

import numpy as np
import pytest

import xc_gga_reference as gr
import xc_reference as xr
import xc_rs_reference as rs
from test_host_xc_gga import FLOOR, host_functional


def host_functional_at(name, omega, rho, grad, w, floor):
    """``host_functional`` at another range separation than the functional's own."""
    import torch

    from nbed_amd import xc

    rho, grad, wt = torch.tensor(rho), torch.tensor(grad), torch.tensor(w)
    keep = ((rho[0] + rho[1]) > floor).to(torch.float64)
    tra = torch.clamp(rho[0], min=0.5 * floor).requires_grad_(True)
    trb = torch.clamp(rho[1], min=0.5 * floor).requires_grad_(True)
    saa = ((grad[0] * grad[0]).sum(dim=0) + 1e-40).requires_grad_(True)
    sab = (grad[0] * grad[1]).sum(dim=0).requires_grad_(True)
    sbb = ((grad[1] * grad[1]).sum(dim=0) + 1e-40).requires_grad_(True)
    exc = (wt * keep * xc.energy_density(name, tra, trb, saa, sab, sbb, omega=omega)).sum()
    vra, vrb, vsaa, vsab, vsbb = (x if x is not None else torch.zeros_like(wt) for x in torch.autograd.grad(
        exc, (tra, trb, saa, sab, sbb), allow_unused=True))
    vr = torch.stack([vra, vrb]).numpy()
    vec = torch.stack([2.0 * vsaa * grad[0] + vsab * grad[1], 2.0 * vsbb * grad[1] + vsab * grad[0]]).numpy()
    return vr, vec, float(exc.detach()), float((wt * (rho[0] + rho[1])).sum())


# ------------------------------------------------------------------ (a) the host expression against the reference
@pytest.mark.parametrize("regime", xr.REGIMES)
@pytest.mark.parametrize("name", rs.FUNCTIONALS)
def test_host_energy_density_against_the_50_digit_reference(name, regime):
    rho, grad, w = rs.regime_inputs(regime, FLOOR)
    assert rho.shape[1] == 64
    ref = rs.regime_reference(name, regime, FLOOR)
    print(f"XCREF own {name} {regime} entries {gr.own_error(ref):.2e} exc {ref[6][2]:.2e}")
    gr.check_functional(f"host {name} {regime}", host_functional(name, rho, grad, w, FLOOR), ref, gr.ENTRY_BOUND)


@pytest.mark.parametrize("case", [c[0] for c in rs.A_CASES])
@pytest.mark.parametrize("name", rs.FUNCTIONALS)
def test_host_energy_density_at_chosen_a(name, case):
    """a just below and just above the switch point of F (both branches, one function), a = 1e-6 and a = 1e4."""
    omega, rho, grad, w = rs.a_case_inputs(case)
    a_t = dict((c[0], c[2]) for c in rs.A_CASES)[case]
    a = rs.channel_a(rho, grad, omega)
    assert np.all(np.abs(a[0] / a_t - 1) < 1e-12) and np.all((a[1] > 0.49 * a_t) & (a[1] < 2.01 * a_t))
    if case.endswith("switch"):
        assert np.all(a[0] < rs.SWITCH) == (case == "below_switch") and np.all(a[0] >= rs.SWITCH) == (case == "above_switch")
    ref = rs.a_case_reference(name, case, FLOOR)
    print(f"XCREF own {name} {case} entries {gr.own_error(ref):.2e}")
    gr.check_functional(f"host {name} {case}", host_functional_at(name, omega, rho, grad, w, FLOOR), ref, gr.ENTRY_BOUND)


def test_aliases_and_parameters():
    from nbed_amd import _nbx, xc

    rho, grad, w = rs.regime_inputs("existing", FLOOR)
    for alias in ("camb3lyp", "CAM-B3LYP", "cam-b3lyp "):
        a, b = host_functional(alias, rho, grad, w, FLOOR), host_functional("cam-b3lyp", rho, grad, w, FLOOR)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert xc.rsh_parameters("cam-b3lyp") == xc.rsh_parameters("CAMB3LYP") == (0.33, 0.19, 0.46)
    assert xc.rsh_parameters("lc-blyp") == (0.33, 0.0, 1.0)
    assert (float(rs.OMEGA), float(rs.ALPHA), float(rs.BETA)) == (0.33, 0.19, 0.46)
    for name, hyb in xc.HYBRID_FRACTION.items():  # the others: (0, hybrid fraction, 0), and the old meaning kept
        assert xc.rsh_parameters(name) == (0.0, hyb, 0.0) and xc.hybrid_fraction(name) == hyb
    assert xc.hybrid_fraction("cam-b3lyp") == 0.19 and xc.hybrid_fraction("lc-blyp") == 0.0
    for bad in ("pbe0", "wb97x", "cam-b3lyp-d3"):
        with pytest.raises(ValueError, match="not in nbed_amd.xc"):
            xc.rsh_parameters(bad)
        with pytest.raises(ValueError, match="not in nbed_amd.xc"):
            xc.hybrid_fraction(bad)
    assert _nbx.XC_RS_CODES == {"cam-b3lyp": 16, "camb3lyp": 16, "lc-blyp": 17} and set(_nbx.XC_RS_CODES) == set(xc.RSH_PARAMETERS)
    assert not set(_nbx.XC_RS_CODES) & set(_nbx.XC_CODES) and max(_nbx.XC_CODES.values()) == 8
    with pytest.raises(ValueError, match="omega"):
        import torch

        one = torch.ones(1, dtype=torch.float64)
        xc.energy_density("blyp", one, one, one, one, one, omega=0.2)


# ------------------------------------------------------------------ (b) the branch rule of F
def test_series_of_F_is_derived_from_the_closed_form():
    """The coefficients the product sums (nbed_amd.xc.ITYH_SERIES, the table of csrc/xc.hip) are the formula of
    rs.series_coefficient; the formula agrees with sympy's expansion of the closed form, and series and closed form
    agree at 50 digits where both converge."""
    import mpmath as mp

    from nbed_amd import xc

    derived = rs.series_coefficients_from_the_closed_form(7)
    assert derived[0] == 0 and [rs.series_coefficient(m) for m in range(1, 8)] == [
        rs.Fraction(int(c.p), int(c.q)) for c in derived[1:]]
    assert rs.series_coefficient(1) == rs.Fraction(1, 9)  # F -> 1 / (36 a^2)
    assert len(xc.ITYH_SERIES) == rs.SERIES_TERMS == 16 and xc.ITYH_SWITCH == rs.SWITCH
    assert list(xc.ITYH_SERIES) == [float(rs.series_coefficient(m)) for m in range(1, 17)]
    src = (Path(__file__).resolve().parents[1] / "nbed_amd" / "csrc" / "xc.hip").read_text()
    table = src[src.index("constexpr double C[16]"):]
    table = table[table.index("{") + 1:table.index("}")]
    dens = [int(float(tok.split("/")[1])) * (-1 if tok.strip().startswith("-") else 1) for tok in table.split(",")]
    assert [rs.Fraction(1, d) for d in dens] == [rs.series_coefficient(m) for m in range(1, 17)]
    with mp.workdps(60):
        saved, rs.SERIES_TERMS = rs.SERIES_TERMS, 60
        try:
            for a in ("0.5", "1", "7", "1000"):
                a = mp.mpf(a)
                assert abs(rs._series_f(a) / rs.f_exact(a) - 1) < mp.mpf(10) ** -50
                assert abs(rs._series_df(a) / rs.df_exact(a) - 1) < mp.mpf(10) ** -50
                assert abs(mp.diff(rs.f_exact, a) / rs.df_exact(a) - 1) < mp.mpf(10) ** -40  # the derivative is F's
        finally:
            rs.SERIES_TERMS = saved


def test_switch_point_is_where_both_branches_are_at_their_best():
    """Measured 53-bit errors of the closed form and of the sixteen-term series, F and a F', against 50 digits: at the
    switch both are within a few ulp; a step below it the series is not, a step above it the closed form starts to
    lose 36 a^4 ulp, and at a = 100 it is wrong in the seventh digit."""
    at = {a: rs.branch_errors(a) for a in (0.3, 0.4, 0.5, 0.7, 1.0, 100.0)}
    for a, e in at.items():
        print(f"XCREF F branches a = {a:g}: closed {e[0]:.1e} {e[1]:.1e}  series {e[2]:.1e} {e[3]:.1e}")
    assert max(at[0.5]) < 4e-15
    assert at[0.4][3] > 20 * max(at[0.4][:2]) and at[0.3][2] > 1e-12     # the series below the switch
    assert max(at[1.0][:2]) > 10 * max(at[1.0][2:]) and at[100.0][0] > 1e-9  # the closed form above it
    assert all(max(at[a][2:]) < 1e-15 for a in (0.5, 0.7, 1.0, 100.0)) and all(max(at[a][:2]) < 4e-15 for a in (0.3, 0.4, 0.5))


def test_host_F_on_both_sides_of_the_switch_and_at_the_guards():
    import mpmath as mp
    import torch

    from nbed_amd import xc

    vals = [0.0, 1e-300, 1e-120, 9.9e-61, 1.1e-60, 1e-6, 0.1, 0.3, np.nextafter(0.5, 0), 0.5, np.nextafter(0.5, 1), 0.7, 3.0, 1e2,
            1e4, 1e8]
    a = torch.tensor(vals, dtype=torch.float64, requires_grad=True)
    f = xc._ityh(torch, a)
    (df,) = torch.autograd.grad(f.sum(), a)
    assert torch.isfinite(f).all() and torch.isfinite(df).all() and float(f[0]) == 1.0
    with mp.workdps(50):
        for v, fv, dv in zip(vals, f.detach().numpy(), df.numpy()):
            want, dwant = rs.f_exact(mp.mpf(v)), rs.df_exact(mp.mpf(v))
            assert abs(mp.mpf(float(fv)) - want) <= 4e-15 * abs(want), v
            assert abs(mp.mpf(float(dv)) - dwant) <= 4e-15 * abs(dwant), v


# ------------------------------------------------------------------ (c) anchors
def test_lc_blyp_at_omega_zero_is_blyp():
    rho, grad, w = rs.regime_inputs("existing", FLOOR)
    blyp = gr.regime_reference("blyp", "existing", FLOOR)
    gr.check_functional("host lc-blyp(omega = 0) against blyp", host_functional_at("lc-blyp", 0.0, rho, grad, w, FLOOR), blyp,
                        gr.ENTRY_BOUND)
    ref0 = rs.functional_reference("lc-blyp", rho, grad, w, FLOOR, omega=0)
    assert gr.scaled_err(ref0[0], blyp[0], blyp[5][0]).max() < 1e-40 and gr.scaled_err(ref0[1], blyp[1], blyp[5][1]).max() < 1e-40


def test_reference_anchors():
    import mpmath as mp
    import sympy as sp

    r = sp.Symbol("r", positive=True)
    w = sp.Symbol("w", positive=True)
    # with the local-density K (no gradient) k is the Fermi wave vector of the spin channel, (6 pi^2 rho)^(1/3)
    a_lda = rs.ityh_a(r, sp.Integer(0), w)
    assert sp.simplify(a_lda - w / (2 * (6 * sp.pi ** 2 * r) ** sp.Rational(1, 3))) == 0
    # the pieces add up: cam-b3lyp is b3lyp5's correlation on 0.35 of BLYP's exchange + 0.46 of lc-blyp's
    cam = dict((label, c) for c, label in rs.pieces("cam-b3lyp"))
    assert cam["slater_a"] == cam["b88_a"] == 1 - rs.ALPHA - rs.BETA == sp.Rational(35, 100) and cam["b88sr_b"] == rs.BETA
    assert cam["vwn5"] == sp.Rational(19, 100) and cam["lyp"] == sp.Rational(81, 100)
    with mp.workdps(xr.DPS):
        assert rs.f_exact(0) == 1 and abs(rs.f_exact(mp.mpf(10) ** -30) - 1) < mp.mpf(10) ** -29
        # F -> 0 as omega -> infinity, like 1 / (36 a^2): the short-range exchange vanishes
        for a in (mp.mpf(10) ** 3, mp.mpf(10) ** 8, mp.mpf(10) ** 20):
            assert abs(rs.f_exact(a) * 36 * a * a - 1) < 1 / a
        at = [mp.mpf("0.37"), mp.mpf("0.052"), mp.mpf("0.8"), mp.mpf("-0.11"), mp.mpf("0.03")]
        e_inf = rs.point("lc-blyp", *at, omega=sp.Integer(10) ** 30)[0]
        lyp = gr._compiled("lyp")(*at)[0]
        assert abs(e_inf - lyp) < mp.mpf(10) ** -50
        # 0 < F < 1 and F falls monotonically: attenuation, never amplification
        grid = [mp.mpf(10) ** (mp.mpf(k) / 4) for k in range(-24, 25)]
        fs = [rs.f_exact(a) for a in grid]
        assert all(0 < f < 1 for f in fs) and all(x > y for x, y in zip(fs, fs[1:]))
        assert all(rs.df_exact(a) < 0 for a in grid)


def test_symbolic_derivatives_agree_with_differences_of_the_energy_density():
    import mpmath as mp

    with mp.workdps(xr.DPS):
        at = [mp.mpf("0.37"), mp.mpf("0.052"), mp.mpf("0.8"), mp.mpf("-0.11"), mp.mpf("0.03")]
        for name in rs.FUNCTIONALS:
            base = rs.point(name, *at)
            for i in range(5):
                h = abs(at[i]) * mp.mpf(10) ** -20
                up, dn = list(at), list(at)
                up[i] += h
                dn[i] -= h
                fd = (rs.point(name, *up)[0] - rs.point(name, *dn)[0]) / (2 * h)
                assert abs(fd - base[1 + i]) <= mp.mpf(10) ** -25 * max(abs(fd), mp.mpf(10) ** -10), (name, i)
