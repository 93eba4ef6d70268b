"""PBE, PBEH, BLYP, B3LYP5 and Slater + PW92 on the host: ``nbed_amd.xc.energy_density`` under autograd, with
XCProvider's conventions, against the 50-digit references of tests/xc_gga_reference.py; anchors of those references
that do not rest on their transcription; and the product path (quadrature, mean field, embedding) with ``pbe``.

Bounds.  Per entry of ``vr`` and ``vec``: the error against the 50-digit value, divided by the sum of the magnitudes
of the pieces' exact contributions to that entry (at least 1e-150: a condition, as in tests/xc_reference.py), below
5e-11 -- in the regimes ``tails`` and ``at_floor`` below max(5e-11, 4 x the error of the reference's own 53-bit
evaluation).  E_xc: 1e-12 of sum_g w |piece|; the electron count: 1e-12.

Measured (64 points per regime, worst entry over the five names and the name it belongs to; the error of the
reference's own 53-bit evaluation beside it):

  regime                    host               reference at 53 bits
  existing                  9.8e-15 (pbeh)     1.4e-14
  closed_shell              1.5e-14 (b3lyp5)   2.2e-14
  polarised_beta_empty      2.0e-12 (pbe)      2.2e-11
  polarised_alpha_empty     5.3e-13 (pbe)      1.9e-11
  polarisation_1e4_1e12     9.4e-14 (pbe)      3.2e-13
  core                      3.5e-14 (pbe)      5.1e-15
  tails                     3.2e-14 (pbe)      8.9e-14
  zero_gradient             2.2e-15 (pbeh)     4.7e-15
  antiparallel              4.2e-13 (pbeh)     1.5e-13
  at_floor                  4.5e-14 (b3lyp5)   1.5e-13

so no regime needs more than 5e-11: with expm1 / log1p the two regimes the textbook evaluation lost (8.6e-11 in
``tails``, 1.3e-10 in ``at_floor``, both through exp(.) - 1) sit at 5e-14.  What does lose digits under autograd is
the quotient (1 + y) / (1 + y + y^2) of H at a large reduced gradient (y = A t^2 to 1e7): differentiated term by term
it cancels to 1 / y^2 of its terms and put vec at 8.6e-11 in ``polarised_alpha_empty``; ``nbed_amd.xc._pbe_c`` writes
it as 1 - 1 / (1 + y + y^2) there.
"""

import math

import numpy as np
import pytest

import xc_gga_reference as gr
import xc_reference as xr

FLOOR = 1e-14  # XCProvider.RHO_FLOOR (asserted below)
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"


def host_functional(name, rho, grad, w, floor):
    """(vr, vec, E_xc, electron count) as XCProvider.__call__ forms them on the host."""
    import torch

    from nbed_amd import xc

    rho, grad, wt = torch.tensor(rho), torch.tensor(grad), torch.tensor(w)
    keep = ((rho[0] + rho[1]) > floor).to(torch.float64)
    tra = torch.clamp(rho[0], min=0.5 * floor).requires_grad_(True)
    trb = torch.clamp(rho[1], min=0.5 * floor).requires_grad_(True)
    saa = ((grad[0] * grad[0]).sum(dim=0) + 1e-40).requires_grad_(True)
    sab = (grad[0] * grad[1]).sum(dim=0).requires_grad_(True)
    sbb = ((grad[1] * grad[1]).sum(dim=0) + 1e-40).requires_grad_(True)
    exc = (wt * keep * xc.energy_density(name, tra, trb, saa, sab, sbb)).sum()
    if not exc.requires_grad:  # every point dropped
        zero = torch.zeros_like(wt)
        vra = vrb = vsaa = vsab = vsbb = zero
    else:
        vra, vrb, vsaa, vsab, vsbb = (x if x is not None else torch.zeros_like(wt) for x in torch.autograd.grad(
            exc, (tra, trb, saa, sab, sbb), allow_unused=True))
    vr = torch.stack([vra, vrb]).numpy()
    vec = torch.stack([2.0 * vsaa * grad[0] + vsab * grad[1], 2.0 * vsbb * grad[1] + vsab * grad[0]]).numpy()
    return vr, vec, float(exc.detach()), float((wt * (rho[0] + rho[1])).sum())


# ------------------------------------------------------------------ (a) the host expression against the reference
@pytest.mark.parametrize("regime", xr.REGIMES)
@pytest.mark.parametrize("name", gr.FUNCTIONALS)
def test_host_energy_density_against_the_50_digit_reference(name, regime):
    from nbed_amd import xc

    assert xc.XCProvider.RHO_FLOOR == FLOOR
    rho, grad, w = gr.regime_inputs(regime, FLOOR)
    assert rho.shape[1] == 64
    ref = gr.regime_reference(name, regime, FLOOR)
    print(f"XCREF own {name} {regime} entries {gr.own_error(ref):.2e} exc {ref[6][2]:.2e}")
    gr.check_functional(f"host {name} {regime}", host_functional(name, rho, grad, w, FLOOR), ref, gr.entry_bound(regime, ref))


def test_aliases_name_the_same_expression():
    rho, grad, w = gr.regime_inputs("existing", FLOOR)
    for alias, name in (("pbe,pbe", "pbe"), ("PBE", "pbe"), ("pbe1pbe", "pbeh"), ("B3LYP5", "b3lyp5")):
        a, b = host_functional(alias, rho, grad, w, FLOOR), host_functional(name, rho, grad, w, FLOOR)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ------------------------------------------------------------------ (b) anchors that do not rest on the transcription
def _hydrogen_quadrature(n=240, rmax=40.0):
    """Gauss-Legendre nodes on three stretches of (0, rmax) with 4 pi r^2 dr weights, and the exact density."""
    x, wx = np.polynomial.legendre.leggauss(n // 3)
    r, w = [], []
    for lo, hi in ((0.0, 1.0), (1.0, 8.0), (8.0, rmax)):
        r.append(0.5 * (hi - lo) * x + 0.5 * (hi + lo))
        w.append(0.5 * (hi - lo) * wx)
    r, w = np.concatenate(r), np.concatenate(w)
    return r, 4.0 * math.pi * r * r * w


# Perdew, Burke and Ernzerhof, Phys. Rev. Lett. 77, 3865 (1996), table I, hydrogen atom (Hartree): exchange and
# correlation energies of the exact density, LSD and PBE
PAPER_H = {"x_lsd": -0.2680, "c_lsd": -0.0222, "x_pbe": -0.3059, "c_pbe": -0.0060}


def test_hydrogen_atom_energies_of_the_pbe_paper_reference():
    import mpmath as mp

    r, w = _hydrogen_quadrature()
    with mp.workdps(30):
        got = dict.fromkeys(PAPER_H, mp.mpf(0))
        for rg, wg in zip(r, w):
            ra = mp.exp(-2 * mp.mpf(float(rg))) / mp.pi  # all spin up; |grad rho| = 2 rho
            args = (ra, mp.mpf(10) ** -300, 4 * ra * ra, mp.mpf(0), mp.mpf(0))
            wg = mp.mpf(float(wg))
            got["x_lsd"] += wg * gr._compiled("slater_a")(*args)[0]
            got["c_lsd"] += wg * gr._compiled("pw_mod")(*args)[0]
            got["x_pbe"] += wg * (gr._compiled("pbe_x_a")(*args)[0] + gr._compiled("pbe_x_b")(*args)[0])
            got["c_pbe"] += wg * (gr._compiled("pw_mod")(*args)[0] + gr._compiled("pbe_h")(*args)[0])
    print("XCREF hydrogen reference", {k: float(v) for k, v in got.items()})
    for key, paper in PAPER_H.items():
        assert abs(float(got[key]) - paper) < 5e-5, (key, float(got[key]), paper)


def test_hydrogen_atom_energies_of_the_pbe_paper_host():
    import torch

    from nbed_amd import xc

    r, w = _hydrogen_quadrature()
    ra = torch.tensor(np.exp(-2.0 * r) / np.pi)
    rb = torch.full_like(ra, 1e-30)
    z = torch.zeros_like(ra)
    wt = torch.tensor(w)
    got = {"x_lsd": float((wt * xc._slater(torch, ra, rb)).sum()), "c_lsd": float((wt * xc._pw_mod(torch, ra, rb)).sum()),
           "x_pbe": float((wt * xc._pbe_x(torch, ra, rb, 4.0 * ra * ra, z)).sum()),
           "c_pbe": float((wt * xc._pbe_c(torch, ra, rb, 4.0 * ra * ra, z, z)).sum())}
    print("XCREF hydrogen host", got)
    for key, paper in PAPER_H.items():
        assert abs(got[key] - paper) < 5e-5, (key, got[key], paper)
    # and on the product's own grid
    pts, wts = xc.build_grid([("H", np.zeros(3))], n_rad=80, n_theta=8)
    ra = torch.tensor(np.exp(-2.0 * np.linalg.norm(pts, axis=1)) / np.pi)
    keep = (ra > FLOOR).to(torch.float64)  # the product's conventions: the empty tail is dropped, densities clamped
    z = torch.zeros_like(ra)
    e = float((torch.tensor(wts) * keep * xc.energy_density("pbe", ra.clamp(min=0.5 * FLOOR), z + 0.5 * FLOOR,
                                                            4.0 * ra * ra + 1e-40, z, z + 1e-40)).sum())
    assert abs(e - (PAPER_H["x_pbe"] + PAPER_H["c_pbe"])) < 1e-4  # (two four-decimal figures)


def test_pbe_without_a_gradient_is_the_local_functional():
    """F(0) = 1 and H(t = 0) = 0: on ``zero_gradient`` (sigma_ss = 1e-40) pbe is lda,pw_mod, to the entry bound."""
    rho, grad, w = gr.regime_inputs("zero_gradient", FLOOR)
    lda = gr.regime_reference("lda,pw_mod", "zero_gradient", FLOOR)
    gr.check_functional("host pbe against lda,pw_mod zero_gradient", host_functional("pbe", rho, grad, w, FLOOR), lda,
                        gr.ENTRY_BOUND)
    pbe = gr.regime_reference("pbe", "zero_gradient", FLOOR)
    assert gr.scaled_err(pbe[0], lda[0], lda[5][0]).max() < gr.ENTRY_BOUND and not np.any(pbe[1])  # (the references too)


def test_reference_anchors():
    import mpmath as mp
    import sympy as sp

    s2 = sp.Symbol("s2", positive=True)
    assert gr.pbe_enhancement(sp.Integer(0)) == 1
    assert sp.simplify(sp.limit(gr.pbe_enhancement(s2), s2, sp.oo) - (1 + gr.KAPPA)) == 0  # the Lieb-Oxford bound
    assert abs(float(gr.MU) - 0.2195149727645171) < 1e-16
    # PBE exchange contains the Slater exchange
    assert sp.simplify(gr.pbe_x_expr().subs({gr.SAA: 0, gr.SBB: 0}) - xr.slater_expr()) == 0
    # H vanishes without a gradient
    assert sp.simplify(gr.pbe_h_expr().subs({gr.SAA: 0, gr.SAB: 0, gr.SBB: 0})) == 0
    assert sp.simplify(gr.pbe_h_expr(stable=True).subs({gr.SAA: 0, gr.SAB: 0, gr.SBB: 0})) == 0
    # b3lyp5 is b3lyp with 0.19 of the correlation fit exchanged
    diff = gr.energy_density_expr("b3lyp5") - xr.energy_density_expr("b3lyp") - sp.Rational(19, 100) * (
        xr.vwn5_expr() - xr.vwn_rpa_expr())
    assert sp.expand(diff) == 0
    assert sp.expand(gr.energy_density_expr("b3lyp") - xr.energy_density_expr("b3lyp")) == 0  # (the pieces add up)
    assert sp.expand(gr.energy_density_expr("blyp") - xr.slater_expr() - xr.b88_expr() - xr.lyp_expr()) == 0
    assert sp.expand(gr.energy_density_expr("pbe") - gr.energy_density_expr("pbeh") - gr.pbe_x_expr() / 4) == 0
    with mp.workdps(xr.DPS):
        # the two ways of writing exp(.) - 1 and ln(1 + .) are the same function at 50 digits
        at = [mp.mpf("0.37"), mp.mpf("0.052"), mp.mpf("0.8"), mp.mpf("-0.11"), mp.mpf("0.03")]
        for label in ("pw_mod", "pbe_h"):
            for a, b in zip(gr._compiled(label, False)(*at), gr._compiled(label, True)(*at)):
                assert abs(a - b) <= mp.mpf(10) ** -44 * abs(a)
        # H -> -eps as t -> infinity (the correlation energy vanishes at a large reduced gradient)
        big = mp.mpf(10) ** 40
        eps = gr._compiled("pw_mod")(at[0], at[1], big, 0, big)[0]
        h = gr._compiled("pbe_h")(at[0], at[1], big, 0, big)[0]
        assert abs(h + eps) < mp.mpf(10) ** -30 * abs(eps)


def test_symbolic_derivatives_agree_with_differences_of_the_energy_density():
    """The compiled derivatives against central differences of the compiled energy density at 50 digits (step 1e-20
    relative: truncation 1e-40) -- a wrong ``diff`` or a wrong output order would show."""
    import mpmath as mp

    with mp.workdps(xr.DPS):
        at = [mp.mpf("0.37"), mp.mpf("0.052"), mp.mpf("0.8"), mp.mpf("-0.11"), mp.mpf("0.03")]
        for name in gr.FUNCTIONALS:
            base = gr.point(name, *at)
            for i in range(5):
                h = abs(at[i]) * mp.mpf(10) ** -20
                up, dn = list(at), list(at)
                up[i] += h
                dn[i] -= h
                fd = (gr.point(name, *up)[0] - gr.point(name, *dn)[0]) / (2 * h)
                assert abs(fd - base[1 + i]) <= mp.mpf(10) ** -25 * max(abs(fd), mp.mpf(10) ** -10), (name, i)


# ------------------------------------------------------------------ (c) the product path on the CPU
def test_names_hybrid_fractions_and_codes():
    from nbed_amd import NbedConfig, _nbx, xc
    from nbed_amd.driver import BuiltinHFProvider

    want = {"pbe": 0.0, "pbe,pbe": 0.0, "pbeh": 0.25, "pbe1pbe": 0.25, "blyp": 0.0, "b3lyp5": 0.2, "lda,pw_mod": 0.0}
    for name, hyb in want.items():
        assert xc.hybrid_fraction(name) == hyb and xc.hybrid_fraction(name.upper()) == hyb
        assert name in _nbx.XC_CODES
        assert BuiltinHFProvider.supports(NbedConfig(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional=name))
    assert [_nbx.XC_CODES[n] for n in ("lda,pw_mod", "pbe", "pbe,pbe", "pbeh", "pbe1pbe", "blyp", "b3lyp5")] == [
        4, 5, 5, 6, 6, 7, 8]
    assert _nbx.NBX_VERSION == 3
    assert set(_nbx.XC_CODES) == set(xc.HYBRID_FRACTION) - {"hf"}  # every semi-local name has a kernel


def test_pbe_potential_is_the_derivative_of_the_energy():
    """v_xc is the derivative of E_xc (central difference along a random symmetric direction) for pbe on water /
    STO-3G with an open-shell density."""
    from nbed_amd import integrals, xc

    atoms = integrals.parse_geometry(WATER)
    basis = integrals.Basis(atoms, "sto-3g")
    ints = integrals.molecule_integrals(WATER, "sto-3g", "angstrom")
    prov = xc.XCProvider(atoms, basis, "pbe", n_rad=60, n_theta=18, device="cpu")
    w, c = np.linalg.eigh(ints["S"])
    x = (c / np.sqrt(w)) @ c.T
    _, u = np.linalg.eigh(x @ ints["hcore"] @ x)
    cmo = x @ u
    dm = np.stack([cmo[:, :5] @ cmo[:, :5].T, cmo[:, :4] @ cmo[:, :4].T])  # open shell on purpose
    exc, vxc = prov(dm)
    assert abs(prov.nelec_last - 9.0) < 1e-5 and exc < -8.0
    np.testing.assert_allclose(vxc, vxc.transpose(0, 2, 1), rtol=0, atol=1e-12)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(2, 7, 7)) * 1e-5  # (the central difference's own error is cubic in the step)
    d = d + d.transpose(0, 2, 1)
    fd = (prov(dm + d)[0] - prov(dm - d)[0]) / 2.0
    assert abs(fd - np.einsum("xij,xji->", vxc, d)) < 2e-9


def test_driver_pbe_in_water_without_pyscf():
    """``nbed`` with xc_functional='pbe' on the built-in provider: the global Kohn-Sham run and the embedded run
    converge and the subsystem energies add up to the global energy."""
    from oracle_backend import OracleBackend

    from nbed_amd import NbedConfig, nbed
    from nbed_amd.driver import BuiltinHFProvider

    cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional="pbe", projector="mu",
                     localization="spade", convergence=1e-8, max_hf_cycles=100, max_dft_cycles=100, run_fci_emb=False,
                     run_ccsd_emb=False)
    drv = nbed(cfg, backend=OracleBackend())
    assert isinstance(drv.provider, BuiltinHFProvider)
    ks = drv._global_ks
    assert ks.converged and drv.mu["scf"].converged
    assert abs(ks.e_tot - (-75.2218469195)) < 2e-8  # (below the UHF energy -74.9610, above B3LYP's -75.3091: the
    # device quadrature is held to this number in tests/test_gpu_xc_gga.py)
    assert abs(drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot) < 1e-8
