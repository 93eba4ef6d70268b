"""``nbed_amd.xc.energy_density`` under autograd, with XCProvider's conventions, against the 50-digit reference of
tests/xc_reference.py -- the host expression is what the CPU checker runs and what csrc/xc.hip mirrors term for term.

Bounds (those the project's kernel-against-autograd test already uses): 5e-11 relative per entry of ``vr`` and
``vec``, 1e-12 relative on E_xc and the electron count.  Condition, not tolerance: an entry whose exact value is
below 1e-150 in magnitude is measured against 1e-150 instead of itself -- LYP's exp(-c rho^(-1/3)) underflows in
float64 below rho ~ 4e-11 while the 50-digit value is 1e-2000, and nothing physical lives there.

150 points per regime, ten regimes, four functionals: 6000 reference points, 15 s.
"""

import numpy as np
import pytest

import xc_reference as xr

FLOOR = 1e-14  # XCProvider.RHO_FLOOR (asserted below)


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


@pytest.mark.parametrize("regime", xr.REGIMES)
@pytest.mark.parametrize("name", xr.FUNCTIONALS)
def test_host_energy_density_against_the_50_digit_reference(name, regime):
    from nbed_amd import xc

    assert xc.XCProvider.RHO_FLOOR == FLOOR
    rho, grad, w = xr.regime_inputs(regime, FLOOR)
    assert rho.shape[1] >= 64
    got = host_functional(name, rho, grad, w, FLOOR)
    xr.check_functional(f"host {name} {regime}", got, xr.regime_reference(name, regime, FLOOR))


def test_regimes_are_what_they_claim():
    ref = {r: xr.regime_inputs(r, FLOOR) for r in xr.REGIMES}
    rho, grad, _ = ref["at_floor"]
    tot = rho[0] + rho[1]
    assert np.all(tot[0::2] == FLOOR) and np.all(tot[1::2] == np.nextafter(FLOOR, np.inf))
    assert not xr.regime_reference("slater", "at_floor", FLOOR)[4][0::2].any()
    assert xr.regime_reference("slater", "at_floor", FLOOR)[4][1::2].all()
    rho, grad, _ = ref["polarised_beta_empty"]
    assert np.all(rho[1] <= 0.0) and (rho[1] == 0.0).any() and (rho[1] < 0.0).any() and rho[0].min() >= 1e-6
    rho, grad, _ = ref["polarised_alpha_empty"]
    assert np.all(rho[0] <= 0.0)
    rho, grad, _ = ref["polarisation_1e4_1e12"]
    ratio = np.maximum(rho[0] / rho[1], rho[1] / rho[0])
    assert ratio.min() >= 1e4 and ratio.max() > 1e11
    rho, grad, _ = ref["antiparallel"]
    assert np.all((grad[0] * grad[1]).sum(axis=0) < 0.0)
    rho, grad, _ = ref["closed_shell"]
    assert np.array_equal(rho[0], rho[1]) and np.array_equal(grad[0], grad[1])
    assert not ref["zero_gradient"][1].any()
    assert ref["core"][0].min() >= 24.0 and ref["tails"][0][0].max() <= 1e-9


# ------------------------------------------------------------------ the reference does not rest on its own transcription
def test_reference_anchors():
    import mpmath as mp
    import sympy as sp

    with mp.workdps(xr.DPS):
        # VWN5 reproduces the Ceperley-Alder energies it was fitted to (Hartree per electron; the values
        # tests/test_host_integrals.py holds the product to): paramagnetic rs = 1, 2, 5, ferromagnetic rs = 1, 2
        for rs, zeta, ca in ((1, 0, -0.0600), (2, 0, -0.0448), (5, 0, -0.0282), (1, 1, -0.0316), (2, 1, -0.0239)):
            rho = 3 / (4 * sp.pi * rs ** 3)
            ra, rb = rho * (1 + zeta) / 2, rho * (1 - zeta) / 2 + sp.Rational(1, 10 ** 300)
            assert abs(xr.evaluate_expr(xr.vwn5_expr(), ra, rb) / mp.mpf(str(sp.N(rho, 50))) - ca) < 1.2e-4
        # Slater in closed form: ra = 8, rb = 1 -> -(3/2) (3 / (4 pi))^(1/3) (16 + 1)
        want = -mp.mpf(3) / 2 * mp.cbrt(3 / (4 * mp.pi)) * 17
        assert abs(xr.evaluate_expr(xr.slater_expr(), 8, 1) - want) < mp.mpf(10) ** -45
        # and its derivative through the compiled path: de/dra = -(4/3) cx ra^(1/3) = -2 (3 / (4 pi))^(1/3) 2
        got = xr.point("slater", 8, 1, 1, 0, 1)
        assert abs(got[0] - want) < mp.mpf(10) ** -45 and abs(got[1] + 4 * mp.cbrt(3 / (4 * mp.pi))) < mp.mpf(10) ** -45
        assert got[3] == 0 and got[4] == 0 and got[5] == 0
        # B88: the enhancement tends to x^2 as x tends to 0
        x = sp.Symbol("x", positive=True)
        assert sp.limit(xr.b88_enhancement(x) / x ** 2, x, 0) == 1
        for xv in ("1e-6", "1e-12"):
            g = mp.mpf(str(sp.N(xr.b88_enhancement(sp.Rational(xv)), 50)))
            assert abs(g / mp.mpf(xv) ** 2 - 1) < 10 * 6 * 0.0042 * float(xv) ** 2
        # LYP vanishes for a fully polarised density: with rb = 0, sbb = sab = 0 the brace reduces to -ra^2 sbb = 0
        ra, rb, saa, sab, sbb = xr.VARS
        assert sp.simplify(xr.lyp_expr().subs({sab: 0}).subs({rb: 0, sbb: 0})) == 0
        # the two arrangements of the gradient remainder are the same polynomial
        rho = ra + rb
        paper = (-sp.Rational(2, 3) * rho ** 2 * (saa + 2 * sab + sbb) + (sp.Rational(2, 3) * rho ** 2 - ra ** 2) * sbb
                 + (sp.Rational(2, 3) * rho ** 2 - rb ** 2) * saa)
        assert sp.expand(paper - (-sp.Rational(4, 3) * rho ** 2 * sab - ra ** 2 * sbb - rb ** 2 * saa)) == 0


def test_symbolic_derivatives_agree_with_differences_of_the_energy_density():
    """The compiled derivatives against central differences of the compiled energy density at 50 digits (step 1e-20
    relative: truncation 1e-40) -- a wrong ``diff`` or a wrong output order would show."""
    import mpmath as mp

    with mp.workdps(xr.DPS):
        at = [mp.mpf("0.37"), mp.mpf("0.052"), mp.mpf("0.8"), mp.mpf("-0.11"), mp.mpf("0.03")]
        for name in xr.FUNCTIONALS:
            base = xr.point(name, *at)
            for i in range(5):
                h = abs(at[i]) * mp.mpf(10) ** -20
                up, dn = list(at), list(at)
                up[i] += h
                dn[i] -= h
                fd = (xr.point(name, *up)[0] - xr.point(name, *dn)[0]) / (2 * h)
                assert abs(fd - base[1 + i]) <= mp.mpf(10) ** -25 * max(abs(fd), mp.mpf(10) ** -10), (name, i)


@pytest.mark.parametrize("longdouble", [True, False])
def test_extended_sums_with_and_without_an_80_bit_type(monkeypatch, longdouble):
    """Both routes of the contraction references (longdouble; error-free products + math.fsum) against rationals."""
    assert xr.HAVE_LONGDOUBLE == bool(np.finfo(np.longdouble).eps < 2e-19)
    if longdouble and not xr.HAVE_LONGDOUBLE:
        return  # (no 80-bit type on this host: the other case is the route in use)
    monkeypatch.setattr(xr, "HAVE_LONGDOUBLE", longdouble)
    rng = np.random.default_rng(0)
    a, b = rng.uniform(0.5, 1.5, size=(5, 7)), rng.uniform(0.5, 1.5, size=(7, 3))
    exact = np.array([[sum(xr.Fraction(float(x)) * xr.Fraction(float(y)) for x, y in zip(a[i], b[:, j]))
                       for j in range(3)] for i in range(5)], dtype=object)
    for got in (xr.matmul(a, b), np.stack([xr.rowdot(a[i][None, :].repeat(3, 0), b.T) for i in range(5)])):
        err = max(abs(xr.Fraction(float(got[i, j])) - exact[i, j]) / max(abs(exact[i, j]), xr.Fraction(1, 10 ** 30))
                  for i in range(5) for j in range(3))
        assert float(err) < 2.0 ** -52


# ------------------------------------------------------------------ the longdouble references and their bounds
def test_a_plain_float64_evaluation_meets_the_contraction_bounds():
    """The bounds of rho_reference / vmat_reference are rounding bounds of ANY float64 evaluation order: numpy's
    (BLAS) evaluation of the same sums has to meet them, at AO rows spread over eight orders of magnitude."""
    for g, nao in ((1, 1), (17, 5), (65, 33), (257, 148)):
        rng = np.random.default_rng(1000 * g + nao)
        scale = 10 ** rng.uniform(-8, 0, g)
        ao = rng.normal(size=(g, nao)) * scale[:, None]
        dao = rng.normal(size=(3, g, nao)) * scale[None, :, None]
        dm = rng.normal(size=(2, nao, nao))
        dm = 0.5 * (dm + dm.transpose(0, 2, 1))
        want_rho, want_grad, b_rho, b_grad = xr.rho_reference(ao, dao, dm)
        c = np.einsum("gm,xmn->xgn", ao, dm)
        rho = (c * ao[None]).sum(axis=2)
        grad = 2.0 * np.einsum("xgn,agn->xag", c, dao)
        assert np.all(np.abs(rho.astype(xr.LD) - want_rho) <= b_rho)
        assert np.all(np.abs(grad.astype(xr.LD) - want_grad) <= b_grad)
        wrong = rho.copy()
        wrong[0, np.argmin(scale)] *= 1.0 + 1e-8  # a relative slip at the smallest point is seen
        assert not np.all(np.abs(wrong.astype(xr.LD) - want_rho) <= b_rho)
        vr, vec = rng.normal(size=(2, g)), rng.normal(size=(2, 3, g))
        want, bound = xr.vmat_reference(ao, dao, vr, vec)
        half = 0.5 * vr[:, :, None] * ao[None] + np.einsum("xag,agn->xgn", vec, dao)
        v = np.einsum("gm,xgn->xmn", ao, half)
        assert np.all(np.abs((v + v.transpose(0, 2, 1)).astype(xr.LD) - want) <= bound)
        short = np.einsum("gm,xgn->xmn", ao[:-1], half[:, :-1]) if g > 1 else 0.0 * v  # the last grid point left out
        short = short + np.transpose(short, (0, 2, 1))
        assert not np.all(np.abs(short.astype(xr.LD) - want) <= bound)


def test_host_eval_ao_and_becke_meet_the_pointwise_references():
    from nbed_amd import integrals
    from nbed_amd import xc as xcmod

    water = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
    atoms = integrals.parse_geometry(water, "angstrom")
    bs = integrals.Basis(atoms, "6-31g*")
    assert not bs.pure_cartesian  # (d shells: the host returns the working AOs, Cartesian components x cart2ao^T)
    centres = np.array([pos for _, pos in atoms])
    rng = np.random.default_rng(9)
    pts = np.concatenate([centres, centres + np.array([6e-9, -8e-9, 0.0]), centres[:1] + [0.0, 40.0, 30.0],
                          rng.normal(scale=2.0, size=(400, 3))])
    shells = [(sh.centre, sh.exps, sh.coefs, [tuple(lmn) for lmn in sh.cart]) for sh in bs.shells]
    want, dwant, bound, dbound = xr.ao_reference(shells, pts)
    ao, dao = xcmod.eval_ao(bs, pts)
    tr, tr_abs = np.asarray(bs.cart2ao.T, dtype=xr.LD), np.abs(bs.cart2ao.T)
    extra = (bs.nao_cart + 1) * xr.U  # the transform's own dot products
    bound = bound @ tr_abs + extra * (np.abs(want).astype(np.float64) @ tr_abs)
    dbound = dbound @ tr_abs + extra * (np.abs(dwant).astype(np.float64) @ tr_abs)
    want, dwant = want @ tr, dwant @ tr
    assert np.all(np.abs(ao.astype(xr.LD) - want) <= bound) and np.all(np.abs(dao.astype(xr.LD) - dwant) <= dbound)
    assert np.isfinite(ao).all() and np.abs(want[:3]).max() > 0.1
    # Becke shares: two atoms of equal size on the bisecting plane, a nucleus, and a random cluster against float64
    two = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    inv2 = np.array([[1.0, 0.5], [0.5, 1.0]])
    plane = np.concatenate([np.zeros((50, 1)), rng.normal(size=(50, 2))], axis=1)
    assert np.all(xr.becke_reference(plane, two, np.zeros((2, 2)), inv2, 0) == 0.5)
    assert list(xr.becke_reference(two, two, np.zeros((2, 2)), inv2, 1)) == [0.0, 1.0]
    assert np.all(xr.becke_reference(plane, two[:1], np.zeros((1, 1)), np.ones((1, 1)), 0) == 1.0)
    natm = 12
    cen = rng.uniform(-4, 4, size=(natm, 3))
    aij = rng.uniform(-0.3, 0.3, size=(natm, natm))
    aij = aij - aij.T
    inv = 1.0 / (np.linalg.norm(cen[:, None] - cen[None], axis=-1) + np.eye(natm))
    p = rng.uniform(-5, 5, size=(200, 3))
    rg = np.linalg.norm(p[:, None, :] - cen[None], axis=-1)
    mu = (rg[:, :, None] - rg[:, None, :]) * inv[None]
    f = mu + aij[None] * (1.0 - mu * mu)
    for _ in range(3):
        f = 1.5 * f - 0.5 * f ** 3
    s = 0.5 * (1.0 - f)
    s[:, np.arange(natm), np.arange(natm)] = 1.0
    cell = s.prod(axis=2)
    for owner in (0, 5, 11):
        np.testing.assert_allclose(cell[:, owner] / cell.sum(axis=1),
                                   xr.becke_reference(p, cen, aij, inv, owner).astype(np.float64), rtol=1e-9, atol=1e-13)
