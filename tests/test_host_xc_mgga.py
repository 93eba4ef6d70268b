"""The meta-GGAs ``tpss`` and ``tpssh`` on the host: ``nbed_amd.xc.energy_density_mgga`` against the 50-digit reference of
tests/xc_mgga_reference.py (whose derivatives are differences of the 50-digit energy), known answers that need no other
program, the tables and look-ups, the C ABI, the provider's potential as the derivative of its energy (tau term
included), and ``nbed`` on the host checker backend.  No GPU.

Known answers:
  * TPSS exchange is exact for the hydrogen atom: n = exp(-2r) / pi, fully polarised, E_x = -5/16 (bound 1e-6);
  * TPSS correlation vanishes for every one-electron density (that one and a Gaussian): below 1e-14 of int n |eps_PBE|.
    The empty channel is set to 1e-30, not to the provider's clamp RHO_FLOOR / 2: the clamp leaves a true residue
    (1 + C) n_b (eps_PBE - eps~_b) of 1e-12 of that integral, which is the convention's and not an error;
  * without a gradient and with tau = tau_unif the energy is that of ``lda,pw_mod``;
  * z -> 0 (tau = 1e12 tau_W): the correlation is PBE's.

Measured worst entry per regime (64 points, the worse of the two names), error over the summed magnitudes of the seven
pieces: the table of tests/test_gpu_xc_mgga.py holds these figures beside the kernel's.
"""

import math
import re
from pathlib import Path

import numpy as np
import pytest

import xc_mgga_reference as mr

FLOOR = 1e-14
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
REPO = Path(__file__).resolve().parent.parent


def host_functional(name, rho, grad, tau, w, floor):
    """nbx_xc_functional_mgga's outputs from the torch expression, with XCProvider.__call__'s conventions."""
    import torch as t

    from nbed_amd import xc

    rho, grad, tau, w = (t.as_tensor(np.asarray(x, dtype=np.float64)) for x in (rho, grad, tau, w))
    ga, gb = grad[0], grad[1]
    keep = ((rho[0] + rho[1]) > floor).to(t.float64)
    ra = t.clamp(rho[0], min=floor * 0.5).requires_grad_(True)
    rb = t.clamp(rho[1], min=floor * 0.5).requires_grad_(True)
    saa = ((ga * ga).sum(dim=0) + 1e-40).requires_grad_(True)
    sab = (ga * gb).sum(dim=0).requires_grad_(True)
    sbb = ((gb * gb).sum(dim=0) + 1e-40).requires_grad_(True)
    ta, tb = tau[0].clone().requires_grad_(True), tau[1].clone().requires_grad_(True)
    exc = (w * keep * xc.energy_density_mgga(name, ra, rb, saa, sab, sbb, ta, tb)).sum()
    vra, vrb, vaa, vab, vbb, vta, vtb = (g if g is not None else t.zeros_like(w) for g in t.autograd.grad(
        exc, (ra, rb, saa, sab, sbb, ta, tb), allow_unused=True))
    vec = t.stack([2.0 * vaa * ga + vab * gb, 2.0 * vbb * gb + vab * ga])
    return (t.stack([vra, vrb]).numpy(), vec.numpy(), t.stack([vta, vtb]).numpy(), float(exc.detach()),
            float((w * (rho[0] + rho[1])).sum()))


@pytest.mark.parametrize("regime", mr.REGIMES)
@pytest.mark.parametrize("name", mr.NAMES)
def test_host_energy_density_against_the_50_digit_reference(name, regime):
    """Energy and all seven first derivatives (autograd) against the differences of the 50-digit energy: 5e-11 of the
    summed magnitudes of the pieces per entry, 1e-12 on E_xc."""
    rho, grad, tau, w = mr.regime_inputs(regime, FLOOR)
    ref = mr.regime_reference(name, regime, FLOOR)
    assert rho.shape[1] == 64
    mr.check_functional(f"host {name} {regime}", host_functional(name, rho, grad, tau, w, FLOOR), ref,
                        mr.entry_bound(regime, ref))


def test_the_new_regimes_are_what_they_say():
    """z = 1 to the bit and unclamped; the clamp acts in ``tau_below_tau_w``; z = 1e-6; alpha = 1 without a gradient."""
    for regime, want in (("z_one", (True, True, True)), ("tau_below_tau_w", (False, False, None)), ("z_1e-6", (True, True, True))):
        rho, grad, tau, _ = mr.regime_inputs(regime, FLOOR)
        r = np.maximum(rho, FLOOR / 2)
        s = (grad * grad).sum(axis=1) + 1e-40
        for g in range(rho.shape[1]):
            if regime == "z_one" and rho[1, g] == 0.0:
                assert tau[0, g] == s[0, g] / (8.0 * r[0, g]) and tau[1, g] == 0.0
                continue
            if regime == "tau_below_tau_w" and g % 8 == 2:
                want_g = (True, True, None)  # inside the margin of the clamp
            else:
                want_g = want
            flags = mr.clamp_flags(r[0, g], r[1, g], s[0, g], (grad[0, :, g] * grad[1, :, g]).sum(), s[1, g], tau[0, g], tau[1, g])
            assert all(f == w_ for f, w_ in zip(flags, want_g) if w_ is not None), (regime, g, flags)
            if regime == "z_one":
                assert tau[0, g] == s[0, g] / (8.0 * r[0, g])


def _radial(n=400, rmax=20.0):
    x, w = np.polynomial.legendre.leggauss(n)
    r = 0.5 * rmax * (x + 1.0)
    return r, 0.5 * rmax * w * 4.0 * math.pi * r * r


def _one_electron(kind):
    """(weights, n, |grad n|^2) of a normalised one-electron density on a radial Gauss-Legendre rule."""
    r, w = _radial()
    if kind == "hydrogen":
        n = np.exp(-2.0 * r) / math.pi
        dn = -2.0 * n
    else:  # Gaussian exp(-a r^2) (a / pi)^(3/2), a = 0.7
        a = 0.7
        n = np.exp(-a * r * r) * (a / math.pi) ** 1.5
        dn = -2.0 * a * r * n
    return w, n, dn * dn


def test_tpss_exchange_is_exact_for_the_hydrogen_atom():
    import torch as t

    from nbed_amd import xc

    w, n, s = _one_electron("hydrogen")
    assert abs((w * n).sum() - 1.0) < 1e-12
    ra, saa = t.as_tensor(n), t.as_tensor(s) + 1e-40
    ta = saa / (8.0 * ra)  # tau = tau_W: one orbital
    rb, sbb, tb = t.full_like(ra, 1e-30), t.full_like(ra, 1e-40), t.zeros_like(ra)
    e_x = float((t.as_tensor(w) * xc._tpss_x(t, ra, rb, saa, sbb, ta, tb)).sum())
    print(f"TPSS E_x[H] = {e_x:.10f} (exact -0.3125): {e_x + 0.3125:.2e}")
    assert abs(e_x + 0.3125) <= 1e-6
    # the whole functional: E_xc = E_x, because E_c = 0
    e_xc = float((t.as_tensor(w) * xc.energy_density_mgga("tpss", ra, rb, saa, t.zeros_like(ra), sbb, ta, tb)).sum())
    assert abs(e_xc - e_x) < 1e-14


@pytest.mark.parametrize("kind", ["hydrogen", "gaussian"])
def test_tpss_correlation_vanishes_for_one_electron(kind):
    import torch as t

    from nbed_amd import xc

    w, n, s = _one_electron(kind)
    sel = n > 1e-14
    w, n, s = w[sel], n[sel], s[sel]
    ra, saa = t.as_tensor(n), t.as_tensor(s) + 1e-40
    ta = saa / (8.0 * ra)
    rb, sbb, sab, tb = t.full_like(ra, 1e-30), t.full_like(ra, 1e-40), t.zeros_like(ra), t.zeros_like(ra)
    e_c = float((t.as_tensor(w) * xc._tpss_c(t, ra, rb, saa, sab, sbb, ta, tb)).sum())
    scale = float((t.as_tensor(w) * xc._pbe_c(t, ra, rb, saa, sab, sbb).abs()).sum())
    print(f"TPSS E_c[{kind}] = {e_c:.2e} of int n |eps_PBE| = {scale:.6f}: {abs(e_c) / scale:.2e}")
    assert scale > 1e-3 and abs(e_c) < 1e-14 * scale


def test_uniform_gas_limit_is_lda_pw_mod():
    """No gradient and tau = tau_unif: p = z = 0, alpha = 1, q_b = 0, x = 0, F_x = 1; C z^2 = 0: Slater + PW92."""
    import torch as t

    from nbed_amd import xc

    rng = np.random.default_rng(11)
    ra = t.as_tensor(10 ** rng.uniform(-6, 2, 200))
    rb = ra * t.as_tensor(10 ** rng.uniform(-2, 2, 200))
    cf = 0.3 * (6.0 * math.pi ** 2) ** (2.0 / 3.0)
    tiny, zero = t.full_like(ra, 1e-40), t.zeros_like(ra)
    got = xc.energy_density_mgga("tpss", ra, rb, tiny, zero, tiny, cf * ra ** (5.0 / 3.0), cf * rb ** (5.0 / 3.0))
    want = xc.energy_density("lda,pw_mod", ra, rb, tiny, zero, tiny)
    rel = float(((got - want).abs() / want.abs()).max())
    print(f"uniform-gas limit: {rel:.2e}")
    assert rel < 1e-14


def test_z_to_zero_correlation_is_pbe():
    import torch as t

    from nbed_amd import xc

    rho, grad, _, _ = mr.regime_inputs("existing", FLOOR)
    ra, rb = t.as_tensor(rho[0]), t.as_tensor(rho[1])
    ga, gb = t.as_tensor(grad[0]), t.as_tensor(grad[1])
    saa, sab, sbb = (ga * ga).sum(0) + 1e-40, (ga * gb).sum(0), (gb * gb).sum(0) + 1e-40
    tw = (saa + 2 * sab + sbb) / (8.0 * (ra + rb))
    got = xc._tpss_c(t, ra, rb, saa, sab, sbb, 0.5e12 * tw, 0.5e12 * tw)  # z = 1e-12: the corrections are O(z^2)
    want = xc._pbe_c(t, ra, rb, saa, sab, sbb)
    rel = float(((got - want).abs() / want.abs()).max())
    print(f"z -> 0: {rel:.2e}")
    assert rel < 1e-14


def test_tables_and_look_ups():
    from nbed_amd import _nbx, xc

    assert xc.MGGA_PARAMETERS == {"tpss": 0.0, "tpssh": 0.1}
    assert xc.hybrid_fraction("tpss") == 0.0 and xc.hybrid_fraction("TPSSh") == 0.1
    assert xc.rsh_parameters("tpssh") == (0.0, 0.1, 0.0) and xc.rsh_parameters("tpss") == (0.0, 0.0, 0.0)
    assert not set(xc.MGGA_PARAMETERS) & (set(xc.HYBRID_FRACTION) | set(xc.RSH_PARAMETERS))
    assert _nbx.XC_MGGA_CODES == {"tpss": 32, "tpssh": 33}
    assert not set(_nbx.XC_MGGA_CODES) & (set(_nbx.XC_CODES) | set(_nbx.XC_RS_CODES))
    with pytest.raises(ValueError, match="tpssh"):
        xc.hybrid_fraction("scan")
    one = __import__("torch").ones(1, dtype=__import__("torch").float64)
    for name in ("tpss", "tpssh"):
        with pytest.raises(ValueError, match="meta-GGA"):
            xc.energy_density(name, one, one, one, one, one)
    with pytest.raises(ValueError, match="meta-GGA"):
        xc.energy_density_mgga("pbe", one, one, one, one, one, one, one)
    x = xc._tpss_x(__import__("torch"), one, one, one, one, one, one)
    c = xc._tpss_c(__import__("torch"), one, one, one, one, one, one, one)
    assert float(xc.energy_density_mgga("tpssh", one, one, one, one, one, one, one)) == pytest.approx(float(0.9 * x + c), rel=1e-15)


def test_the_new_entry_points_are_in_the_header_and_the_ctypes_table():
    from nbed_amd import _nbx

    header = (REPO / "include" / "nbx.h").read_text()
    for fn in ("nbx_xc_rho_tau", "nbx_xc_functional_mgga", "nbx_xc_vmat_tau", "nbx_xc_vmat_tau_worksize"):
        assert re.search(rf"^(?:int|size_t)\s+{fn}\s*\(", header, flags=re.M) and fn in _nbx.SIGNATURES, fn
        idx = header.index(f" {fn}(")
        assert "nbed/" in header[max(0, idx - 4000):idx], fn  # the block comment cites the reference lines
    assert "#define NBX_XC_TPSS 32" in header and "#define NBX_XC_TPSSH 33" in header
    assert _nbx.NBX_VERSION == 3
    assert len(_nbx.SIGNATURES["nbx_xc_functional_mgga"][1]) == 14
    if _nbx.LIB_PATH.exists():
        lib = _nbx.load_library()
        assert lib.nbx_xc_vmat_tau_worksize(1000, 33) == lib.nbx_xc_vmat_worksize(1000, 33)


@pytest.mark.parametrize("name", mr.NAMES)
def test_potential_is_the_derivative_of_the_energy(name):
    """v_xc, its 1/2 int v_tau grad phi . grad phi term included, is the derivative of E_xc: central difference along a
    random symmetric direction on water / STO-3G with an open-shell density (the grid, step and bound of
    tests/test_host_xc_gga.py::test_pbe_potential_is_the_derivative_of_the_energy)."""
    from nbed_amd import integrals, xc

    atoms = integrals.parse_geometry(WATER)
    basis = integrals.Basis(atoms, "sto-3g")
    ints = integrals.molecule_integrals(WATER, "sto-3g", "angstrom")
    prov = xc.XCProvider(atoms, basis, name, n_rad=60, n_theta=18, device="cpu")
    w, c = np.linalg.eigh(ints["S"])
    x = (c / np.sqrt(w)) @ c.T
    _, u = np.linalg.eigh(x @ ints["hcore"] @ x)
    cmo = x @ u
    dm = np.stack([cmo[:, :5] @ cmo[:, :5].T, cmo[:, :4] @ cmo[:, :4].T])  # open shell on purpose
    exc, vxc = prov(dm)
    assert abs(prov.nelec_last - 9.0) < 1e-5 and exc < -8.0
    np.testing.assert_allclose(vxc, vxc.transpose(0, 2, 1), rtol=0, atol=1e-12)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(2, 7, 7)) * 1e-5
    d = d + d.transpose(0, 2, 1)
    fd = (prov(dm + d)[0] - prov(dm - d)[0]) / 2.0
    got = np.einsum("xij,xji->", vxc, d)
    print(f"{name}: central difference {fd:.12e}, tr(v d) {got:.12e}, difference {fd - got:.2e}")
    assert abs(fd - got) < 2e-9


@pytest.fixture(scope="module")
def runs():
    from oracle_backend import OracleBackend

    from nbed_amd import NbedConfig, nbed
    from nbed_amd.driver import BuiltinHFProvider

    be = OracleBackend()
    out = {}
    for name in mr.NAMES:
        cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional=name, projector="both",
                         localization="spade", convergence=1e-8, mu_level_shift=1e6, max_hf_cycles=100, max_dft_cycles=100,
                         run_fci_emb=False, run_ccsd_emb=False, run_dft_in_dft=True)
        assert BuiltinHFProvider.supports(cfg)
        out[name] = nbed(cfg, provider=BuiltinHFProvider(be), backend=be)
    return out


@pytest.mark.parametrize("name", mr.NAMES)
def test_driver_both_projectors_and_dft_in_dft(name, runs):
    """``nbed`` on water / STO-3G on the host checker backend: the embedding potential
    and DFT-in-DFT go through with tau of each subsystem density -- DFT-in-DFT reproduces the global Kohn-Sham energy
    (Huzinaga 1e-9, level shift 5e-6) and the subsystem energies add up to it (1e-8), the figures of
    tests/test_host_rsh.py.  The converged energies are unverified against another program."""
    from nbed_amd.driver import BuiltinHFProvider

    drv = runs[name]
    ks = drv._global_ks
    assert isinstance(drv.provider, BuiltinHFProvider) and ks.converged and ks.xc_provider.xc == name
    assert ks.hyb == (0.1 if name == "tpssh" else 0.0)
    assert drv.mu["scf"].converged and drv.huzinaga["scf"].converged
    print(f"MGGA {name} e_ks {ks.e_tot:.10f} mu - huz {drv.mu['e_rhf'] - drv.huzinaga['e_rhf']:.2e} dft_in_dft - ks "
          f"mu {drv.mu['e_dft_in_dft'] - ks.e_tot:.2e} huz {drv.huzinaga['e_dft_in_dft'] - ks.e_tot:.2e} sum rule "
          f"{drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot:.2e}")
    assert abs(drv.mu["e_rhf"] - drv.huzinaga["e_rhf"]) < 1e-5
    assert abs(drv.huzinaga["e_dft_in_dft"] - ks.e_tot) < 1e-9
    assert abs(drv.mu["e_dft_in_dft"] - ks.e_tot) < 5e-6
    assert abs(drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot) < 1e-8
    assert -75.4 < ks.e_tot < -75.1  # every DFT energy of this molecule here lies in this window
    assert abs(ks.e_tot - HOST_ENERGY[name]) < 2e-8


#: converged global Kohn-Sham energies of water / STO-3G on the default grid from the host form (unverified against
#: another program); tests/test_gpu_xc_mgga.py holds the device quadrature to the same numbers
HOST_ENERGY = {"tpss": -75.3229339519, "tpssh": -75.3211315861}


def test_tpssh_is_not_tpss(runs):
    assert abs(runs["tpss"]._global_ks.e_tot - runs["tpssh"]._global_ks.e_tot) > 1e-3


def test_what_is_still_refused():
    from oracle_backend import OracleBackend

    from nbed_amd import NbedConfig
    from nbed_amd.driver import BuiltinHFProvider
    from nbed_amd.exceptions import NbedDriverError

    for bad in ("scan", "revtpss", "m06-l"):
        cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional=bad)
        with pytest.raises(NbedDriverError, match="covers xc_functional.*tpss"):
            BuiltinHFProvider(OracleBackend()).global_ks(cfg)
