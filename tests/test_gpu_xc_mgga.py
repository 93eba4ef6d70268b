"""The meta-GGA chain on the MI355X: nbx_xc_functional_mgga (NBX_XC_TPSS, NBX_XC_TPSSH) against the 50-digit reference of
tests/xc_mgga_reference.py; nbx_xc_rho_tau and nbx_xc_vmat_tau exactly on integer operands, against longdouble on real
ones and bit for bit against nbx_xc_rho / nbx_xc_vmat; the whole chain on the H atom; ``nbed`` end to end.

Bounds.  Per entry of ``vr``, ``vec`` and ``vt``: the error against the 50-digit value over the sum of the magnitudes of
the seven pieces' exact contributions to that entry (the two exchange channels, the eps_PW and the H parts of
n eps_PBE (1 + C z^2) and of -(1 + C) z^2 sum n_s eps~_s, and d n z^3 eps_revPKZB^2), below 5e-11 -- in ``tails``,
``at_floor`` and ``zero_gradient_tau_unif`` below max(5e-11, 4 x the worst error of the reference's own 53-bit evaluation
of the derivatives of that kind).  E_xc: 1e-12 of sum_g w |piece|; the electron count: 1e-12.  Dropped points are exact
zeros and nothing is non-finite.

The one regime that needs more than 5e-11 is ``zero_gradient_tau_unif``, and only in ``vt``: there
alpha - 1 = (tau - tau_W - tau_unif) / tau_unif is the rounding residue of its three terms, and dE/dtau, proportional to
it through q_b, is 1e-16 of its size elsewhere with no correct digit in any float64 evaluation (the reference's own
53-bit evaluation is off by 4e1 of the pieces' magnitudes).  ``vr``, ``vec`` and E_xc hold 5e-11 and 1e-12 there.

Measured worst entries, 64 points per regime, the worse of the two names; host = the torch expression
(tests/test_host_xc_mgga.py), kernel = nbx_xc_functional_mgga on the MI355X:

  regime                    host       kernel
  existing                  4.9e-15    8.9e-15
  closed_shell              5.8e-15    1.8e-15
  polarised_beta_empty      1.7e-14    8.4e-15
  polarised_alpha_empty     1.3e-14    2.9e-15
  polarisation_1e4_1e12     4.7e-15    3.3e-15
  core                      2.5e-14    2.6e-15
  tails                     7.3e-15    1.9e-15
  zero_gradient             2.2e-15    1.2e-15
  antiparallel              3.0e-14    4.7e-15
  at_floor                  1.0e-14    1.1e-15
  z_one                     4.2e-14    4.5e-14
  z_one_plus_1e-12          3.6e-15    2.3e-15
  tau_below_tau_w           5.5e-13    6.1e-13
  z_1e-6                    1.9e-14    1.9e-14
  zero_gradient_tau_unif    1.8e-15 (vr), 2.2e1 (vt)    9.2e-16 (vr), 9.2e0 (vt)
  polarised_tau_empty       6.7e-15    5.0e-15
  all sixteen in one launch            6.1e-13
  grids of one point                   4.1e-16

E_xc: at most 5.7e-16 of sum w |piece| (kernel), 4.6e-16 (host).
"""

import numpy as np
import pytest

import xc_mgga_reference as mr
import xc_reference as xr

pytestmark = pytest.mark.gpu

FLOOR = 1e-14
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
U = xr.U
NAO = (1, 15, 16, 17, 33, 80, 81, 160, 161)  # (160 | 161: the ao fragments of xc_rho_tau leave the registers)
NPTS = (1, 63, 64, 65, 255, 257, 1000, 2049)


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


# ------------------------------------------------------------------------------------------------ nbx_xc_functional_mgga
def _kernel_functional(be, name, rho, grad, tau, w):
    from nbed_amd import _nbx

    vr, vec, vt, sums = be.xc_functional_mgga(_nbx.XC_MGGA_CODES[name], be.asarray(rho), be.asarray(grad), be.asarray(tau),
                                              be.asarray(w), FLOOR)
    sums = be.to_host(sums)
    return be.to_host(vr), be.to_host(vec), be.to_host(vt), float(sums[0]), float(sums[1])


def _all_regimes(name):
    """Every regime in one launch: 1024 points, four blocks; the bound of each point is its regime's."""
    import mpmath as mp

    ins = [mr.regime_inputs(r, FLOOR) for r in mr.REGIMES]
    refs = [mr.regime_reference(name, r, FLOOR) for r in mr.REGIMES]
    with mp.workdps(xr.DPS):
        exc, nelec, mexc = sum(r[3] for r in refs), sum(r[4] for r in refs), sum(r[6][3] for r in refs)
    cat = lambda k, ax: np.concatenate([r[k] for r in refs], axis=ax)  # noqa: E731
    mag = (np.concatenate([r[6][0] for r in refs], axis=1), np.concatenate([r[6][1] for r in refs], axis=2),
           np.concatenate([r[6][2] for r in refs], axis=1), mexc)
    ref = (cat(0, 1), cat(1, 2), cat(2, 1), exc, nelec, np.concatenate([r[5] for r in refs]), mag, None)
    bounds = [mr.entry_bound(reg, r) for reg, r in zip(mr.REGIMES, refs)]
    bound = tuple(np.concatenate([np.full(r[5].shape, b[k]) for b, r in zip(bounds, refs)]) for k in range(3))
    return tuple(np.concatenate([i[k] for i in ins], axis=-1) for k in range(4)), ref, bound


@pytest.mark.parametrize("regime", mr.REGIMES + ("all",))
@pytest.mark.parametrize("name", mr.NAMES)
def test_functional_kernel_against_the_50_digit_reference(be, name, regime):
    from nbed_amd import xc

    assert xc.XCProvider.RHO_FLOOR == FLOOR
    if regime == "all":
        (rho, grad, tau, w), ref, bound = _all_regimes(name)
        assert rho.shape[1] == 1024
    else:
        rho, grad, tau, w = mr.regime_inputs(regime, FLOOR)
        ref = mr.regime_reference(name, regime, FLOOR)
        bound = mr.entry_bound(regime, ref)
        assert rho.shape[1] == 64
    mr.check_functional(f"kernel {name} {regime}", _kernel_functional(be, name, rho, grad, tau, w), ref, bound)


@pytest.mark.parametrize("regime,index", [("z_one", 0), ("z_one", 63), ("tau_below_tau_w", 0), ("tau_below_tau_w", 1),
                                          ("at_floor", 0), ("at_floor", 1)])
@pytest.mark.parametrize("name", mr.NAMES)
def test_functional_kernel_on_a_grid_of_one_point(be, name, regime, index):
    """The z = 1 point (one electron; closed shell), the clamped point (tau = 0; 0 < tau < tau_W), on and one ulp above
    the floor."""
    rho, grad, tau, w = mr.regime_inputs(regime, FLOOR)
    rho, grad, tau, w = rho[:, index:index + 1], grad[:, :, index:index + 1], tau[:, index:index + 1], w[index:index + 1]
    ref = mr.functional_reference(name, rho, grad, tau, w, FLOOR, own_error=regime in mr.LOOSE_REGIMES)
    if regime == "at_floor":
        assert bool(ref[5][0]) == bool(index)  # exactly on the floor: dropped; one ulp above: kept
    if regime == "tau_below_tau_w":
        assert (tau[0, 0] == 0.0) == (index == 0)
    mr.check_functional(f"kernel {name} {regime}[{index}]", _kernel_functional(be, name, rho, grad, tau, w), ref,
                        mr.entry_bound(regime, ref))


def test_codes_are_refused_where_they_do_not_belong(be):
    from nbed_amd import _nbx

    rho, grad, tau, w = (be.asarray(x) for x in mr.regime_inputs("existing", FLOOR))
    for code in (32, 33):
        with pytest.raises(_nbx.NbxError):
            be.xc_functional(code, rho, grad, w, FLOOR)
        with pytest.raises(_nbx.NbxError):
            be.xc_functional_rs(code, 0.33, rho, grad, w, FLOOR)
    for code in tuple(range(9)) + (16, 17, 34, -1):
        with pytest.raises(_nbx.NbxError):
            be.xc_functional_mgga(code, rho, grad, tau, w, FLOOR)


# ------------------------------------------------------------------------------------------------ nbx_xc_rho_tau / _vmat_tau
def _integer_case(nao, npts, seed):
    rng = np.random.default_rng(seed)
    ao = rng.integers(-3, 4, (npts, nao)).astype(np.float64)
    dao = rng.integers(-3, 4, (3, npts, nao)).astype(np.float64)
    dm = rng.integers(-2, 3, (2, nao, nao))
    dm = (dm + dm.transpose(0, 2, 1)).astype(np.float64)
    vr = 2.0 * rng.integers(-3, 4, (2, npts))
    vec = rng.integers(-3, 4, (2, 3, npts)).astype(np.float64)
    vt = 4.0 * rng.integers(-3, 4, (2, npts))
    return ao, dao, dm, vr, vec, vt


def _vmat_tau_exact(ao, dao, vr, vec, vt, dtype):
    out, mag = [], []
    a, d = ao.astype(dtype), dao.astype(dtype)
    for x in range(2):
        half = 0.5 * vr[x].astype(dtype)[:, None] * a + sum(vec[x, k].astype(dtype)[:, None] * d[k] for k in range(3))
        habs = 0.5 * np.abs(vr[x])[:, None] * np.abs(ao) + sum(np.abs(vec[x, k])[:, None] * np.abs(dao[k]) for k in range(3))
        v = a.T @ half + sum(d[k].T @ (0.25 * vt[x].astype(dtype)[:, None] * d[k]) for k in range(3))
        m = np.abs(ao).T @ habs + sum(np.abs(dao[k]).T @ (0.25 * np.abs(vt[x])[:, None] * np.abs(dao[k])) for k in range(3))
        out.append(v + v.T)
        mag.append(m + m.T)
    return np.stack(out), np.stack(mag)


@pytest.mark.parametrize("nao", NAO)
def test_rho_tau_and_vmat_tau_are_exact_on_integer_operands(be, nao):
    """Integer-valued ao, dao, D, vr (even), vec and vt (multiples of four): every product and sum is exact in float64, so
    the kernels must return the integers -- and rho, grad of xc_rho_tau are xc_rho's bits, xc_vmat_tau with vt = 0 is
    xc_vmat's."""
    for npts in NPTS:
        ao, dao, dm, vr, vec, vt = _integer_case(nao, npts, 100 * nao + npts)
        aod, daod, dmd = be.asarray(ao), be.asarray(dao), be.asarray(dm)
        rho, grad, tau = (be.to_host(x) for x in be.xc_rho_tau(aod, daod, dmd))
        rho0, grad0 = (be.to_host(x) for x in be.xc_rho(aod, daod, dmd))
        assert rho.tobytes() == rho0.tobytes() and grad.tobytes() == grad0.tobytes(), (nao, npts)
        c = np.einsum("gm,xmn->xgn", ao, dm)
        np.testing.assert_array_equal(rho, np.einsum("xgn,gn->xg", c, ao))
        np.testing.assert_array_equal(grad, 2.0 * np.einsum("xgn,agn->xag", c, dao))
        np.testing.assert_array_equal(tau, 0.5 * np.einsum("agm,xmn,agn->xg", dao, dm, dao))
        vrd, vecd = be.asarray(vr), be.asarray(vec)
        v = be.to_host(be.xc_vmat_tau(aod, daod, vrd, vecd, be.asarray(vt)))
        want, _ = _vmat_tau_exact(ao, dao, vr, vec, vt, np.float64)
        np.testing.assert_array_equal(v, want)
        v0 = be.to_host(be.xc_vmat_tau(aod, daod, vrd, vecd, be.asarray(np.zeros_like(vt))))
        assert v0.tobytes() == be.to_host(be.xc_vmat(aod, daod, vrd, vecd)).tobytes(), (nao, npts)


@pytest.mark.parametrize("nao,npts", [(17, 65), (81, 1000), (160, 257), (161, 2049)])
def test_rho_tau_and_vmat_tau_on_real_operands(be, nao, npts):
    """Real operands against longdouble.  tau: two nested sums of nao terms, three components: (L + 4) eps sum |terms| with
    L = 2 nao + 3 (tests/scf_kernel_cases.py; eps = 2^-52).  v: four products over npts grid points, L = 4 npts + 8 for the
    terms of the operands, the chunk sums and the symmetrisation."""
    rng = np.random.default_rng(7 * nao + npts)
    ao, dao = rng.normal(size=(npts, nao)), rng.normal(size=(3, npts, nao))
    dm = rng.normal(size=(2, nao, nao))
    dm = 0.5 * (dm + dm.transpose(0, 2, 1))
    vr, vec, vt = rng.normal(size=(2, npts)), rng.normal(size=(2, 3, npts)), rng.normal(size=(2, npts))
    aod, daod, dmd = be.asarray(ao), be.asarray(dao), be.asarray(dm)
    rho, grad, tau = (be.to_host(x) for x in be.xc_rho_tau(aod, daod, dmd))
    rho0, grad0 = (be.to_host(x) for x in be.xc_rho(aod, daod, dmd))
    assert rho.tobytes() == rho0.tobytes() and grad.tobytes() == grad0.tobytes()
    eps = 2.0 * U
    want = np.stack([0.5 * sum(xr.rowdot(xr.matmul(dao[a], dm[x]), dao[a]) for a in range(3)) for x in range(2)])
    terms = np.stack([0.5 * sum(((np.abs(dao[a]) @ np.abs(dm[x])) * np.abs(dao[a])).sum(axis=1) for a in range(3))
                      for x in range(2)])
    ratio = (np.abs(tau - want) / ((2 * nao + 7) * eps * terms)).max()
    print(f"XCTAU nao {nao} npts {npts} tau err / bound {float(ratio):.2e}")
    assert ratio < 1.0
    v = be.to_host(be.xc_vmat_tau(aod, daod, be.asarray(vr), be.asarray(vec), be.asarray(vt)))
    vwant, vmag = _vmat_tau_exact(ao, dao, vr, vec, vt, xr.LD)
    vratio = (np.abs(v - vwant) / ((4 * npts + 12) * eps * vmag)).max()
    print(f"XCTAU nao {nao} npts {npts} vmat err / bound {float(vratio):.2e}")
    assert vratio < 1.0
    v0 = be.to_host(be.xc_vmat_tau(aod, daod, be.asarray(vr), be.asarray(vec), be.asarray(np.zeros_like(vt))))
    assert v0.tobytes() == be.to_host(be.xc_vmat(aod, daod, be.asarray(vr), be.asarray(vec))).tobytes()


def test_rho_tau_refuses_what_rho_refuses(be):
    from nbed_amd import _nbx

    ao, dao, dm = be.asarray(np.zeros((4, 641))), be.asarray(np.zeros((3, 4, 641))), be.asarray(np.zeros((2, 641, 641)))
    for fn in (be.xc_rho, be.xc_rho_tau):
        with pytest.raises(_nbx.NbxError, match="640"):
            fn(ao, dao, dm)
    ok = be.xc_rho_tau(be.asarray(np.zeros((4, 640))), be.asarray(np.zeros((3, 4, 640))), be.asarray(np.zeros((2, 640, 640))))
    assert not be.to_host(ok[2]).any()


# ------------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("name", mr.NAMES)
def test_h_atom_open_shell_chain(be, name):
    """tests/test_gpu_xc_gga.py::test_h_atom_open_shell_chain for the meta-GGAs, same construction and bounds: H / 6-31G,
    one alpha electron, no beta electron, 1728 points: XCProvider on the device against XCProvider on the host.  E_xc:
    1e-12 relative; v_xc: 1e-10 of the largest entry of each spin.  One orbital: tau = tau_W at every point up to
    rounding, which is what the margin of the clamp is for (without it the two potentials differed by 1.5e-3)."""
    from nbed_amd import integrals, xc

    atoms = integrals.parse_geometry("1\n\nH 0.0 0.0 0.0", "angstrom")
    bs = integrals.Basis(atoms, "6-31g")
    s = integrals.molecule_integrals("1\n\nH 0.0 0.0 0.0", "6-31g")["S"]
    c = np.array([0.45, 0.65])
    c = c / np.sqrt(c @ s @ c)
    dm = np.stack([np.outer(c, c), np.zeros((2, 2))])
    dev = xc.XCProvider(atoms, bs, name, n_rad=32, n_theta=6, device=be.device)
    host = xc.XCProvider(atoms, bs, name, n_rad=32, n_theta=6, device="cpu")
    np.testing.assert_array_equal(dev.points, host.points)
    npts = dev.points.shape[0]
    assert 1000 < npts < 2500 and dev._ao is not None and host._ao is None
    e_dev, v_dev = dev(dm)
    e_host, v_host = host(dm)
    e_rel = abs(e_dev - e_host) / abs(e_host)
    dv = [np.abs(v_dev[x] - v_host[x]).max() / np.abs(v_host[x]).max() for x in range(2)]
    print(f"XCCHAIN {name} npts {npts} E_xc {e_dev:.12f} rel host {e_rel:.2e} v rel host {dv[0]:.2e} {dv[1]:.2e}")
    assert abs(dev.nelec_last - 1.0) < 1e-4 and abs(dev.nelec_last - host.nelec_last) < 1e-11
    assert e_rel < 1e-12 and max(dv) < 1e-10
    assert np.abs(v_host[1]).max() > 1e-3  # the empty spin's potential is not small


def _water(be, name, engine):
    from nbed_amd import NbedConfig, nbed
    from nbed_amd.driver import BuiltinHFProvider

    cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional=name, projector="huzinaga",
                     localization="spade", convergence=1e-8, mu_level_shift=1e6, max_hf_cycles=100, max_dft_cycles=100,
                     run_fci_emb=False, run_ccsd_emb=False, run_dft_in_dft=True)
    drv = nbed(cfg, provider=BuiltinHFProvider(be, eri_engine=engine), backend=be)
    ks, res = drv._global_ks, drv.huzinaga
    assert ks.converged and res["scf"].converged
    assert ks.xc_provider._ao is not None  # the quadrature ran on the device
    print(f"XCE2E {name} {engine} e_ks {ks.e_tot:.10f} dft_in_dft - ks {res['e_dft_in_dft'] - ks.e_tot:.2e} "
          f"sum rule {drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot:.2e}")
    assert abs(drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot) < 1e-8
    assert abs(res["e_dft_in_dft"] - ks.e_tot) < 1e-9
    return ks.e_tot


@pytest.mark.parametrize("name", mr.NAMES)
def test_driver_dft_in_dft_water(be, name):
    """``nbed`` with a meta-GGA (global Kohn-Sham, embedding potential, DFT-in-DFT) on libnbx: the converged global energy
    is the host-form provider's on the same grid (2e-8, the bound of
    tests/test_gpu_xc_gga.py::test_driver_pbe_dft_in_dft_water), the subsystem energies add up (1e-8) and Huzinaga
    DFT-in-DFT reproduces the global energy (1e-9).  The energies themselves are unverified against another program."""
    from test_host_xc_mgga import HOST_ENERGY

    assert abs(_water(be, name, None) - HOST_ENERGY[name]) < 2e-8


def test_driver_on_the_cholesky_factor(be):
    """``tpssh`` with eri_engine='cholesky': nothing of the meta-GGA path needs the dense tensor.  The factor reproduces
    every (pq|rs) within 1e-8, so the energy moves by at most 1e-8 (sum |D_pq|)^2 < 1e-8 (7 sqrt(10))^2 = 5e-6 to first
    order: 1e-5."""
    from test_host_xc_mgga import HOST_ENERGY

    assert abs(_water(be, "tpssh", "cholesky") - HOST_ENERGY["tpssh"]) < 1e-5
