"""nbx_xc_functional for NBX_XC_LDA_PW_MOD, _PBE, _PBEH, _BLYP and _B3LYP5 on the MI355X against the 50-digit
references of tests/xc_gga_reference.py; the whole chain (eval_ao, xc_rho, xc_functional, xc_vmat) on the H atom with
``pbe`` and ``b3lyp5``; and ``nbed`` end to end with ``pbe``.

Bounds.  Per entry of ``vr`` and ``vec``: the error against the 50-digit value, divided by the sum of the magnitudes
of the pieces' exact contributions to that entry (each exchange channel, the eps part and the H part of PBE
correlation, B88 per channel, LYP, VWN; at least 1e-150, a condition), below 5e-11 -- in the regimes ``tails`` and
``at_floor`` below max(5e-11, 4 x the error of the reference's own 53-bit evaluation with expm1 / log1p).  E_xc: 1e-12
of sum_g w |piece|; the electron count: 1e-12.  Dropped points are exact zeros and nothing is non-finite.

Measured on the MI355X, 64 points per regime, worst entry over the five codes (the code it belongs to), beside the
host expression's worst entry and the error of the reference's own 53-bit evaluation (the yardstick of the rule):

  regime                    kernel             host               reference at 53 bits   bound
  existing                  5.8e-15 (b3lyp5)   9.8e-15 (pbeh)     1.4e-14                5e-11
  closed_shell              7.8e-16 (blyp)     1.5e-14 (b3lyp5)   2.2e-14                5e-11
  polarised_beta_empty      2.7e-12 (pbe)      2.0e-12 (pbe)      2.2e-11                5e-11
  polarised_alpha_empty     4.7e-13 (pbe)      5.3e-13 (pbe)      1.9e-11                5e-11
  polarisation_1e4_1e12     9.5e-14 (pbe)      9.4e-14 (pbe)      3.2e-13                5e-11
  core                      4.5e-15 (b3lyp5)   3.5e-14 (pbe)      5.1e-15                5e-11
  tails                     4.2e-14 (b3lyp5)   3.2e-14 (pbe)      8.9e-14                max(5e-11, 3.6e-13) = 5e-11
  zero_gradient             2.3e-15 (b3lyp5)   2.2e-15 (pbeh)     4.7e-15                5e-11
  antiparallel              4.1e-15 (b3lyp5)   4.2e-13 (pbeh)     1.5e-13                5e-11
  at_floor                  4.7e-14 (b3lyp5)   4.5e-14 (b3lyp5)   1.5e-13                max(5e-11, 6.0e-13) = 5e-11
  all ten in one launch     2.7e-12
  grids of one point        1.7e-14

E_xc: at most 5.4e-15 of sum w |piece| (kernel), 3.9e-15 (host).  No regime needs more than 5e-11: with expm1 / log1p
the two regimes in which the textbook evaluation lost digits (8.6e-11 in ``tails``, 1.3e-10 in ``at_floor``, through
exp(.) - 1) sit at 5e-14.  The largest figure, 2.7e-12, is dE/drho of the EMPTY channel of a fully polarised density
under PBE correlation: there d eps / d zeta and dH / d zeta, each carrying (1 - zeta)^(-1/3) = 1e4 .. 1e5, nearly cancel.

Reference cost: 64 points per regime x 10 regimes, eleven pieces shared by the five names, at 50 digits and at 53
bits (25 s); 1728 points for the H atom.
"""

import numpy as np
import pytest

import xc_gga_reference as gr
import xc_reference as xr

pytestmark = pytest.mark.gpu

FLOOR = 1e-14
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


# ------------------------------------------------------------------------------------------------ nbx_xc_functional
def _kernel_functional(be, name, rho, grad, w):
    from nbed_amd import _nbx

    vr, vec, sums = be.xc_functional(_nbx.XC_CODES[name], be.asarray(rho), be.asarray(grad), be.asarray(w), FLOOR)
    sums = be.to_host(sums)
    return be.to_host(vr), be.to_host(vec), float(sums[0]), float(sums[1])


def _all_regimes(name):
    """Every regime in one launch: 640 points, two and a half blocks; the bound of each point is its regime's."""
    import mpmath as mp

    ins = [gr.regime_inputs(r, FLOOR) for r in xr.REGIMES]
    refs = [gr.regime_reference(name, r, FLOOR) for r in xr.REGIMES]
    with mp.workdps(xr.DPS):
        exc, nelec, mexc = sum(r[2] for r in refs), sum(r[3] for r in refs), sum(r[5][2] for r in refs)
    ref = (np.concatenate([r[0] for r in refs], axis=1), np.concatenate([r[1] for r in refs], axis=2), exc, nelec,
           np.concatenate([r[4] for r in refs]),
           (np.concatenate([r[5][0] for r in refs], axis=1), np.concatenate([r[5][1] for r in refs], axis=2), mexc), None)
    bound = np.concatenate([np.full(r[4].shape, gr.entry_bound(reg, r)) for reg, r in zip(xr.REGIMES, refs)])
    return tuple(np.concatenate([i[k] for i in ins], axis=-1) for k in range(3)), ref, bound


@pytest.mark.parametrize("regime", xr.REGIMES + ("all",))
@pytest.mark.parametrize("name", gr.FUNCTIONALS)
def test_functional_kernel_against_the_50_digit_reference(be, name, regime):
    from nbed_amd import xc

    assert xc.XCProvider.RHO_FLOOR == FLOOR
    if regime == "all":
        (rho, grad, w), ref, bound = _all_regimes(name)
        assert rho.shape[1] == 640
    else:
        rho, grad, w = gr.regime_inputs(regime, FLOOR)
        ref = gr.regime_reference(name, regime, FLOOR)
        bound = gr.entry_bound(regime, ref)
        print(f"XCREF own {name} {regime} entries {gr.own_error(ref):.2e} exc {ref[6][2]:.2e}")
        assert rho.shape[1] == 64
    gr.check_functional(f"kernel {name} {regime}", _kernel_functional(be, name, rho, grad, w), ref, bound)


@pytest.mark.parametrize("regime,index", [("existing", 0), ("polarised_beta_empty", 0), ("polarised_alpha_empty", 149),
                                          ("at_floor", 0), ("at_floor", 1)])
@pytest.mark.parametrize("name", gr.FUNCTIONALS)
def test_functional_kernel_on_a_grid_of_one_point(be, name, regime, index):
    rho, grad, w = xr.regime_inputs(regime, FLOOR)
    rho, grad, w = rho[:, index:index + 1], grad[:, :, index:index + 1], w[index:index + 1]
    ref = gr.functional_reference(name, rho, grad, w, FLOOR)
    if regime == "at_floor":
        assert bool(ref[4][0]) == bool(index)  # exactly on the floor: dropped; one ulp above: kept
    gr.check_functional(f"kernel {name} {regime}[{index}]", _kernel_functional(be, name, rho, grad, w), ref,
                        gr.entry_bound(regime, ref))


def test_an_unknown_code_is_refused(be):
    from nbed_amd import _nbx

    rho, grad, w = gr.regime_inputs("existing", FLOOR)
    for code in (-1, 9):
        with pytest.raises(_nbx.NbxError):
            be.xc_functional(code, be.asarray(rho), be.asarray(grad), be.asarray(w), FLOOR)


# ------------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("name", ["pbe", "b3lyp5"])
def test_h_atom_open_shell_chain(be, name):
    """tests/test_gpu_xc.py::test_h_atom_open_shell_chain for the new names, same construction and bounds: H / 6-31G,
    one alpha electron, no beta electron, on a 24 x 6 x 12 product grid (1728 points): XCProvider on the device
    against XCProvider on the host and against the references chained on the same points.  E_xc: 1e-12 relative to
    the host and 1e-11 to the reference; v_xc: 1e-10 of the largest entry of each spin."""
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
    assert 1000 < npts < 2500 and bs.pure_cartesian
    e_dev, v_dev = dev(dm)
    e_host, v_host = host(dm)
    shells = [(sh.centre, sh.exps, sh.coefs, [tuple(lmn) for lmn in sh.cart]) for sh in bs.shells]
    ao, dao, _, _ = xr.ao_reference(shells, dev.points)
    dml = np.asarray(dm, dtype=xr.LD)
    cmat = np.stack([ao @ dml[x] for x in range(2)])
    rho = (cmat * ao[None]).sum(axis=2).astype(np.float64)
    grad = np.stack([[2 * (cmat[x] * dao[a]).sum(axis=1) for a in range(3)] for x in range(2)]).astype(np.float64)
    assert not rho[1].any() and not grad[1].any() and abs(dev.nelec_last - 1.0) < 1e-4
    vr, vec, exc, nelec, keep, _, _ = gr.functional_reference(name, rho, grad, dev.weights, FLOOR, own_error=False)
    assert keep.sum() > npts // 2
    e_rel_host, e_rel_ref = abs(e_dev - e_host) / abs(e_host), xr.rel_err_scalar(e_dev, exc)
    v_ref, _ = xr.vmat_reference(ao.astype(np.float64), dao.astype(np.float64), vr.astype(np.float64), vec.astype(np.float64))
    v_ref = v_ref.astype(np.float64)
    dv_host = [np.abs(v_dev[x] - v_host[x]).max() / np.abs(v_host[x]).max() for x in range(2)]
    dv_ref = [np.abs(v_dev[x] - v_ref[x]).max() / np.abs(v_ref[x]).max() for x in range(2)]
    print(f"XCCHAIN {name} npts {npts} E_xc {e_dev:.12f} rel host {e_rel_host:.2e} ref {e_rel_ref:.2e} "
          f"v rel host {dv_host[0]:.2e} {dv_host[1]:.2e} ref {dv_ref[0]:.2e} {dv_ref[1]:.2e}")
    assert xr.rel_err_scalar(dev.nelec_last, nelec) < 1e-11
    assert e_rel_host < 1e-12 and e_rel_ref < 1e-11
    assert np.abs(v_ref[1]).max() > 1e-3  # the empty spin's potential is not small
    assert max(dv_host) < 1e-10 and max(dv_ref) < 1e-10


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("projector", ["mu", "huzinaga"])
def test_driver_pbe_dft_in_dft_water(be, projector):
    """``nbed`` with xc_functional='pbe' (global Kohn-Sham, embedding, DFT-in-DFT) on libnbx: the subsystem energies
    add up to the global energy (1e-8) and DFT-in-DFT embedding reproduces the global Kohn-Sham energy -- Huzinaga to
    1e-9, the level shift to 5e-6, the figures of tests/test_reference_kats.py::test_dft_in_dft_reproduces_global_ks.
    The identity holds to the residual of the global run: convergence = 1e-8 (at 1e-6 the Huzinaga figure is 2e-9 on
    either backend)."""
    from nbed_amd import NbedConfig, nbed
    from nbed_amd.driver import BuiltinHFProvider

    cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional="pbe", projector=projector,
                     localization="spade", convergence=1e-8, mu_level_shift=1e6, max_hf_cycles=100, max_dft_cycles=100,
                     run_fci_emb=False, run_ccsd_emb=False, run_dft_in_dft=True)
    drv = nbed(cfg, backend=be)
    assert isinstance(drv.provider, BuiltinHFProvider)
    res = drv.mu if projector == "mu" else drv.huzinaga
    ks = drv._global_ks
    assert ks.converged and res["scf"].converged
    assert ks.xc_provider._ao is not None  # the quadrature ran on the device
    print(f"XCE2E pbe {projector} e_ks {ks.e_tot:.10f} dft_in_dft - ks {res['e_dft_in_dft'] - ks.e_tot:.2e} "
          f"sum rule {drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot:.2e}")
    assert abs(ks.e_tot - (-75.2218469195)) < 2e-8  # the host quadrature's number (tests/test_host_xc_gga.py runs it)
    assert abs(drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot) < 1e-8
    assert abs(res["e_dft_in_dft"] - ks.e_tot) < (5e-6 if projector == "mu" else 1e-9)


def test_b3lyp5_is_not_b3lyp(be):
    """The same molecule with ``b3lyp5`` and ``b3lyp``: 0.19 (VWN5 - VWN-RPA) moves the energy by 37 mHa."""
    from nbed_amd import NbedConfig
    from nbed_amd.driver import BuiltinHFProvider

    prov = BuiltinHFProvider(be)
    e = {}
    for name in ("b3lyp", "b3lyp5"):
        cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional=name, convergence=1e-8,
                         max_dft_cycles=100)
        ks = prov.global_ks(cfg)
        assert ks.converged
        e[name] = ks.e_tot
    print(f"XCE2E b3lyp {e['b3lyp']:.10f} b3lyp5 {e['b3lyp5']:.10f}")
    assert abs(e["b3lyp"] - (-75.3091447400438)) < 2e-8  # tests/test_reference_kats.py::test_global_ks_b3lyp
    assert abs(e["b3lyp5"] - e["b3lyp"]) > 1e-4
    assert abs(e["b3lyp5"] - (-75.2718528669)) < 2e-8  # the host quadrature's number
