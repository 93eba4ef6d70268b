"""``cam-b3lyp`` and ``lc-blyp`` on the device: nbx_xc_functional_rs (csrc/xc.hip) against the 50-digit reference of
tests/xc_rs_reference.py -- every regime, all regimes in one launch, grids of one point, chosen values of the attenuation
parameter a -- the whole quadrature chain on one atom against the host, and ``nbed`` end to end on HipBackend.

Bounds: those of tests/test_gpu_xc_gga.py.  Per entry of ``vr`` and ``vec`` 5e-11 of the sum of the magnitudes of the
pieces' exact contributions (at least 1e-150); E_xc 1e-12 of sum_g w |piece|; the electron count 1e-12.  Dropped points are
exact zeros and nothing is non-finite.  The loose rule of ``tails`` and ``at_floor`` is not used: the kernel does not need
it, and the reference's own 53-bit evaluation is no guide here -- it forms the sigma derivative as G' F + G F' da/dsigma,
whose leading orders cancel at large a (2e-9 in ``existing``), where the kernel sums P = F + a F' / 2 term by term.

Measured worst entry (MI355X, 64 points per regime, 16 per chosen a, the worse of the two names):

  existing 8.6e-15, closed_shell 2.8e-15, polarised_beta_empty 9.7e-15, polarised_alpha_empty 1.4e-14,
  polarisation_1e4_1e12 2.7e-14, core 4.5e-15, tails 5.6e-14, zero_gradient 2.7e-15, antiparallel 2.0e-14, at_floor 8.1e-14,
  all regimes in one launch 8.1e-14, grids of one point <= 3.0e-14 (exactly on the floor: exact zeros),
  a = 0.5 (1 -+ 2^-20) 2.9e-14 / 2.2e-15, a = 1e-6 6.6e-16, a = 1e4 4.7e-15; E_xc <= 2.5e-14 of sum w |piece|.
  Chain on the H atom: E_xc 3e-16 relative to the host, v_xc 6e-16; water / STO-3G end to end: device and host
  backends agree in all ten printed decimals (cam-b3lyp -75.2765112172).
"""

import numpy as np
import pytest

import xc_gga_reference as gr
import xc_reference as xr
import xc_rs_reference as rs

pytestmark = pytest.mark.gpu

FLOOR = 1e-14
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


def _kernel_functional(be, name, rho, grad, w, omega=0.33):
    from nbed_amd import _nbx

    vr, vec, sums = be.xc_functional_rs(_nbx.XC_RS_CODES[name], omega, be.asarray(rho), be.asarray(grad), be.asarray(w), FLOOR)
    sums = be.to_host(sums)
    return be.to_host(vr), be.to_host(vec), float(sums[0]), float(sums[1])


def _all_regimes(name):
    """Every regime in one launch: 640 points, two and a half blocks."""
    import mpmath as mp

    ins = [rs.regime_inputs(r, FLOOR) for r in xr.REGIMES]
    refs = [rs.regime_reference(name, r, FLOOR) for r in xr.REGIMES]
    with mp.workdps(xr.DPS):
        exc, nelec, mexc = sum(r[2] for r in refs), sum(r[3] for r in refs), sum(r[5][2] for r in refs)
    ref = (np.concatenate([r[0] for r in refs], axis=1), np.concatenate([r[1] for r in refs], axis=2), exc, nelec,
           np.concatenate([r[4] for r in refs]),
           (np.concatenate([r[5][0] for r in refs], axis=1), np.concatenate([r[5][1] for r in refs], axis=2), mexc), None)
    return tuple(np.concatenate([i[k] for i in ins], axis=-1) for k in range(3)), ref


@pytest.mark.parametrize("regime", xr.REGIMES + ("all",))
@pytest.mark.parametrize("name", rs.FUNCTIONALS)
def test_functional_kernel_against_the_50_digit_reference(be, name, regime):
    from nbed_amd import xc

    assert xc.XCProvider.RHO_FLOOR == FLOOR and xc.rsh_parameters(name)[0] == 0.33
    if regime == "all":
        (rho, grad, w), ref = _all_regimes(name)
        assert rho.shape[1] == 640
    else:
        rho, grad, w = rs.regime_inputs(regime, FLOOR)
        ref = rs.regime_reference(name, regime, FLOOR)
        assert rho.shape[1] == 64
    gr.check_functional(f"kernel {name} {regime}", _kernel_functional(be, name, rho, grad, w), ref, gr.ENTRY_BOUND)


@pytest.mark.parametrize("regime,index", [("existing", 0), ("polarised_beta_empty", 0), ("polarised_alpha_empty", 149),
                                          ("at_floor", 0), ("at_floor", 1)])
@pytest.mark.parametrize("name", rs.FUNCTIONALS)
def test_functional_kernel_on_a_grid_of_one_point(be, name, regime, index):
    rho, grad, w = xr.regime_inputs(regime, FLOOR)
    rho, grad, w = rho[:, index:index + 1], grad[:, :, index:index + 1], w[index:index + 1]
    ref = rs.functional_reference(name, rho, grad, w, FLOOR)
    if regime == "at_floor":
        assert bool(ref[4][0]) == bool(index)  # exactly on the floor: dropped; one ulp above: kept
    gr.check_functional(f"kernel {name} {regime}[{index}]", _kernel_functional(be, name, rho, grad, w), ref, gr.ENTRY_BOUND)


@pytest.mark.parametrize("case", [c[0] for c in rs.A_CASES])
@pytest.mark.parametrize("name", rs.FUNCTIONALS)
def test_functional_kernel_at_chosen_a(be, name, case):
    """a just below and just above the switch point of F, a = 1e-6 and a = 1e4 (the kernel takes any omega)."""
    omega, rho, grad, w = rs.a_case_inputs(case)
    ref = rs.a_case_reference(name, case, FLOOR)
    gr.check_functional(f"kernel {name} {case}", _kernel_functional(be, name, rho, grad, w, omega), ref, gr.ENTRY_BOUND)


def test_lc_blyp_at_omega_zero_is_the_blyp_kernel(be):
    rho, grad, w = rs.regime_inputs("existing", FLOOR)
    blyp = gr.regime_reference("blyp", "existing", FLOOR)
    gr.check_functional("kernel lc-blyp(omega = 0) against blyp", _kernel_functional(be, "lc-blyp", rho, grad, w, 0.0), blyp,
                        gr.ENTRY_BOUND)


def test_entry_points_keep_to_their_codes(be):
    """The old entry point still refuses the new codes (and 9); the new one refuses the old codes and a bad omega."""
    from nbed_amd import _nbx

    rho, grad, w = (be.asarray(x) for x in rs.regime_inputs("existing", FLOOR))
    for code in (-1, 9, 16, 17):
        with pytest.raises(_nbx.NbxError):
            be.xc_functional(code, rho, grad, w, FLOOR)
    for code in (0, 3, 7, 8, 9, 15, 18):
        with pytest.raises(_nbx.NbxError):
            be.xc_functional_rs(code, 0.33, rho, grad, w, FLOOR)
    for omega in (-0.33, float("nan"), float("inf")):
        with pytest.raises(_nbx.NbxError):
            be.xc_functional_rs(16, omega, rho, grad, w, FLOOR)


# ------------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("name", rs.FUNCTIONALS)
def test_h_atom_open_shell_chain(be, name):
    """tests/test_gpu_xc.py::test_h_atom_open_shell_chain for the two names, same construction and bounds: H / 6-31G, one
    alpha electron, no beta electron, on a 24 x 6 x 12 product grid (1728 points): XCProvider on the device against
    XCProvider on the host and against the references chained on the same points.  E_xc: 1e-12 relative to the host and
    1e-11 to the reference; v_xc: 1e-10 of the largest entry of each spin."""
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
    vr, vec, exc, nelec, keep, _, _ = rs.functional_reference(name, rho, grad, dev.weights, FLOOR)
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
def _config(name, **kw):
    from nbed_amd import NbedConfig

    base = dict(geometry=WATER, n_active_atoms=1, basis="STO-3G", xc_functional=name, projector="both", localization="spade",
                convergence=1e-8, mu_level_shift=1e6, max_hf_cycles=100, max_dft_cycles=100, run_fci_emb=False,
                run_ccsd_emb=False, run_dft_in_dft=True)
    base.update(kw)
    return NbedConfig(**base)


def test_driver_cam_b3lyp_on_the_device_equals_the_host_backend(be):
    """``nbed`` with cam-b3lyp, both projectors and DFT-in-DFT on HipBackend (device integral engine for both tensors,
    device quadrature, libnbx J/K on both) against the same run on the host checker backend, to the bound the PBE driver
    test holds between the device quadrature and the host's number (2e-8) -- for the embedded energies of the level-shift
    projector 2e-6, because mu = 1e6 amplifies rounding differences between two backends a hundredfold (the 1e-6 against
    1e-8 of tests/test_host_driver.py::test_embed_matches_oracle_flow) -- and the identities of tests/test_host_rsh.py
    on the device."""
    from oracle_backend import OracleBackend

    from nbed_amd import nbed
    from nbed_amd.driver import BuiltinHFProvider

    cfg = _config("cam-b3lyp")
    drv = nbed(cfg, provider=BuiltinHFProvider(be, eri_engine="device"), backend=be)
    ref = nbed(cfg, backend=OracleBackend())
    ks = drv._global_ks
    assert ks.converged and ks.xc_provider._ao is not None and ks._eri_lr_d.is_cuda and ks.beta == 0.46
    print(f"XCE2E cam-b3lyp device e_ks {ks.e_tot:.10f} host {ref._global_ks.e_tot:.10f} mu - huz "
          f"{drv.mu['e_rhf'] - drv.huzinaga['e_rhf']:.2e} dft_in_dft - ks mu {drv.mu['e_dft_in_dft'] - ks.e_tot:.2e} "
          f"huz {drv.huzinaga['e_dft_in_dft'] - ks.e_tot:.2e}")
    assert abs(ks.e_tot - ref._global_ks.e_tot) < 2e-8
    for proj in ("mu", "huzinaga"):
        got, want = getattr(drv, proj), getattr(ref, proj)
        assert got["scf"].converged
        for key in ("e_rhf", "e_dft_in_dft"):
            assert abs(got[key] - want[key]) < (2e-6 if proj == "mu" else 2e-8), (proj, key, got[key], want[key])
    assert abs(drv.mu["e_rhf"] - drv.huzinaga["e_rhf"]) < 1e-5
    assert abs(drv.huzinaga["e_dft_in_dft"] - ks.e_tot) < 1e-9 and abs(drv.mu["e_dft_in_dft"] - ks.e_tot) < 5e-6
    assert abs(drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - ks.e_tot) < 1e-8


def test_lc_blyp_is_not_blyp(be):
    from nbed_amd.driver import BuiltinHFProvider

    prov = BuiltinHFProvider(be)
    e = {}
    for name in ("blyp", "lc-blyp"):
        ks = prov.global_ks(_config(name))
        assert ks.converged
        e[name] = ks.e_tot
    print(f"XCE2E blyp {e['blyp']:.10f} lc-blyp {e['lc-blyp']:.10f} difference {e['lc-blyp'] - e['blyp']:.6f}")
    assert abs(e["lc-blyp"] - e["blyp"]) > 1e-3
