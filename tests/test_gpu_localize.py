"""Pipek-Mezey and Boys on the MI355X: nbx_loc_pm / nbx_loc_boys against the numpy restatement
(tests/loc_reference.py), the localizers on real molecules of the built-in provider, and the driver end to end."""

import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

import loc_reference as ref

from nbed_amd import NbedConfig, _nbx, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.localizers import BOYSLocalizer, PMLocalizer
from nbed_amd.localizers.occupied.base import check_values

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
from molecules import octane_xyz  # noqa: E402

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


def _offsets(rng, nao, natm):
    inner = np.sort(rng.choice(np.arange(1, nao), natm - 1, replace=False)) if natm > 1 else []
    return np.concatenate([[0], inner, [nao]]).astype(np.int64)


def _raw(be, kind, batch_inputs, max_sweeps, tol=1e-10):
    """One launch through the C ABI; returns (U (batch, n, n), sweeps, f, rc of nbx_loc_status)."""
    lib = be.lib
    if kind == "boys":
        q = be.asarray(np.array(batch_inputs))
        batch, n = q.shape[0], q.shape[-1]
        nbytes = lib.nbx_loc_worksize(_nbx.LOC_BOYS, batch, 0, n, 0)
        work = be._workspace("loc_test", nbytes)
        u = be.empty((batch, n, n))
        _nbx.check(lib, lib.nbx_loc_boys(be.ctx, batch, n, be._p(q), be._p(u), max_sweeps, tol, be._p(work), work.numel()))
    else:
        xs, ys, offs = batch_inputs
        x = be.asarray(np.array(xs))
        y = None if ys is None else be.asarray(np.array(ys))
        batch, nao, n = x.shape
        natm = len(offs) - 1
        nbytes = lib.nbx_loc_worksize(_nbx.LOC_PM, batch, nao, n, natm)
        work = be._workspace("loc_test", nbytes)
        u = be.empty((batch, n, n))
        o = np.ascontiguousarray(offs, dtype=np.int64)
        _nbx.check(lib, lib.nbx_loc_pm(be.ctx, batch, nao, n, natm, o.ctypes.data_as(ctypes.c_void_p), be._p(x),
                                       be._p(y), be._p(u), max_sweeps, tol, be._p(work), work.numel()))
    sweeps = (ctypes.c_int * batch)()
    f = (ctypes.c_double * batch)()
    rc = lib.nbx_loc_status(be.ctx, batch, be._p(work), sweeps, f)
    return be.to_host(u), np.array(sweeps[:]), np.array(f[:]), rc


PM_CASES = [(1, 1, 5, True), (2, 3, 8, False), (3, 3, 12, True), (7, 3, 20, False), (33, 26, 148, True),
            (33, 26, 148, False), (64, 26, 148, True), (65, 60, 200, False), (81, 60, 300, True), (128, 3, 160, True),
            (200, 60, 400, False)]


@pytest.mark.parametrize("n,natm,nao,same", PM_CASES)
def test_pm_kernel_follows_the_restatement(be, n, natm, nao, same):
    """A fixed number of sweeps on both sides: the same trajectory, LDS (small) and global (large) working sets."""
    rng = np.random.default_rng(n * 1000 + natm)
    offs = _offsets(rng, nao, natm)
    x = np.linalg.qr(rng.normal(size=(nao, n)))[0]
    y = None if same else x * rng.uniform(0.5, 1.5, size=(nao, 1))
    sweeps = 3
    u, sw, f, _ = _raw(be, "pm", ([x, x], None if same else [y, y], offs), sweeps)
    u_ref, sw_ref, f_ref, _ = ref.localize_pm(x, y, offs, max_sweeps=sweeps)
    assert sw[0] == sw_ref and sw[1] == sw_ref
    assert abs(f[0] - f_ref) <= 1e-12 * abs(f_ref)
    np.testing.assert_allclose(u[0], u_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(u[0].T @ u[0], np.eye(n), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(u[0], u[1])  # identical problems of one batch: identical bits
    u2, _, f2, _ = _raw(be, "pm", ([x, x], None if same else [y, y], offs), sweeps)
    np.testing.assert_array_equal(u2, u)  # and repeated calls
    np.testing.assert_array_equal(f2, f)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 33, 64, 65, 81, 128, 200])
def test_boys_kernel_follows_the_restatement(be, n):
    rng = np.random.default_rng(n)
    v = np.linalg.qr(rng.normal(size=(n, n)))[0]
    q = np.array([v.T @ (np.diag(rng.normal(size=n)) + 0.05 * (e + e.T)) @ v
                  for e in rng.normal(size=(3, n, n))])
    sweeps = 3
    u, sw, f, _ = _raw(be, "boys", [q, q], sweeps)
    u_ref, sw_ref, f_ref, _ = ref.localize_boys(q, max_sweeps=sweeps)
    assert sw[0] == sw_ref
    assert abs(f[0] - f_ref) <= 1e-12 * abs(f_ref)
    np.testing.assert_allclose(u[0], u_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(u[0].T @ u[0], np.eye(n), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(u[0], u[1])


@pytest.mark.parametrize("n", [33, 81])
def test_boys_kernel_converges_to_the_restatement(be, n):
    """Nearly commuting matrices: a well-conditioned maximum, reached by both to the last digits."""
    rng = np.random.default_rng(7 + n)
    v = np.linalg.qr(rng.normal(size=(n, n)))[0]
    q = np.array([v.T @ (np.diag(rng.normal(size=n)) + 0.02 * (e + e.T)) @ v for e in rng.normal(size=(3, n, n))])
    u, sweeps, f = be.localize_boys(be.asarray(q[None]))
    u = be.to_host(u)[0]
    u_ref, _, f_ref, conv = ref.localize_boys(q)
    assert conv and abs(f[0] - f_ref) <= 1e-12 * f_ref
    _assert_same_columns(u, u_ref, 1e-8)
    qq = np.einsum("pi,kpq,qj->kij", u, q, u)
    assert ref.all_pair_gains(qq).max() <= 1e-12 * f[0]


def test_pm_kernel_converges_to_the_restatement(be):
    rng = np.random.default_rng(5)
    nao, n, natm = 60, 12, 12
    offs = np.arange(0, nao + 1, nao // natm)
    z = np.zeros((nao, n))  # orbital i mostly on atom i: a well-separated maximum
    for i in range(n):
        z[:, i] = 0.05 * rng.normal(size=nao)
        z[offs[i]:offs[i + 1], i] += rng.normal(size=offs[i + 1] - offs[i])
    x = np.linalg.qr(z @ np.linalg.qr(rng.normal(size=(n, n)))[0])[0]
    u, sweeps, f = be.localize_pm(be.asarray(x[None]), None, offs)
    u = be.to_host(u)[0]
    u_ref, _, f_ref, conv = ref.localize_pm(x, None, offs)
    assert conv and abs(f[0] - f_ref) <= 1e-12 * f_ref
    _assert_same_columns(u, u_ref, 1e-8)
    assert ref.all_pair_gains(ref.pm_matrices(x @ u, x @ u, offs)).max() <= 1e-12 * f[0]


def test_bad_arguments_are_refused(be):
    lib = be.lib
    x = be.asarray(np.eye(4)[None])
    u = be.empty((1, 4, 4))
    work = be._workspace("loc_test", lib.nbx_loc_worksize(_nbx.LOC_PM, 1, 4, 4, 2))
    for offs in ([0, 3, 2], [1, 2, 4], [0, 2, 5]):
        o = np.array(offs, dtype=np.int64)
        rc = lib.nbx_loc_pm(be.ctx, 1, 4, 4, 2, o.ctypes.data_as(ctypes.c_void_p), be._p(x), None, be._p(u), 10, 1e-10,
                            be._p(work), work.numel())
        assert rc == _nbx.NBX_E_INVALID
    o = np.array([0, 2, 4], dtype=np.int64)
    assert lib.nbx_loc_pm(be.ctx, 1, 4, 4, 2, o.ctypes.data_as(ctypes.c_void_p), be._p(x), None, be._p(u), 10, 1e-10,
                          be._p(work), 16) == _nbx.NBX_E_INVALID
    assert lib.nbx_loc_pm(be.ctx, 1, -4, 4, 2, o.ctypes.data_as(ctypes.c_void_p), be._p(x), None, be._p(u), 10, 1e-10,
                          be._p(work), work.numel()) == _nbx.NBX_E_INVALID
    # the sweep limit: results written, NBX_E_NOCONV reported
    rng = np.random.default_rng(0)
    q = rng.normal(size=(3, 20, 20))
    q = q + q.transpose(0, 2, 1)
    u1, sw, f, rc = _raw(be, "boys", [q], 1)
    assert rc == _nbx.NBX_E_NOCONV and sw[0] == 1 and np.isfinite(u1).all()


def _assert_same_columns(a, b, atol):
    """Equal up to the sign and the order of the columns."""
    used = set()
    for j in range(a.shape[1]):
        d = [min(np.abs(a[:, j] - b[:, k]).max(), np.abs(a[:, j] + b[:, k]).max()) for k in range(b.shape[1])]
        k = int(np.argmin(d))
        assert d[k] < atol and k not in used, (j, d[k])
        used.add(k)


# ---------------------------------------------------------------------------------------------- real molecules
@pytest.fixture(scope="module")
def molecules(be):
    out = {}
    for name, xyz, basis in (("water_sto3g", WATER, "STO-3G"), ("water_ccpvdz", WATER, "cc-pVDZ"),
                             ("octane", octane_xyz(), "6-31G*")):
        cfg = NbedConfig(geometry=xyz, n_active_atoms=1, basis=basis, xc_functional="hf", convergence=1e-10,
                         max_hf_cycles=100, max_dft_cycles=100)
        prov = BuiltinHFProvider(be)
        out[name] = prov.global_hf(cfg)
    return out


def _loc(kind, scf, be):
    if kind == "boys":
        return BOYSLocalizer(scf, 1, backend=be)
    return PMLocalizer(scf, 1, pop_method=kind, backend=be)


@pytest.mark.parametrize("name", ["water_sto3g", "water_ccpvdz", "octane"])
@pytest.mark.parametrize("kind", ["boys", "mulliken", "lowdin"])
def test_real_molecule_localization(be, molecules, name, kind):
    scf = molecules[name]
    loc = _loc(kind, scf, be)
    ls = loc.localize()
    s = np.asarray(scf.get_ovlp())
    nocc = int(np.count_nonzero(scf.mo_occ[0]))
    c_occ = np.asarray(scf.mo_coeff[0])[:, :nocc]
    c_loc = np.asarray(ls.c_loc_occ[0])
    np.testing.assert_allclose(c_loc @ c_loc.T, c_occ @ c_occ.T, rtol=0, atol=1e-12)
    np.testing.assert_allclose(c_loc.T @ s @ c_loc, np.eye(nocc), rtol=0, atol=1e-12)
    if np.array_equal(scf.mo_coeff[0], scf.mo_coeff[1]):  # identical spins, identical bits
        np.testing.assert_array_equal(ls.c_loc_occ[0], ls.c_loc_occ[1])
    # stationary: no pair can gain more than 1e-12 f
    if kind == "boys":
        q = ref.boys_matrices(c_loc, scf.mol.intor_symmetric("int1e_r", comp=3))
    else:
        sl = np.asarray(scf.mol.aoslice_by_atom())
        offs = np.concatenate([[0], sl[:, 3]])
        if kind == "mulliken":
            q = ref.pm_matrices(c_loc, s @ c_loc, offs)
        else:
            w, v = np.linalg.eigh(s)
            xo = (v * np.sqrt(w)) @ v.T @ c_loc
            q = ref.pm_matrices(xo, xo, offs)
    f = ref.functional(q)
    assert abs(f - loc.functional[0]) <= 1e-10 * f
    assert ref.all_pair_gains(q).max() <= 1e-12 * f


def test_water_boys_is_unique_and_symmetric(be, molecules):
    scf = molecules["water_ccpvdz"]
    s = np.asarray(scf.get_ovlp())
    nocc = int(np.count_nonzero(scf.mo_occ[0]))
    c_occ = np.asarray(scf.mo_coeff[0])[:, :nocc]
    r = scf.mol.intor_symmetric("int1e_r", comp=3)
    rng = np.random.default_rng(3)
    results = []
    for _ in range(2):  # two random starting rotations of the occupied space reach the same orbitals
        c0 = c_occ @ np.linalg.qr(rng.normal(size=(nocc, nocc)))[0]
        cd = be.asarray(c0[None])
        q = be.empty((1, 3, nocc, nocc))
        be.gemm(cd[0], be.gemm(be.asarray(r), cd[0]), "T", "N", out=q[0])
        u, _, _ = be.localize_boys(q)
        results.append(c0 @ be.to_host(u)[0])
    _assert_same_columns(results[0], results[1], 1e-6)
    # the two O-H bonds are mirror images: their H1 / H2 Mulliken populations swap
    sl = np.asarray(scf.mol.aoslice_by_atom())
    c = results[0]
    pops = np.array([[np.sum((c[a0:a1, i]) * (s @ c[:, i])[a0:a1]) for (_, _, a0, a1) in sl] for i in range(nocc)])
    bonds = np.argsort(pops[:, 1] + pops[:, 2])[-2:]
    b1, b2 = bonds[np.argsort(pops[bonds, 1])[::-1]]
    assert abs(pops[b1, 1] - pops[b2, 2]) < 1e-8 and abs(pops[b1, 2] - pops[b2, 1]) < 1e-8
    assert pops[b1, 1] > 0.2


# ---------------------------------------------------------------------------------------------- driver end to end
@pytest.mark.parametrize("projector", ["mu", "huzinaga"])
@pytest.mark.parametrize("n_active_atoms", [1, 2])
def test_driver_boys_hf_in_hf_water(be, projector, n_active_atoms):
    cfg = NbedConfig(geometry=WATER, n_active_atoms=n_active_atoms, basis="STO-3G", xc_functional="hf",
                     projector=projector, localization="boys", convergence=1e-10, max_hf_cycles=100,
                     max_dft_cycles=100, virtual_localization="disable")
    drv = nbed(cfg, backend=be)
    res = drv.mu if projector == "mu" else drv.huzinaga
    e_global = drv._global_ks.e_tot
    assert res["scf"].converged
    assert abs(res["e_rhf"] - e_global) < 2e-6
    assert abs(drv.e_act + drv.e_env + drv.two_e_cross + drv.e_nuc - e_global) < 1e-8
    check_values(drv.localized_system, drv._global_ks)


def test_driver_boys_b3lyp_water_ccpvdz(be):
    cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="cc-pVDZ", xc_functional="b3lyp", projector="huzinaga",
                     localization="boys", convergence=1e-8, max_hf_cycles=100, max_dft_cycles=100,
                     virtual_localization="cl")
    drv = nbed(cfg, backend=be)
    assert drv.huzinaga["scf"].converged and np.isfinite(drv.huzinaga["e_rhf"])
    check_values(drv.localized_system, drv._global_ks)


def test_driver_boys_octane(be):
    cfg = NbedConfig(geometry=octane_xyz(), n_active_atoms=4, basis="6-31G*", xc_functional="b3lyp",
                     projector="huzinaga", localization="boys", convergence=1e-8, max_hf_cycles=100,
                     max_dft_cycles=100, virtual_localization="disable")
    drv = nbed(cfg, backend=be)
    assert drv.huzinaga["scf"].converged and np.isfinite(drv.huzinaga["e_rhf"])
    check_values(drv.localized_system, drv._global_ks)


class _Restricted:
    """The restricted view of a closed-shell unrestricted mean field (the reference's global_rks fixture)."""

    def __init__(self, uks):
        self.mol, self._uks = uks.mol, uks
        self.mo_coeff = np.asarray(uks.mo_coeff[0])
        self.mo_occ = 2.0 * np.asarray(uks.mo_occ[0])

    def get_ovlp(self):
        return self._uks.get_ovlp()

    def make_rdm1(self):
        c = self.mo_coeff[:, self.mo_occ > 0]
        return 2.0 * c @ c.T


@pytest.fixture(scope="module")
def water_631g_b3lyp(be):
    """The reference's tests/test_localizers.py fixture: water / 6-31G, B3LYP, n_active_atoms = 1."""
    cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="6-31G", xc_functional="b3lyp", convergence=1e-6,
                     max_hf_cycles=100, max_dft_cycles=100)
    uks = BuiltinHFProvider(be).global_ks(cfg)
    return _Restricted(uks), uks


@pytest.mark.parametrize("kind", ["lowdin", "boys"])
def test_reference_pm_check_values_and_mo_indices(be, water_631g_b3lyp, kind):
    """Ports of test_PM_check_values, test_PM_mo_indices and test_PMLocalizer_local_basis_transform
    (tests/test_localizers.py:96-194)."""
    rks, uks = water_631g_b3lyp
    systems = []
    for ks in (rks, uks):
        loc = _loc(kind, ks, be)
        ls = loc.localize()
        check_values(ls, loc._global_scf)
        systems.append(ls)
    restricted, unrestricted = systems
    assert np.all(restricted.active_mo_inds == unrestricted.active_mo_inds[0])
    assert np.all(restricted.enviro_mo_inds == unrestricted.enviro_mo_inds[1])
    assert np.all(unrestricted.active_mo_inds[0] == unrestricted.active_mo_inds[1])
    assert np.all(unrestricted.enviro_mo_inds[0] == unrestricted.enviro_mo_inds[1])
    dm_full = rks.make_rdm1()
    np.testing.assert_allclose(restricted.dm_active + restricted.dm_enviro, dm_full, rtol=0, atol=1e-10)
    s = rks.get_ovlp()
    n_act = np.trace(restricted.dm_active @ s)
    n_env = np.trace(restricted.dm_enviro @ s)
    assert abs(n_act + n_env - rks.mol.nelectron) < 1e-10
