"""Host side of the Pipek-Mezey / Boys localizers (nbed_amd/localizers/occupied/jacobi.py) and the dipole
integrals Boys needs: no GPU.  The sweeps themselves run on the numpy restatement (tests/loc_reference.py) through
a checker backend; the kernels are tested against it in test_gpu_localize.py."""

import numpy as np
import pytest

import loc_reference as ref
from oracle import gto as oracle_gto
from oracle_backend import OracleBackend
from synthetic_provider import SyntheticProvider

from nbed_amd import NbedConfig, integrals, nbed
from nbed_amd.localizers import BOYSLocalizer, IBOLocalizer, PMLocalizer
from nbed_amd.localizers.occupied.base import check_values
from nbed_amd.scf import Mole

WATER_XYZ = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"


class LocCheckerBackend(OracleBackend):
    """OracleBackend plus the two localisation entry points, on the numpy restatement."""

    def localize_pm(self, x, y, ao_offsets, max_sweeps=1000, tol=1e-10):
        out = [ref.localize_pm(self._np(x[b]), None if y is None else self._np(y[b]), list(ao_offsets), max_sweeps, tol)
               for b in range(x.shape[0])]
        return self._pack(out)

    def localize_boys(self, q, max_sweeps=1000, tol=1e-10):
        return self._pack([ref.localize_boys(self._np(q[b]), max_sweeps, tol) for b in range(q.shape[0])])

    def _pack(self, out):
        assert all(r[3] for r in out), "no convergence"
        return (self.asarray(np.array([r[0] for r in out])), np.array([r[1] for r in out]),
                np.array([r[2] for r in out]))


# ---------------------------------------------------------------------------------------------- dipole integrals
@pytest.mark.parametrize("basis,cart", [("sto-3g", False), ("cc-pvdz", False), ("6-31g*", False), ("6-31g*", True)])
def test_native_dipole_matches_numpy_engine(basis, cart):
    bs = integrals.Basis(integrals.parse_geometry(WATER_XYZ), basis, cart)
    r = integrals.dipole(bs)
    for nthreads in (1, 0):
        got = integrals.dipole_native(bs, nthreads=nthreads)
        assert got.shape == (3, bs.nao, bs.nao)
        np.testing.assert_allclose(got, r, rtol=0, atol=1e-13)
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))


def test_dipole_against_oracle_primitive_overlaps():
    """x_B G_b(l) = G_b(l + 1_x): <a|x|b> = <a|b(l + 1_x)> + B_x <a|b>, from oracle/gto.py's primitive overlap."""

    def dipole_prim(a, lmn1, centre_a, b, lmn2, centre_b, d):
        up = tuple(v + (k == d) for k, v in enumerate(lmn2))
        return (oracle_gto._overlap_prim(a, lmn1, centre_a, b, up, centre_b)
                + centre_b[d] * oracle_gto._overlap_prim(a, lmn1, centre_a, b, lmn2, centre_b))

    for basis in ("cc-pvdz", "6-31g*"):
        ob = oracle_gto.SphericalBasis(oracle_gto.parse_xyz(WATER_XYZ), integrals.BASIS_SETS[basis])
        want = np.array([[[oracle_gto._ao_pair(fi, fj, dipole_prim, d) for fj in ob.aos] for fi in ob.aos]
                         for d in range(3)])
        got = integrals.dipole_native(integrals.Basis(integrals.parse_geometry(WATER_XYZ), basis))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_dipole_origin_shift():
    atoms = integrals.parse_geometry(WATER_XYZ)
    d = np.array([0.3, -0.7, 1.1])
    bs = integrals.Basis(atoms, "cc-pvdz")
    moved = integrals.Basis([(s, p + d) for s, p in atoms], "cc-pvdz")
    s_mat = integrals.one_electron_native(bs)[0]
    np.testing.assert_allclose(integrals.dipole_native(moved), integrals.dipole_native(bs) + d[:, None, None] * s_mat,
                               rtol=0, atol=1e-12)


def test_native_dipole_rejects_bad_shells():
    import ctypes

    from nbed_amd import _nbx

    lib = _nbx.load_library()
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = np.zeros(3)
    one = np.ones(1)
    args = lambda ang, nfunc: (1, ptr(i32(ang)), ptr(i32(1)), ptr(i32(nfunc)), ptr(np.zeros(3)), ptr(one), ptr(one),  # noqa: E731
                               ptr(np.ones(100)), 1, ptr(out))
    assert lib.nbx_host_dipole(*args(4, 9)) == -1
    assert lib.nbx_host_dipole(*args(2, 4)) == -1
    assert lib.nbx_host_dipole(*args(0, 1)) == 0


# ---------------------------------------------------------------------------------------------- the restatement
def test_angle_and_gain_match_a_brute_force_scan():
    rng = np.random.default_rng(3)
    grid = np.linspace(-np.pi / 4, np.pi / 4, 400001)
    c, s = np.cos(grid), np.sin(grid)
    for nk in (1, 3, 7):
        q = rng.normal(size=(nk, 2, 2))
        q = q + q.transpose(0, 2, 1)
        f = 0.0
        for k in range(nk):
            ss = c * c * q[k, 0, 0] + s * s * q[k, 1, 1] + 2 * c * s * q[k, 0, 1]
            tt = s * s * q[k, 0, 0] + c * c * q[k, 1, 1] - 2 * c * s * q[k, 0, 1]
            f = f + ss * ss + tt * tt
        f0 = float(np.sum(q[:, 0, 0] ** 2 + q[:, 1, 1] ** 2))
        a, b, p = ref.pair_terms(q[:, 0, 0][:, None], q[:, 1, 1][:, None], q[:, 0, 1][:, None])
        assert abs(ref.gains(a, b)[0] - (f.max() - f0)) < 1e-8 * f.max()
        cg, sg, _ = ref.angles(a, b, p)
        gamma = np.arctan2(sg[0], cg[0])
        assert abs(gamma - grid[np.argmax(f)]) < 1e-4


@pytest.mark.parametrize("kind", ["pm", "pm_xy", "boys"])
def test_restatement_increases_f_and_ends_stationary(kind):
    rng = np.random.default_rng({"pm": 1, "pm_xy": 2, "boys": 3}[kind])
    n, nao = 9, 30
    x = np.linalg.qr(rng.normal(size=(nao, n)))[0]
    hist = []
    if kind == "boys":
        r = rng.normal(size=(3, nao, nao))
        r = r + r.transpose(0, 2, 1)
        u, sweeps, f, conv = ref.localize_boys(ref.boys_matrices(x, r), history=hist)
        q = ref.boys_matrices(x @ u, r)
    else:
        offs = [0, 4, 9, 15, 22, 30]
        y = None if kind == "pm" else x @ np.diag(rng.uniform(0.5, 1.5, n))
        u, sweeps, f, conv = ref.localize_pm(x, y, offs, history=hist)
        q = ref.pm_matrices(x @ u, (x if y is None else y) @ u, offs)
    assert conv and sweeps == len(hist)
    assert np.all(np.diff(hist) >= -1e-12 * f)
    np.testing.assert_allclose(u.T @ u, np.eye(n), rtol=0, atol=1e-13)
    assert abs(ref.functional(q) - f) < 1e-12 * f
    assert ref.all_pair_gains(q).max() <= 1e-12 * f


# ---------------------------------------------------------------------------------------------- host bookkeeping
class _Scf:
    def __init__(self, c, occ, mol, s):
        self.mo_coeff, self.mo_occ, self.mol, self._s = c, occ, mol, s

    def get_ovlp(self):
        return self._s


class IdentityBackend(LocCheckerBackend):
    """The rotation is the identity: C_loc = C_occ, so a test chooses the active shares itself."""

    def localize_boys(self, q, max_sweeps=1000, tol=1e-10):
        b, n = q.shape[0], q.shape[-1]
        return self.asarray(np.broadcast_to(np.eye(n), (b, n, n))), np.zeros(b, int), np.zeros(b)


def _scf_with_shares(shares, nao=4):
    """Restricted SCF whose occupied orbitals have the given weights on the active AOs [0, 2)."""
    c = np.zeros((nao, nao))
    for j, w in enumerate(shares):
        c[0, j], c[2, j] = np.sqrt(w), np.sqrt(1 - w)
    mol = Mole(nao, (len(shares), len(shares)), ao_slices=[[0, 1, 0, 2], [1, 2, 2, nao]],
               dipole=lambda: np.zeros((3, nao, nao)))
    occ = np.array([2.0] * len(shares) + [0.0] * (nao - len(shares)))
    return _Scf(c, occ, mol, np.eye(nao))


def test_selection_edge_cases():
    be = IdentityBackend()
    # every share the same: half and half
    ls = BOYSLocalizer(_scf_with_shares([0.5, 0.5, 0.5]), 1, backend=be).localize()
    assert list(ls.active_mo_inds) == [0] and list(ls.enviro_mo_inds) == [1, 2]
    # nothing above the cutoff: the largest share is forced active
    loc = BOYSLocalizer(_scf_with_shares([0.3, 0.6, 0.1]), 1, occ_cutoff=0.95, backend=be)
    ls = loc.localize()
    assert list(ls.active_mo_inds) == [1] and list(ls.enviro_mo_inds) == [0, 2]
    np.testing.assert_allclose(loc.enviro_selection_condition, [0.3, 0.6, 0.1], rtol=0, atol=1e-15)
    # no environment: a zero column stands in for it
    ls = BOYSLocalizer(_scf_with_shares([0.99, 0.97]), 1, occ_cutoff=0.9, backend=be).localize()
    assert list(ls.active_mo_inds) == [0, 1] and len(ls.enviro_mo_inds) == 0
    assert ls.c_enviro.shape == (4, 1) and not ls.c_enviro.any()


@pytest.mark.parametrize("cls", [PMLocalizer, BOYSLocalizer])
def test_arguments(cls):
    """Port of the reference's test_PM_arguments (tests/test_localizers.py:61-93) to both classes."""
    scf = _scf_with_shares([0.3, 0.6])
    kw = {"pop_method": "mulliken"} if cls is PMLocalizer else {}
    for occ, virt in ((1.1, 0.95), (0.95, 1.1), (-0.1, 0.95), (0.95, -0.1)):
        with pytest.raises(ValueError):
            cls(scf, n_active_atoms=1, occ_cutoff=occ, virt_cutoff=virt, backend=LocCheckerBackend(), **kw).localize()
    loc = cls(scf, n_active_atoms=1, backend=LocCheckerBackend(), **kw)
    with pytest.raises(NotImplementedError, match="Virtual orbital localization"):
        loc.localize_virtual(scf)
    with pytest.raises(ValueError, match="pop_method"):
        PMLocalizer(scf, 1, pop_method="iao", backend=LocCheckerBackend())


def test_meta_lowdin_needs_pyscf_or_pop_ao():
    scf = _scf_with_shares([0.3, 0.6])
    with pytest.raises(NotImplementedError, match="ANO") as err:
        PMLocalizer(scf, 1, backend=LocCheckerBackend())
    assert "mulliken" in str(err.value) and "lowdin" in str(err.value)
    # with the orthogonal AOs given, 'meta-lowdin' runs: identity AOs on an orthonormal basis = Mulliken
    a = PMLocalizer(scf, 1, pop_ao=np.eye(4), backend=LocCheckerBackend()).localize()
    b = PMLocalizer(scf, 1, pop_method="mulliken", backend=LocCheckerBackend()).localize()
    np.testing.assert_allclose(a.c_loc_occ, b.c_loc_occ, rtol=0, atol=1e-12)
    with pytest.raises(NotImplementedError):
        IBOLocalizer(scf, 1)


def test_driver_boys_needs_dipole_integrals():
    with pytest.raises(NotImplementedError, match="dipole integrals"):
        nbed(NbedConfig(geometry=WATER_XYZ, n_active_atoms=1, basis="STO-3G", xc_functional="b3lyp", localization="boys",
                        virtual_localization="disable"),
             provider=SyntheticProvider(14, (5, 5), 5), backend=LocCheckerBackend())
    with pytest.raises(NotImplementedError, match="dipole integrals"):
        Mole(4, (1, 1)).intor_symmetric("int1e_r", comp=3)
