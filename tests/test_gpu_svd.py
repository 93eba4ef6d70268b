"""nbx_svd_right on the MI355X, both kernels, against the extended-precision Jacobi reference
(oracle/svd.py) under the contract of tests/svd_cases.py.

Every case names the kernel it runs (svd_lds_kernel or the global-memory svd_jacobi_kernel, by
svd.hip's dispatch rule); the workspace size nbx_svd_worksize asks for confirms it, since only the
LDS path adds a rotation log.  Shapes sit on both sides of each dispatch edge; the matrix classes
are Gaussian, column-graded, clustered and exactly repeated spectra, exact low rank, zero, a zero
column, twin columns and the concentric-localisation shell-0 matrix.  Then: bit-exact scale
invariance, bit-exact repetition, and the two consumers (concentric, SPADE) at sizes that take the
fallback kernel, against the LAPACK-based oracle.
"""

from functools import lru_cache

import numpy as np
import pytest

import svd_cases as sc
from oracle import localize as oloc
from oracle import synth

pytestmark = pytest.mark.gpu

MAX_SWEEPS = {"lds": 40, "fallback": 60}  # SL_MAX_SWEEPS, SVD_MAX_SWEEPS of svd.hip


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@lru_cache(maxsize=None)
def _ref(case):
    return sc.reference(sc.make(*case))


def _svd(be, a):
    s, vt = be.svd_right(be.asarray(np.ascontiguousarray(a)))
    return be.to_host(s), be.to_host(vt), be.last_svd_sweeps


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_svd_contract(be, case):
    kind, m, n = case
    kernel = sc.kernel_for(m, n)
    ws = int(be.lib.nbx_svd_worksize(m, n))
    if kernel == "fallback":
        assert ws == sc.fallback_worksize(m, n)
    else:
        assert ws > sc.fallback_worksize(m, n)
    a = sc.make(*case)
    s, vt, sweeps = _svd(be, a)
    assert 0 < sweeps < MAX_SWEEPS[kernel], sweeps
    sc.check_contract(a, s, vt, _ref(case), sc.case_id(case))
    s2, vt2, sweeps2 = _svd(be, a)  # the same input twice: the same bits
    np.testing.assert_array_equal(s2, s)
    np.testing.assert_array_equal(vt2, vt)
    assert sweeps2 == sweeps


@pytest.mark.parametrize("k", [-500, -200, 200, 500])
@pytest.mark.parametrize("case", [("gauss", 60, 40), ("gauss", 150, 140), ("graded", 90, 60), ("graded", 150, 150)],
                         ids=sc.case_id)
def test_svd_scale_invariance(be, case, k):
    """svd(2^k A) = 2^k svd(A) and the same vt, bit for bit: scaling by a power of two is exact, so an
    implementation that removes the scale before the sweeps computes the same rotations."""
    a = sc.make(*case)
    s0, vt0, _ = _svd(be, a)
    s, vt, sweeps = _svd(be, np.ldexp(a, k))
    assert 0 < sweeps < MAX_SWEEPS[sc.kernel_for(case[1], case[2])], sweeps
    np.testing.assert_array_equal(s, np.ldexp(s0, k))
    np.testing.assert_array_equal(vt, vt0)


# ------------------------------------------------------------------ consumers at fallback sizes
@pytest.mark.parametrize("max_shells", [1, 4])
def test_concentric_fallback_size_matches_reference(be, max_shells):
    """~170 virtuals: the shell-0 SVD is 170 x 170 (fallback kernel).  Tolerances of
    tests/test_host_localizers_ham.py::test_concentric_matches_reference, except for the sigma of the
    later shells: those are sigma of C_tot^T F C_ker, and the shell-0 split of the virtual space into
    span and kernel is only as accurate as the contract's vector bound (svd_cases.py) for the gap
    between sigma_na and the floor, delta = C p eps ||M0||_F / (sigma_na - floor): the kernel's rank
    floor leaves the numerically-zero columns unrotated, so the split carries p eps ||M0||_F / sigma_na
    where LAPACK's carries eps ||M0||_2 / sigma_na.  Their sigma may move by 2 delta ||F|| ||C||^2."""
    from nbed_amd.localizers import ConcentricLocalizer

    nao, nocc, na = 200, 30, 40
    assert sc.kernel_for(nao - nocc, nao - nocc) == "fallback"
    s = synth.overlap(nao)
    _, c = synth.lowdin_orthonormal(s, synth.hcore(nao))
    # O(1) like the golden case's Fock matrix, so that its absolute tolerances mean the same here
    fock = 0.05 * (synth.hcore(nao) + 0.1 * synth.sym_matrix(synth.STREAM_MISC, nao))
    occ = np.zeros(nao)
    occ[:nocc] = 1
    cl = ConcentricLocalizer(None, 1, max_shells=max_shells, backend=be)
    cl.projected_overlap, cl.overlap_two_basis, cl.n_act_proj_aos = s[:na, :na], s[:na, :], na
    got, shells, svals = cl._localize_virtual_spin(occ, c, fock)
    ref, rshells, rsvals = oloc.concentric_localize_spin(occ, c, fock, s[:na, :na], s[:na, :], na, max_shells)
    np.testing.assert_array_equal(shells, rshells)
    assert len(svals) == len(rsvals)
    sab_c = s[:na, :] @ c[:, nocc:]
    m0 = np.linalg.solve(s[:na, :na], sab_c).T @ sab_c
    p, fro0 = m0.shape[0], np.linalg.norm(m0)
    floor0 = p * sc.EPS * fro0
    delta = sc.C_BOUND * p * sc.EPS * fro0 / (rsvals[0][na - 1] - floor0)
    later = 1e-11 + 2 * delta * np.linalg.norm(fock, 2) * np.linalg.norm(c, 2) ** 2
    for i, (x, y) in enumerate(zip(svals, rsvals)):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-11 if i == 0 else later)
    edges = [nocc] + list(shells)
    for lo, hi in zip(edges[:-1], edges[1:]):
        np.testing.assert_allclose(got[:, lo:hi] @ got[:, lo:hi].T, ref[:, lo:hi] @ ref[:, lo:hi].T, rtol=0,
                                   atol=1e-9)


SPADE_SEED = synth.SEED + 3  # largest gap 4.2e-3 of the sigma, runner-up 1.1e-3


def test_spade_fallback_size_matches_reference(be):
    """n_act_aos x n_occ = 150 x 140 (fallback kernel) against the LAPACK-based oracle."""
    from nbed_amd.localizers import SPADELocalizer
    from nbed_amd.scf import GpuUHF, Mole

    nao, nocc, n_act_aos = 200, 140, 150
    assert sc.kernel_for(n_act_aos, nocc) == "fallback"
    s = synth.overlap(nao, SPADE_SEED)
    h = synth.hcore(nao, SPADE_SEED)
    _, c = synth.lowdin_orthonormal(s, h)
    occ = np.zeros((2, nao))
    occ[:, :nocc] = 1
    mf = GpuUHF(Mole(nao, (nocc, nocc), ao_slices=[[0, 1, 0, n_act_aos], [1, 2, n_act_aos, nao]]), s, h, None,
                backend=be)
    mf.mo_coeff, mf.mo_occ = np.stack([c, c]), occ
    ls_ref, cond_ref = oloc.spade_localize(mf.mo_coeff, occ, s, n_act_aos)
    diffs = np.sort(cond_ref[0][:-1] - cond_ref[0][1:])[::-1]
    assert diffs[0] - diffs[1] > 1e-8, diffs[:2]  # the partition is decided by a clear largest gap
    loc = SPADELocalizer(mf, 1, backend=be)
    ls = loc.localize()
    np.testing.assert_array_equal(ls.active_mo_inds, ls_ref.active_mo_inds)
    np.testing.assert_array_equal(ls.enviro_mo_inds, ls_ref.enviro_mo_inds)
    np.testing.assert_allclose(loc.enviro_selection_condition[0], cond_ref[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(loc.enviro_selection_condition[1], cond_ref[1], rtol=0, atol=1e-12)
    for k in ("dm_active", "dm_enviro", "dm_loc_occ"):
        np.testing.assert_allclose(getattr(ls, k), getattr(ls_ref, k), rtol=0, atol=1e-10)
