"""The device FCI's densities (nbed_amd/fci_gpu.py, csrc/fci_rdm.hip) against tests/fci_rdm_reference.py -- operators
applied to bit masks, independent of the generators, link tables and D the kernels rest on -- for normalised random
vectors, as state densities (b = c) and as transition densities (b != c); the identities that tie the densities to
the existing sigma build; <S^2>; and the methods of the solver objects, alone and through the driver."""

from math import comb

import numpy as np
import pytest

import fci_reference as ref
import fci_rdm_reference as rref

from nbed_amd import NbedConfig, fci_gpu, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.ham_builder import HamiltonianBuilder

pytestmark = pytest.mark.gpu

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
README_WATER = "3\n\nO 0 0 0.115\nH 0 0.754 -0.459\nH 0 -0.754 -0.459"
SECTORS = [(1, 1, 0), (2, 1, 1), (4, 4, 1), (5, 3, 0), (5, 3, 2), (6, 3, 3), (7, 5, 5)]


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@pytest.fixture(scope="module")
def provider(be):
    return BuiltinHFProvider(be)


def unit_vectors(shape, seed):
    """Two normalised random vectors (bra, ket) of a sector."""
    rng = np.random.default_rng(seed)
    b, c = rng.standard_normal(shape), rng.standard_normal(shape)
    return b / np.linalg.norm(b), c / np.linalg.norm(c)


@pytest.fixture(scope="module")
def small():
    """Per small sector: bra, ket and the reference densities of the state (c, c) and the transition (b, c), made once."""
    cache = {}

    def get(sector):
        if sector not in cache:
            n, na, nb = sector
            b, c = unit_vectors((comb(n, na), comb(n, nb)), 1000 * n + 10 * na + nb)
            cache[sector] = (b, c, rref.rdm12(n, (na, nb), c), rref.rdm12(n, (na, nb), c, b))
        return cache[sector]

    return get


def plans(sector):
    """(chunk_rows, slabs): unchunked, one alpha row per chunk, three (a ragged last chunk), with one slab, two, and a
    number that does not divide the chunk's determinants."""
    n, na, nb = sector
    n_a, n_b = comb(n, na), comb(n, nb)
    out = []
    for chunk_rows in (None, 1, 3):
        rows = n_a if chunk_rows is None else min(chunk_rows, n_a)
        odd = next(s for s in range(3, 100) if (rows * n_b) % s)
        out += [(None if chunk_rows is None else rows, slabs) for slabs in (1, 2, odd)]
    return out


def worst(got, want):
    return max(float(np.max(np.abs(g - w))) for g, w in zip(got, want))


# ---------------------------------------------------------------- every element, every plan
@pytest.mark.parametrize("sector", SECTORS)
def test_rdm12_every_element(be, small, sector):
    n, na, nb = sector
    b, c, want_state, want_trans = small(sector)
    ndet = b.size
    for bra, want, label in ((None, want_state, "state"), (b, want_trans, "transition")):
        tol = rref.rdm_tolerance(ndet, c if bra is None else bra, c)
        got = {}
        for plan in plans(sector):
            dm1, dm2 = fci_gpu.rdm12(c, n, (na, nb), bra=bra, backend=be, chunk_rows=plan[0], slabs=plan[1])
            got[plan] = (be.to_host(dm1).copy(), be.to_host(dm2).copy())
            assert got[plan][0].shape == (2, n, n) and got[plan][1].shape == (3, n, n, n, n)
            err = worst(got[plan], want)
            print(f"{sector} {label} chunk_rows={plan[0]} slabs={plan[1]}: max|err| {err:.2e}, bound {tol:.2e}")
            assert np.isfinite(err) and err <= tol
        first = got[plans(sector)[0]]
        assert all(worst(g, first) <= tol for g in got.values())  # across plans
        plan = plans(sector)[-1]
        again = fci_gpu.rdm12(c, n, (na, nb), bra=bra, backend=be, chunk_rows=plan[0], slabs=plan[1])
        assert all(np.array_equal(be.to_host(a), g) for a, g in zip(again, got[plan]))  # the same plan twice: the same bits


@pytest.mark.parametrize("sector", SECTORS)
def test_direct_rdm1(be, small, sector):
    """The kernel without D: against the reference, against the GEMM route, and bit for bit against itself."""
    n, na, nb = sector
    b, c, want_state, want_trans = small(sector)
    for bra, want in ((None, want_state), (b, want_trans)):
        tol = rref.rdm_tolerance(b.size, c if bra is None else bra, c)
        got = be.to_host(fci_gpu.rdm1(c, n, (na, nb), bra=bra, backend=be)).copy()
        via_gemm = be.to_host(fci_gpu.rdm12(c, n, (na, nb), bra=bra, backend=be)[0])
        print(f"{sector}: direct dm1 max|err| {np.max(np.abs(got - want[0])):.2e}, bound {tol:.2e}")
        assert got.shape == (2, n, n) and np.all(np.abs(got - want[0]) <= tol) and np.all(np.abs(got - via_gemm) <= tol)
        assert np.array_equal(be.to_host(fci_gpu.rdm1(c, n, (na, nb), bra=bra, backend=be)), got)


def sampled(rng, n, count):
    return [tuple(int(i) for i in rng.integers(0, n, 4)) for _ in range(count)]


def test_row_longer_than_a_workgroup(be):
    """n = 13 (1, 6): rows of 1716 beta strings (more than a workgroup of 1024 threads), 22 308 determinants."""
    n, nelec = 13, (1, 6)
    sec = ref.Sector(n, nelec)
    assert sec.shape == (13, 1716) and sec.ndet == 22308
    b, c = unit_vectors(sec.shape, 1316)
    tol = rref.rdm_tolerance(sec.ndet, b, c)
    rng = np.random.default_rng(13)
    dm1 = be.to_host(fci_gpu.rdm1(c, n, nelec, bra=b, backend=be))
    gemm1, dm2 = (be.to_host(x) for x in fci_gpu.rdm12(c, n, nelec, bra=b, backend=be))
    assert np.all(np.isfinite(dm1)) and np.all(np.isfinite(dm2)) and np.all(np.abs(dm1 - gemm1) <= tol)
    for spin in range(2):
        pairs = [(p, p) for p in range(n)] + [(0, 1), (n - 1, 0)] + [tuple(int(i) for i in rng.integers(0, n, 2)) for _ in range(8)]
        err = max(abs(dm1[spin, p, q] - rref.dm1_element(sec, c, b, spin, p, q)) for p, q in pairs)
        print(f"n=13 (1,6) dm1 spin {spin}: {len(pairs)} elements, max|err| {err:.2e}, bound {tol:.2e}")
        assert err <= tol
    for x in range(3):
        err = max(abs(dm2[(x, *e)] - rref.dm2_element(sec, c, b, x, *e)) for e in sampled(rng, n, 16))
        print(f"n=13 (1,6) dm2 block {x}: 16 elements, max|err| {err:.2e}, bound {tol:.2e}")
        assert err <= tol


def test_sampled_elements_n9_chunked(be):
    """n = 9 (4, 3), 10 584 determinants, 126 alpha rows cut 50 + 50 + 26."""
    n, nelec = 9, (4, 3)
    sec = ref.Sector(n, nelec)
    assert sec.ndet == 10584 and sec.shape[0] == 126
    b, c = unit_vectors(sec.shape, 943)
    tol = rref.rdm_tolerance(sec.ndet, b, c)
    dm1, dm2 = (be.to_host(x) for x in fci_gpu.rdm12(c, n, nelec, bra=b, backend=be, chunk_rows=50))
    want1 = rref.rdm12(n, nelec, c, b, two_particle=False)[0]
    print(f"n=9 (4,3) chunk_rows=50: dm1 max|err| {np.max(np.abs(dm1 - want1)):.2e}, bound {tol:.2e}")
    assert np.all(np.abs(dm1 - want1) <= tol)
    rng = np.random.default_rng(9)
    for x in range(3):
        err = max(abs(dm2[(x, *e)] - rref.dm2_element(sec, c, b, x, *e)) for e in sampled(rng, n, 32))
        print(f"n=9 (4,3) dm2 block {x}: 32 elements, max|err| {err:.2e}, bound {tol:.2e}")
        assert err <= tol


# ---------------------------------------------------------------- identities
def integrals_norm(ham):
    """1-norm of the integrals as the energy identity weights them (the ab block twice)."""
    two = np.abs(np.asarray(ham.two_body))
    return float(np.abs(np.asarray(ham.one_body)).sum() + two[0].sum() + two[1].sum() + 2.0 * two[2].sum())


def energy_tolerance(ham, nelec, b, c):
    """Every element of dm1 / dm2 within rdm_tolerance, weighted by the integrals; every element of the device sigma
    within sigma_tolerance, weighted by the bra."""
    return (rref.rdm_tolerance(b.size, b, c) * integrals_norm(ham)
            + b.size * np.abs(b).max() * ref.sigma_tolerance(ham, nelec, np.abs(c).max()))


@pytest.mark.parametrize("sector", SECTORS[1:])
def test_identities(be, small, sector):
    n, na, nb = sector
    nelec = (na, nb)
    b, c, _, _ = small(sector)
    ham = ref.synthetic(n, 100 * n + 10 * na + nb)
    sig = be.to_host(fci_gpu.sigma(ham, nelec, c, backend=be))
    for bra in (c, b):
        tol = rref.rdm_tolerance(b.size, bra, c)
        rb = fci_gpu.RdmBuilder(be, n, nelec)
        dm1, dm2, overlap = (be.to_host(x) for x in rb.rdm12(c, None if bra is c else bra))
        assert abs(overlap[0] - np.vdot(bra, c)) <= tol
        # <b|H|c> from the densities and from the sigma build; <b|c> and the dot product in numpy
        e_rdm = fci_gpu.energy_from_rdm(ham, dm1, dm2, overlap=float(np.vdot(bra, c)))
        e_sig = float(np.vdot(bra, sig))
        print(f"{sector}: <b|H|c> densities {e_rdm:.15f} sigma {e_sig:.15f} bound {energy_tolerance(ham, nelec, bra, c):.2e}")
        assert abs(e_rdm - e_sig) <= energy_tolerance(ham, nelec, bra, c)
        # traces: sum_pq <b| a+_p a+_q a_q a_p |c> = N_s (N_s - 1) <b|c>, N_a N_b <b|c>  (n^2 elements, and <b|c> in numpy)
        counts = (na * (na - 1), nb * (nb - 1), na * nb)
        for x in range(3):
            assert abs(np.einsum("pqqp->", dm2[x]) - counts[x] * np.vdot(bra, c)) <= 2 * n * n * tol
        # sum_q <b| a+_p a+_q a_q a_s |c> = <b| a+_p a_s (N_t - 1 or N_t) |c>  (n elements, and dm1's own error N_t times)
        for x, (spin, factor) in enumerate(((0, na - 1), (1, nb - 1), (0, nb))):
            assert np.all(np.abs(np.einsum("pqqs->ps", dm2[x]) - factor * dm1[spin]) <= (n + abs(factor)) * tol)
        assert np.all(np.abs(np.einsum("pqrp->qr", dm2[2]) - na * dm1[1]) <= (n + na) * tol)


def single_determinant(n, nelec, occ_a, occ_b):
    c = np.zeros((comb(n, nelec[0]), comb(n, nelec[1])))
    c[fci_gpu.string_rank(n, occ_a), fci_gpu.string_rank(n, occ_b)] = 1.0
    return c


def test_spin_square_of_single_determinants(be):
    """Three alpha electrons in orbitals 0-2 and a beta electron in orbital 1: two unpaired alpha spins, S = 1, <S^2> = 2.
    Alpha in orbital 0 and beta in orbital 1: half singlet, half triplet, <S^2> = 1."""
    for n, nelec, occ_a, occ_b, want in ((4, (3, 1), (0, 1, 2), (1,), 2.0), (2, (1, 1), (0,), (1,), 1.0)):
        dm2 = fci_gpu.rdm12(single_determinant(n, nelec, occ_a, occ_b), n, nelec, backend=be)[1]
        assert abs(fci_gpu.spin_square(dm2, nelec) - want) <= 1e-13


# ---------------------------------------------------------------- the solver objects
@pytest.fixture(scope="module")
def water(be, provider):
    """Water / STO-3G: the spatial Hamiltonian and the two lowest roots from the HF determinant."""
    cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="sto-3g", xc_functional="hf", convergence=1e-11)
    hf = provider.global_hf(cfg)
    ham = HamiltonianBuilder(hf, hf.energy_nuc(), backend=be).build_spatial()
    mo_occ = np.asarray(hf.mo_occ)
    if mo_occ.ndim == 1:
        mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
    occupied = [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]
    return ham, fci_gpu.solve_spatial(ham, (5, 5), occupied, conv_tol=1e-10, nroots=2, backend=be)


def test_solver_result_methods_water_sto3g(be, water):
    ham, res = water
    n, nelec, ndet = ham.n, (5, 5), 441
    assert res.converged and res.nelec == nelec
    dm1, dm2 = res.rdm12(0)  # (the device copy of the vectors)
    assert isinstance(dm1, np.ndarray) and dm1.shape == (2, n, n) and dm2.shape == (3, n, n, n, n)
    c = res.ci  # (drops the device copy: everything below uploads the host copy again)
    assert c.shape == (2, 21, 21) and res._ci_dev is None
    # the Ritz value is y^T (V^T H V) y with the subspace matrix from device dot products of length ndet, each within
    # ndet eps |H| of exact, |H| <= |constant| + the 1-norm of the integrals, over a basis of at most 12 vectors
    norm_h = abs(ham.constant) + integrals_norm(ham)
    tol = energy_tolerance(ham, nelec, c[0], c[0]) + 13 * ndet * ref.EPS * norm_h
    e0 = fci_gpu.energy_from_rdm(ham, dm1, dm2, overlap=float(np.vdot(c[0], c[0])))
    print(f"water / STO-3G: E from the densities {e0:.12f}, Ritz value {res.energies[0]:.12f}, bound {tol:.2e}")
    assert abs(e0 - res.energies[0]) <= tol
    again = res.rdm12(0)
    assert np.array_equal(again[0], dm1) and np.array_equal(again[1], dm2)
    assert np.all(np.abs(res.rdm1(0) - dm1) <= rref.rdm_tolerance(ndet, c[0], c[0]))
    # orthogonal roots: tr <0| a+_p a_q |1> = N_s <0|1>
    t1 = res.trans_rdm1(0, 1)
    bound = n * rref.rdm_tolerance(ndet, c[0], c[1]) + 5 * abs(np.vdot(c[0], c[1]))
    assert t1.shape == (2, n, n) and abs(np.trace(t1[0])) <= bound and abs(np.trace(t1[1])) <= bound
    t1b, t2 = res.trans_rdm12(0, 1)
    assert np.all(np.abs(t1b - t1) <= rref.rdm_tolerance(ndet, c[0], c[1])) and t2.shape == dm2.shape
    # the closed-shell ground state is a singlet as far as it is converged
    s2 = res.spin_square(0)
    print(f"water / STO-3G: <S^2> {s2:.3e}, residual {res.residual_norm[0]:.2e}")
    assert abs(s2) <= 10 * res.residual_norm[0]
    occ = res.natural_occupations(0)
    trace_tol = 2 * n * rref.rdm_tolerance(ndet, c[0], c[0]) + 10 * abs(np.vdot(c[0], c[0]) - 1.0) + 10 * ndet * ref.EPS
    assert occ.shape == (n,) and np.all(np.diff(occ) <= 0) and abs(occ.sum() - 10.0) <= trace_tol
    assert np.all(occ <= 2.0 + 1e-12) and np.all(occ >= -1e-12)


def test_driver_hands_out_the_solver_with_densities(be, provider, monkeypatch):
    """The README's water / STO-3G through nbed(): the host and the device solver's objects give the same densities (to
    what the two solvers converge to), and their traces are the embedded electron counts."""
    cfg = NbedConfig(geometry=README_WATER, n_active_atoms=2, basis="STO-3G", xc_functional="hf", projector="huzinaga",
                     convergence=1e-9, run_fci_emb=True)
    got = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("NBED_FCI_SOLVER", mode)
        drv = nbed(cfg, provider=provider, backend=be)
        solver = drv.huzinaga["fci_solver"]
        got[mode] = solver.rdm12(0)
        na, nb = (int(x) for x in drv.embedded_scf.mol.nelec)
    assert isinstance(drv.huzinaga["fci_emb"], float)  # (the energy, as before)
    assert isinstance(solver, fci_gpu.FCIGpuResult)
    for x in range(2):
        print(f"driver: max|dm{x + 1} host - device| {np.max(np.abs(got['host'][x] - got['device'][x])):.2e}")
        assert np.max(np.abs(got["host"][x] - got["device"][x])) <= 1e-8
    dm1, dm2 = got["device"]
    assert abs(np.trace(dm1[0]) - na) <= 1e-8 and abs(np.trace(dm1[1]) - nb) <= 1e-8
    for x, count in enumerate((na * (na - 1), nb * (nb - 1), na * nb)):
        assert abs(np.einsum("pqqp->", dm2[x]) - count) <= 1e-8
