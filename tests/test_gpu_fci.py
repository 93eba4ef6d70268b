"""The device FCI (nbed_amd/fci_gpu.py, csrc/fci.hip) against tests/fci_reference.py -- rows of the Hamiltonian matrix
straight from the operator definition, independent of the generator form the kernels rest on -- against the host
solver nbed_amd/fci.py, against the device CCSD where the two must agree, and through the driver."""

from math import comb

import numpy as np
import pytest

import fci_reference as ref

from nbed_amd import NbedConfig, ccsd_gpu, fci, fci_gpu, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.exceptions import NbedDriverError
from nbed_amd.ham_builder import HamiltonianBuilder

pytestmark = pytest.mark.gpu

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
README_WATER = "3\n\nO 0 0 0.115\nH 0 0.754 -0.459\nH 0 -0.754 -0.459"
H2_WATER = "5\n\nH 0 0 3.0\nH 0 0 3.74\nO 0 0 -0.115\nH 0 0.754 -0.689\nH 0 -0.754 -0.689"  # H2 (0.74 A) 3 A above the oxygen
SMALL = [(2, 1, 1), (4, 4, 1), (5, 3, 0), (5, 3, 2), (6, 3, 3), (7, 5, 5)]


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@pytest.fixture(scope="module")
def provider(be):
    return BuiltinHFProvider(be)


@pytest.fixture(scope="module")
def small():
    """Per small sector: the synthetic Hamiltonian, the dense reference matrix and a random vector, made once."""
    cache = {}

    def get(sector):
        if sector not in cache:
            n, na, nb = sector
            ham = ref.synthetic(n, 100 * n + 10 * na + nb)
            mat = ref.dense(ham, (na, nb))
            cache[sector] = (ham, mat, np.random.default_rng(n + na).standard_normal(mat.shape[0]))
        return cache[sector]

    return get


def occupied_of(scf_obj):
    mo_occ = np.asarray(scf_obj.mo_occ)
    if mo_occ.ndim == 1:
        mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
    return [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]


@pytest.fixture(scope="module")
def molecules(be, provider):
    """Global HF objects and their spatial Hamiltonians, computed once per (geometry, basis)."""
    cache = {}

    def get(geometry, basis):
        if (geometry, basis) not in cache:
            cfg = NbedConfig(geometry=geometry, n_active_atoms=1, basis=basis, xc_functional="hf", convergence=1e-11)
            hf = provider.global_hf(cfg)
            ham = HamiltonianBuilder(hf, hf.energy_nuc(), backend=be).build_spatial()
            cache[(geometry, basis)] = (hf, ham)
        return cache[(geometry, basis)]

    return get


# ---------------------------------------------------------------- sigma and diagonal
@pytest.mark.parametrize("sector", SMALL)
def test_sigma_every_element(be, small, sector):
    """Against dense(ham) @ c: unchunked, one alpha row per chunk, three rows per chunk (a ragged last chunk)."""
    n, na, nb = sector
    ham, mat, c = small(sector)
    want = mat @ c
    tol = ref.sigma_tolerance(ham, (na, nb), np.abs(c).max())
    n_a = comb(n, na)
    got = {}
    for chunk_rows in (None, 1, 3):
        rows = None if chunk_rows is None else min(chunk_rows, n_a)
        got[chunk_rows] = be.to_host(fci_gpu.sigma(ham, (na, nb), c, backend=be, chunk_rows=rows)).ravel().copy()
        err = np.max(np.abs(got[chunk_rows] - want))
        print(f"{sector} chunk_rows={chunk_rows}: max|err| {err:.2e}, bound {tol:.2e}")
        assert got[chunk_rows].shape == want.shape and np.all(np.abs(got[chunk_rows] - want) <= tol)
        again = be.to_host(fci_gpu.sigma(ham, (na, nb), c, backend=be, chunk_rows=rows)).ravel()
        assert np.array_equal(again, got[chunk_rows])  # the same plan twice: the same bits
    assert np.all(np.abs(got[1] - got[None]) <= tol) and np.all(np.abs(got[3] - got[None]) <= tol)


@pytest.mark.parametrize("sector", SMALL)
def test_diagonal(be, small, sector):
    """H_II is a sum of (na + nb)^2 + (na + nb) + 1 terms of at most max|one_body| + 2 max|two_body|."""
    n, na, nb = sector
    ham, mat, _ = small(sector)
    got = be.to_host(fci_gpu.diagonal(ham, (na, nb), backend=be)).ravel()
    scale = np.abs(ham.one_body).max() + 2 * np.abs(ham.two_body).max() + abs(ham.constant)
    assert np.max(np.abs(got - mat.diagonal())) <= ((na + nb) ** 2 + (na + nb) + 1) * ref.EPS * (na + nb + 1) ** 2 * scale


def _check_rows(be, ham, nelec, rows_to_check, chunk_rows, seed):
    sec = ref.Sector(ham.n, nelec)
    c = np.random.default_rng(seed).standard_normal(sec.shape)
    tol = ref.sigma_tolerance(ham, nelec, np.abs(c).max())
    got_dev = fci_gpu.sigma(ham, nelec, c, backend=be, chunk_rows=chunk_rows).view(-1)
    idx = np.asarray(sorted(set(int(i) for i in rows_to_check)), dtype=np.int64)
    got = be.to_host(got_dev[be.torch.from_numpy(idx).to(got_dev.device)])
    worst = 0.0
    for i, g in zip(idx, got):
        worst = max(worst, abs(g - ref.row_dot(ham, nelec, int(i), c, sec)))
    print(f"n={ham.n} {nelec} chunk_rows={chunk_rows}: {idx.size} rows, max|err| {worst:.2e}, bound {tol:.2e}")
    assert np.isfinite(worst) and worst <= tol


def test_sigma_sampled_rows_n9(be):
    ham, nelec = ref.synthetic(9, 943), (4, 3)
    ndet = comb(9, 4) * comb(9, 3)
    rows = list(np.random.default_rng(9).integers(0, ndet, 64)) + [0, ndet - 1]
    _check_rows(be, ham, nelec, rows, None, 1)
    _check_rows(be, ham, nelec, rows, 50, 1)  # 126 alpha rows: 50 + 50 + 26


def test_sigma_sampled_rows_row_longer_than_a_workgroup(be):
    """n = 12 (6, 6): rows of 924 beta strings (more than one workgroup of 256 threads), 924 alpha rows cut 400 + 400 + 124."""
    ham, nelec = ref.synthetic(12, 1266), (6, 6)
    nb_str = comb(12, 6)
    rng = np.random.default_rng(12)
    rows = [0, nb_str * nb_str - 1] + [int(a) * nb_str + int(b) for a, b in zip(rng.integers(0, nb_str, 6), rng.integers(0, nb_str, 6))]
    rows += [399 * nb_str + 923, 400 * nb_str, 800 * nb_str + 255, 800 * nb_str + 256]
    _check_rows(be, ham, nelec, rows, 400, 2)


def test_sigma_sampled_rows_past_32_bit_indices(be):
    """n = 14 (6, 6): 9.0e6 determinants, 2 n^2 Ndet = 3.5e9 elements of D -- the smallest sector where 32-bit index
    arithmetic goes wrong -- in ONE chunk (56 GB of D and E), rows from the first, a middle and the last alpha row."""
    ham, nelec = ref.synthetic(14, 1466), (6, 6)
    ns = comb(14, 6)
    assert 2 * 14 * 14 * ns * ns > 2**31
    rows = [0, 1500, ns - 1, 1501 * ns, 1501 * ns + 1702, 1502 * ns - 1, (ns - 1) * ns, (ns - 1) * ns + 77, ns * ns - 1]
    _check_rows(be, ham, nelec, rows, ns, 3)


# ---------------------------------------------------------------- the solver against the host solver
def _against_host(be, ham, nelec, occupied, label):
    n, (na, nb) = ham.n, nelec
    host = fci.ground_state(*ham.to_dense(), nelec, nroots=2)
    start = fci_gpu.string_rank(n, [i >> 1 for i in occupied if i % 2 == 0]) * comb(n, nb) + fci_gpu.string_rank(
        n, [i >> 1 for i in occupied if i % 2 == 1])
    signs = fci_gpu.interleave_signs(n, na, nb).ravel()
    c_host = host.ci[:, 0] * signs
    dev = fci_gpu.solve_spatial(ham, nelec, occupied, conv_tol=1e-10, backend=be)
    one_row = fci_gpu.solve_spatial(ham, nelec, occupied, conv_tol=1e-10, backend=be, chunk_rows=1)
    overlap = abs(np.dot(dev.ci.ravel(), c_host))
    print(f"{label}: E {dev.e_tot:.12f} host {host.e_tot:.12f} gap {host.energies[1] - host.energies[0]:.3e} "
          f"weight {c_host[start]:.3f} iterations {dev.iterations} residual {dev.residual_norm:.2e} 1-overlap {1 - overlap:.2e} "
          f"chunk_rows=1 dE {one_row.e_tot - dev.e_tot:.2e}")
    assert host.energies[1] - host.energies[0] > 1e-3
    assert abs(c_host[start]) > 0.5
    assert dev.converged and one_row.converged
    assert dev.determinants == host.determinants
    assert abs(dev.e_tot - host.e_tot) < 1e-9
    assert 1.0 - overlap < 1e-12
    assert abs(one_row.e_tot - dev.e_tot) < 1e-12
    return dev


@pytest.mark.parametrize("sector", [(5, 3, 2), (6, 3, 3)])
def test_solver_matches_the_host_solver_synthetic(be, small, sector):
    n, na, nb = sector
    ham, mat, _ = small(sector)
    lowest = int(np.argmin(mat.diagonal()))
    sec = ref.Sector(n, (na, nb))
    mask = sec.mask(lowest)
    occupied = [2 * p for p in range(n) if (mask >> p) & 1] + [2 * p + 1 for p in range(n) if (mask >> (n + p)) & 1]
    dev = _against_host(be, ham, (na, nb), occupied, f"synthetic {sector}")
    # no start determinant given: the lowest diagonal element, the same one
    auto = fci_gpu.solve_spatial(ham, (na, nb), conv_tol=1e-10, backend=be)
    assert auto.converged and abs(auto.e_tot - dev.e_tot) < 1e-12


@pytest.mark.parametrize("space,max_cycle", [(4, 3), (4, 4), (4, 6), (12, 11), (12, 12), (12, 1), (12, 0)])
def test_running_out_of_cycles_returns_the_current_ritz_pair(be, small, space, max_cycle):
    """A tolerance nothing reaches: the result says so and carries the Ritz pair of the basis as it stands -- also when
    the last iteration collapsed the basis (space 4: iterations 3, 6, ...; space 12: iteration 12), and with no
    iteration at all.  Energy and residual belong to the returned vector."""
    ham, mat, _ = small((6, 3, 3))
    dev = fci_gpu.solve_spatial(ham, (3, 3), conv_tol=1e-30, space=space, max_cycle=max_cycle, backend=be)
    assert not dev.converged and dev.iterations == max_cycle
    c = dev.ci.ravel()
    assert c.shape == (400,) and np.all(np.isfinite(c)) and abs(np.linalg.norm(c) - 1.0) < 1e-12
    assert np.isfinite(dev.e_tot) and abs(dev.e_tot - c @ mat @ c) < 1e-11
    assert abs(dev.residual_norm - np.linalg.norm(mat @ c - dev.e_tot * c)) < 1e-11
    assert dev.e_tot >= np.linalg.eigvalsh(mat)[0] - 1e-12
    two = fci_gpu.solve_spatial(ham, (3, 3), conv_tol=1e-30, space=space, max_cycle=max_cycle, nroots=2, backend=be)
    assert not two.converged and two.ci.shape == (2, 20, 20) and np.all(np.isfinite(two.ci)) and two.energies[0] <= two.energies[1]


def test_solver_matches_the_host_solver_water_sto3g(be, molecules):
    hf, ham = molecules(WATER, "sto-3g")
    assert 2 * ham.n == 14
    dev = _against_host(be, ham, (5, 5), occupied_of(hf), "water / STO-3G")
    assert abs(dev.e_tot - (-75.00912605315143)) < 1e-7  # the reference's literal (tests/test_reference_kats.py)


def test_two_electrons_are_exact(be, molecules):
    """H2 / cc-pVDZ, 20 spin orbitals, 100 determinants: FCI = the singlet ground state of the two-particle matrix = CCSD."""
    hf, ham = molecules("2\n\nH 0 0 0\nH 0 0 0.74", "cc-pvdz")
    const, h1, h2 = ham.to_dense()
    assert h1.shape[0] == 20
    dev = fci_gpu.solve_spatial(ham, (1, 1), [0, 1], conv_tol=1e-10, backend=be)
    n = ham.n
    ha = h1[0::2, 0::2]
    v = 2.0 * h2[0::2, 1::2, 1::2, 0::2]
    mat = (np.einsum("pr,qs->pqrs", ha, np.eye(n)) + np.einsum("qs,pr->pqrs", ha, np.eye(n))
           + v.transpose(0, 1, 3, 2)).reshape(n * n, n * n)
    cc = ccsd_gpu.solve(const, h1, h2, [0, 1], conv_tol=1e-12, backend=be)
    exact = np.linalg.eigvalsh(0.5 * (mat + mat.T))[0] + const
    print(f"H2 / cc-pVDZ: FCI {dev.e_tot:.12f} two-particle matrix {exact:.12f} CCSD {cc.e_tot:.12f}")
    assert dev.converged and cc.converged and dev.ci.shape == (10, 10)
    assert abs(dev.e_tot - exact) < 1e-9 and abs(dev.e_tot - cc.e_tot) < 1e-9


def test_past_the_host_cap_water_631g(be, molecules):
    """26 spin orbitals, (5, 5), 1.66e6 determinants: converges from the HF determinant; below HF; below the device CCSD
    by less than 5 mHartree; and the converged vector satisfies the eigen-equation on sampled rows of the independent
    reference, |(H c - E c)_I| <= sigma bound + conv_tol."""
    hf, ham = molecules(WATER, "6-31g")
    assert 2 * ham.n == 26 and 2 * ham.n > fci.MAX_SPIN_ORBITALS
    nelec, occupied = (5, 5), occupied_of(hf)
    stats = {}
    dev = fci_gpu.solve_spatial(ham, nelec, occupied, conv_tol=1e-8, backend=be, stats=stats)
    cc = ccsd_gpu.solve_spatial(ham, occupied, conv_tol=1e-9, backend=be)
    print(f"water / 6-31G: E_HF {hf.e_tot:.10f} E_CCSD {cc.e_tot:.10f} E_FCI {dev.e_tot:.10f} ({dev.iterations} iterations, "
          f"residual {dev.residual_norm:.2e}, {stats['plan']['chunks']} chunk(s))")
    assert stats["ndet"] == comb(13, 5) ** 2 == 1656369
    assert dev.converged and dev.residual_norm < 1e-8 and cc.converged
    assert dev.e_tot < hf.e_tot
    assert 0.0 < cc.e_tot - dev.e_tot < 5e-3
    c = dev.ci
    sec = ref.Sector(ham.n, nelec)
    tol = ref.sigma_tolerance(ham, nelec, np.abs(c).max()) + 1e-8
    sig = fci_gpu.sigma(ham, nelec, c, backend=be).view(-1)
    start = fci_gpu.string_rank(13, range(5)) * sec.shape[1] + fci_gpu.string_rank(13, range(5))
    rows = sorted({start, 0, sec.ndet - 1, *(int(i) for i in np.random.default_rng(26).integers(0, sec.ndet, 5)),
                   *(int(i) for i in np.argsort(-np.abs(c.ravel()))[:3])})
    got = be.to_host(sig[be.torch.from_numpy(np.asarray(rows)).to(sig.device)])
    for i, g in zip(rows, got):
        want = ref.row_dot(ham, nelec, i, c, sec)
        assert abs(g - want) <= tol, (i, g, want)                 # the fresh sigma is the reference's
        assert abs(want - dev.e_tot * c.ravel()[i]) <= tol, (i,)  # and the reference's residual vanishes


# ---------------------------------------------------------------- the driver
@pytest.mark.parametrize("projector", ["mu", "huzinaga"])
def test_driver_device_solver_forced_at_small_size(be, provider, monkeypatch, projector):
    """The README's water / STO-3G: NBED_FCI_SOLVER=device agrees with the default (host) route."""
    cfg = NbedConfig(geometry=README_WATER, n_active_atoms=2, basis="STO-3G", xc_functional="hf", projector=projector,
                     convergence=1e-9, run_fci_emb=True)
    monkeypatch.delenv("NBED_FCI_SOLVER", raising=False)
    host = getattr(nbed(cfg, provider=provider, backend=be), projector)
    monkeypatch.setenv("NBED_FCI_SOLVER", "device")
    dev = getattr(nbed(cfg, provider=provider, backend=be), projector)
    print(f"{projector}: e_fci host route {host['e_fci']:.12f} device route {dev['e_fci']:.12f}")
    assert np.isfinite(host["e_fci"]) and abs(dev["e_fci"] - host["e_fci"]) < 1e-9


def test_driver_runs_embedded_fci_past_the_host_cap(be, provider, monkeypatch):
    """H2 beside a water, 6-31G, the H2 active with one occupied orbital per spin: two active electrons in more than 16
    spin orbitals, where FCI and CCSD are the same number.  The host solver forced is refused past its cap, as before."""
    monkeypatch.delenv("NBED_FCI_SOLVER", raising=False)
    monkeypatch.delenv("NBED_CCSD_SOLVER", raising=False)
    cfg = NbedConfig(geometry=H2_WATER, n_active_atoms=2, basis="6-31G", xc_functional="hf", projector="huzinaga",
                     convergence=1e-9, run_fci_emb=True, run_ccsd_emb=True, n_mo_overwrite=(1, 1))
    drv = nbed(cfg, provider=provider, backend=be)
    emb = drv.embedded_scf
    assert tuple(int(x) for x in emb.mol.nelec) == (1, 1)
    assert 2 * np.asarray(emb.mo_coeff).shape[-1] > fci.MAX_SPIN_ORBITALS
    res = drv.huzinaga
    print(f"H2 + water / 6-31G: e_fci {res['e_fci']:.12f} e_ccsd {res['e_ccsd']:.12f}")
    assert np.isfinite(res["e_fci"]) and abs(res["e_fci"] - res["e_ccsd"]) < 1e-8
    monkeypatch.setenv("NBED_FCI_SOLVER", "host")
    with pytest.raises(NbedDriverError, match="PySCF"):
        nbed(cfg, provider=provider, backend=be)
