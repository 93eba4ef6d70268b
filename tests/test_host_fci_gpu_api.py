"""The host side of the device FCI (nbed_amd/fci_gpu.py) that needs no GPU: import, the memory plan, string ranks and
link tables against brute force, the independent reference of tests/fci_reference.py against the host solver, and the
driver's routing between the two solvers."""

import itertools
from math import comb

import numpy as np
import pytest

import fci_reference as ref
from oracle_backend import OracleBackend
from synthetic_provider import SyntheticProvider
from test_host_driver import config

from nbed_amd import fci, fci_gpu, nbed
from nbed_amd.exceptions import NbedDriverError


def test_imports_without_a_gpu_and_refuses_a_host_backend():
    assert callable(fci_gpu.solve) and callable(fci_gpu.solve_spatial) and callable(fci_gpu.sigma)
    spatial = (0.0, np.zeros((2, 2, 2)), np.zeros((3, 2, 2, 2, 2)))
    with pytest.raises(NbedDriverError, match="HipBackend"):
        fci_gpu.solve_spatial(spatial, (1, 1), backend=OracleBackend())
    with pytest.raises(NbedDriverError, match="HipBackend"):
        fci_gpu.sigma(spatial, (1, 1), np.zeros((2, 2)), backend=OracleBackend())


@pytest.mark.parametrize("n,na,nb,space", [(13, 5, 5, 12), (16, 8, 8, 12), (7, 5, 2, 6)])
def test_memory_plan_is_the_sum_of_its_parts(n, na, nb, space):
    n_a, n_b = comb(n, na), comb(n, nb)
    ndet, g = n_a * n_b, 2 * n * n
    plan = fci_gpu.memory_plan(n, na, nb, space=space)
    assert plan["ndet"] == ndet
    assert plan["vectors"] == 8 * 2 * space * ndet
    assert plan["work"] == 8 * (3 + 2) * ndet
    assert plan["tables"] == 4 * (n_a * n * n + n * n * n_b + n_a + n_b)
    assert plan["hamiltonian"] == 8 * (3 * n**4 + 2 * n * n + g * (g + 1))
    assert plan["chunk"] == 8 * ((g + 1) + g) * plan["chunk_rows"] * n_b
    assert plan["total"] == sum(plan[k] for k in ("vectors", "work", "tables", "hamiltonian", "chunk"))
    assert plan["chunks"] == -(-n_a // plan["chunk_rows"])
    forced = fci_gpu.memory_plan(n, na, nb, space=space, chunk_rows=1)
    assert forced["chunks"] == n_a and forced["chunk"] == 8 * (2 * g + 1) * n_b
    with pytest.raises(ValueError, match="chunk_rows"):
        fci_gpu.memory_plan(n, na, nb, chunk_rows=n_a + 1)


def test_memory_plan_chunks_the_largest_sector_and_not_the_typical_one():
    big = fci_gpu.memory_plan(16, 8, 8, capacity=288 * 10**9)  # 1.66e8 determinants: D + E of all of them are 1.36 TB
    assert big["chunks"] > 1 and big["total"] <= 288 * 10**9
    assert big["chunk_rows"] * comb(16, 8) < 2**31
    typical = fci_gpu.memory_plan(13, 5, 5, capacity=288 * 10**9)  # water / 6-31G: 1.66e6 determinants, 9 GB of D + E
    assert typical["chunks"] == 1 and typical["chunk_rows"] == comb(13, 5) and typical["total"] < 12 * 10**9


def _apply(mask, p, q):
    """a+_p a_q on a string, signs by counting bits: (sign, mask') or (0, 0)."""
    if not (mask >> q) & 1:
        return 0, 0
    sign = -1 if bin(mask & ((1 << q) - 1)).count("1") & 1 else 1
    mask &= ~(1 << q)
    if (mask >> p) & 1:
        return 0, 0
    if bin(mask & ((1 << p) - 1)).count("1") & 1:
        sign = -sign
    return sign, mask | (1 << p)


@pytest.mark.parametrize("n,k", [(1, 1), (4, 0), (4, 4), (6, 3), (9, 4)])
def test_string_ranks_and_link_tables_match_brute_force(n, k):
    combos = list(itertools.combinations(range(n), k))
    masks = fci_gpu.strings(n, k)
    assert masks.tolist() == [sum(1 << p for p in occ) for occ in combos] and masks.size == comb(n, k)
    assert [fci_gpu.string_rank(n, occ) for occ in combos] == list(range(len(combos)))
    rank = {int(m): i for i, m in enumerate(masks)}
    table = fci_gpu.link_table(n, k)
    assert table.shape == (len(combos), n * n) and table.dtype == np.int32
    want = np.zeros_like(table)
    for i, m in enumerate(masks):
        for p in range(n):
            for q in range(n):
                sign, new = _apply(int(m), p, q)
                if sign:
                    want[i, p * n + q] = sign * (rank[new] + 1)
    assert np.array_equal(table, want)
    assert np.all(np.count_nonzero(table, axis=1) == k * (n - k + 1))


@pytest.mark.parametrize("n,na,nb", [(4, 2, 2), (5, 3, 2)])
def test_reference_matrix_reproduces_the_host_solver(n, na, nb):
    ham = ref.synthetic(n, 40 + n)
    assert not np.allclose(ham.one_body[0], ham.one_body[1]) and not np.allclose(ham.two_body[0], ham.two_body[1])
    mat = ref.dense(ham, (na, nb))
    assert np.max(np.abs(mat - mat.T)) < 1e-14
    host = fci.ground_state(*ham.to_dense(), (na, nb), nroots=2)
    assert np.max(np.abs(np.linalg.eigvalsh(mat)[:2] - host.energies)) < 1e-12
    # the same matrix up to the sign per determinant between the two orderings of the creators
    signs = fci_gpu.interleave_signs(n, na, nb).ravel()
    c = host.ci[:, 0] * signs
    assert np.max(np.abs(mat @ c - host.energies[0] * c)) < 1e-12


def test_host_only_backend_still_raises_past_the_cap(monkeypatch):
    monkeypatch.delenv("NBED_FCI_SOLVER", raising=False)
    try:
        import pyscf  # noqa: F401

        pytest.skip("PySCF installed: its FCI runs")
    except ImportError:
        pass
    assert 2 * 24 > fci.MAX_SPIN_ORBITALS
    for mode in (None, "device", "host"):
        if mode:
            monkeypatch.setenv("NBED_FCI_SOLVER", mode)
        with pytest.raises(NbedDriverError, match="PySCF"):
            nbed(config(run_fci_emb=True, virtual_localization="disable"), provider=SyntheticProvider(24, (5, 5), 5),
                 backend=OracleBackend())


def test_unknown_solver_switch_is_refused(monkeypatch):
    monkeypatch.setenv("NBED_FCI_SOLVER", "gpu")
    with pytest.raises(NbedDriverError, match="NBED_FCI_SOLVER='gpu'.*'auto', 'host' or 'device'"):
        nbed(config(run_fci_emb=True, virtual_localization="disable"), provider=SyntheticProvider(8, (2, 2), 2),
             backend=OracleBackend())
