"""The (T) correction of the host CCSD (nbed_amd/ccsd.py: ``triples_correction``, ``solve(triples=True)``), its switch in the
driver and the memory plan of the device path -- no GPU.

The formula is checked against FCI by its perturbation order, which does not depend on the oracle's own algebra; the
semicanonical rotation by invariance under rotations of the occupied and of the virtual spin orbitals."""

import numpy as np
import pytest
from oracle_backend import OracleBackend
from synthetic_provider import SyntheticProvider

from nbed_amd import NbedConfig, ccsd, ccsd_gpu, fci, nbed
from nbed_amd.exceptions import NbedDriverError
from nbed_amd.ham_builder import HamiltonianBuilder

GEOM = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"


def model_hamiltonian(n: int, lam: float, seed: int):
    """n spatial orbitals, eps_p = p + 0.1 normal, h = diag(eps) + 0.2 lam (symmetric normal),
    (pq|rs) = 0.3 lam sum_{L<4} B_L[pq] B_L[rs]; spin-orbital h2[P,R,S,Q] = 1/2 (pq|rs), alpha on the even indices."""
    rng = np.random.default_rng(seed)
    eps = np.arange(n) + 0.1 * rng.standard_normal(n)
    a = rng.standard_normal((n, n))
    b = rng.standard_normal((4, n, n))
    a, b = 0.5 * (a + a.T), 0.5 * (b + b.transpose(0, 2, 1))
    h = np.diag(eps) + 0.2 * lam * a
    eri = 0.3 * lam * np.einsum("Lpq,Lrs->pqrs", b, b)
    h1, h2 = np.zeros((2 * n, 2 * n)), np.zeros((2 * n,) * 4)
    for s in (0, 1):
        h1[s::2, s::2] = h
        for t in (0, 1):
            h2[s::2, t::2, t::2, s::2] = 0.5 * eri.transpose(0, 2, 3, 1)
    return h1, h2


def lowest(nelec):
    return [2 * i for i in range(nelec[0])] + [2 * i + 1 for i in range(nelec[1])]


# ---------------------------------------------------------------- the formula: perturbation order against FCI
@pytest.mark.parametrize("n, nelec, seed", [(5, (2, 2), 1), (5, (2, 2), 2), (6, (3, 2), 1), (6, (3, 2), 2)])
def test_ccsd_t_is_exact_through_fourth_order(n, nelec, seed):
    """CCSD(T) is exact through fourth order, the f_ov terms of a non-HF reference included, so halving lambda divides
    |E_FCI - E_CCSD(T)| by about 2^5; CCSD alone, or (T) without any one of its fourth-order pieces, gives about 2^4.
    The bound of 24 lies above the log-midpoint 22.6 of 16 and 32.

    Measured between lambda = 0.025 and 0.0125 (CCSD converged to 1e-13), cases in the order of the parameters:
        CCSD(T)                           27.0, 29.9, 31.2, 29.4
        CCSD alone                        14.9, 15.4, 17.7, 15.2
        (T) without the f_ia t_jk^bc term 16.9, 14.6, 15.0, 16.1"""
    gaps, gaps_ccsd = [], []
    for lam in (0.025, 0.0125):
        h1, h2 = model_hamiltonian(n, lam, seed)
        cc = ccsd.solve(0.0, h1, h2, lowest(nelec), conv_tol=1e-13, triples=True)
        assert cc.converged
        assert cc.e_tot_t == cc.e_tot + cc.e_t
        e_fci = fci.ground_state(0.0, h1, h2, nelec).e_tot
        gaps.append(abs(e_fci - cc.e_tot_t))
        gaps_ccsd.append(abs(e_fci - cc.e_tot))
    print(f"n={n} nelec={nelec} seed={seed}: CCSD(T) ratio {gaps[0] / gaps[1]:.1f}, CCSD ratio {gaps_ccsd[0] / gaps_ccsd[1]:.1f}")
    assert gaps[0] / gaps[1] >= 24.0
    assert gaps_ccsd[0] / gaps_ccsd[1] < 20.0  # (the test can tell the orders apart)


# ---------------------------------------------------------------- the semicanonical rotation: invariance
def spin_preserving_rotation(nso, occupied, rng):
    """Random orthogonal matrix that mixes occupied alpha with occupied alpha, ..., virtual beta with virtual beta."""
    occ = set(occupied)
    u = np.zeros((nso, nso))
    for s in (0, 1):
        for group in ([p for p in range(s, nso, 2) if p in occ], [p for p in range(s, nso, 2) if p not in occ]):
            if group:
                q, _ = np.linalg.qr(rng.standard_normal((len(group), len(group))))
                u[np.ix_(group, group)] = q
    return u


def relabelled(h1, h2, occupied_from, occupied_to):
    """The same Hamiltonian with its spin orbitals renamed so that the determinant ``occupied_from`` becomes
    ``occupied_to`` (spins kept: even stays even)."""
    nso = h1.shape[0]
    perm = np.full(nso, -1)
    for s in (0, 1):
        src = [p for p in occupied_from if p % 2 == s] + [p for p in range(s, nso, 2) if p not in occupied_from]
        dst = [p for p in occupied_to if p % 2 == s] + [p for p in range(s, nso, 2) if p not in occupied_to]
        perm[dst] = src
    return h1[np.ix_(perm, perm)], h2[np.ix_(perm, perm, perm, perm)]


@pytest.mark.parametrize("case", ["open-shell", "occupied-not-leading"])
def test_triples_are_invariant_under_occupied_and_virtual_rotations(case):
    """lambda = 0.3 (E_T ~ 1e-3).  Rotating the occupied and the virtual spin orbitals by random spin-preserving
    orthogonal matrices leaves the determinant, E_corr and -- with the semicanonical rotation -- E_T unchanged:
    |dE_T| < 1e-10.  With the diagonal of the unrotated Fock matrix as denominators E_T would move by 3e-5 to 2e-3."""
    if case == "open-shell":
        h1, h2 = model_hamiltonian(6, 0.3, 4)
        occupied = lowest((3, 2))
    else:
        h1, h2 = model_hamiltonian(6, 0.3, 7)
        occupied = [0, 1, 4, 7, 9]
        h1, h2 = relabelled(h1, h2, lowest((2, 3)), occupied)
    first = ccsd.solve(0.0, h1, h2, occupied, conv_tol=1e-13, triples=True)
    u = spin_preserving_rotation(12, occupied, np.random.default_rng(9))
    assert np.abs(u - np.diag(np.diag(u))).max() > 0.1
    h1r = u.T @ h1 @ u
    h2r = np.einsum("abcd,ap,bq,cr,ds->pqrs", h2, u, u, u, u, optimize=True)
    second = ccsd.solve(0.0, h1r, h2r, occupied, conv_tol=1e-13, triples=True)
    print(f"{case}: E_corr {first.e_corr:.12f} / {second.e_corr:.12f}, E_T {first.e_t:.3e}, "
          f"dE_T {abs(first.e_t - second.e_t):.1e}")
    assert first.converged and second.converged
    assert abs(first.e_t) > 1e-5
    assert abs(first.e_corr - second.e_corr) < 1e-10
    assert abs(first.e_t - second.e_t) < 1e-10
    # the amplitudes of the rotated problem give the same number when handed over directly
    assert ccsd.triples_correction(h1r, h2r, occupied, second.t1, second.t2) == second.e_t


# ---------------------------------------------------------------- edge cases
def test_no_triples_means_zero():
    h1, h2 = model_hamiltonian(4, 0.3, 5)
    two = ccsd.solve(0.0, h1, h2, [0, 1], conv_tol=1e-12, triples=True)  # two electrons: CCSD is exact
    assert two.e_t == 0.0 and two.e_tot_t == two.e_tot
    assert abs(two.e_tot - fci.ground_state(0.0, h1, h2, (1, 1)).e_tot) < 1e-9
    h1, h2 = model_hamiltonian(3, 0.3, 5)
    few_virtuals = ccsd.solve(0.0, h1, h2, lowest((2, 2)), conv_tol=1e-12, triples=True)  # o = 4, v = 2
    assert few_virtuals.e_t == 0.0
    few_occupied = ccsd.solve(0.0, h1, h2, lowest((1, 1)), conv_tol=1e-12, triples=True)  # o = 2, v = 4
    assert few_occupied.e_t == 0.0
    assert ccsd.triples_correction(h1, h2, [0, 1], few_occupied.t1, few_occupied.t2) == 0.0


def test_triples_are_off_by_default():
    h1, h2 = model_hamiltonian(4, 0.1, 6)
    plain = ccsd.solve(0.0, h1, h2, lowest((2, 1)))
    assert plain.e_t is None and plain.e_tot_t is None
    asked = ccsd.solve(0.0, h1, h2, lowest((2, 1)), triples=True)
    assert abs(asked.e_t) > 1e-8 and asked.e_tot == plain.e_tot and np.array_equal(asked.t2, plain.t2)


def test_absolute_sum_bounds_the_signed_one():
    """``triples_sum(absolute=True)`` -- the S of the device tests' rounding bound -- dominates the signed sum."""
    rng = np.random.default_rng(12)
    blocks = random_blocks(rng, 4, 5)
    sc = ccsd.semicanonical_blocks(**blocks)
    assert abs(ccsd.triples_sum(sc)) <= ccsd.triples_sum(sc, absolute=True)


def random_blocks(rng, no, nv):
    """Random operands of (T) with the right antisymmetry, a non-diagonal Fock matrix and f_ov != 0."""
    def anti(x, pairs):
        for p, q in pairs:
            perm = list(range(x.ndim))
            perm[p], perm[q] = q, p
            x = x - x.transpose(perm)
        return x

    occ_spins, vir_spins = np.arange(no) % 2, (np.arange(nv) + 1) % 2
    foo = np.diag(-2.0 - rng.random(no)) + 0.1 * rng.standard_normal((no, no))
    fvv = np.diag(1.0 + rng.random(nv)) + 0.1 * rng.standard_normal((nv, nv))
    foo[np.not_equal.outer(occ_spins, occ_spins)] = 0.0
    fvv[np.not_equal.outer(vir_spins, vir_spins)] = 0.0
    return {
        "t1": rng.standard_normal((no, nv)), "fov": rng.standard_normal((no, nv)),
        "t2": anti(rng.standard_normal((no, no, nv, nv)), [(0, 1), (2, 3)]),
        "foo": 0.5 * (foo + foo.T), "fvv": 0.5 * (fvv + fvv.T),
        "oovv": anti(rng.standard_normal((no, no, nv, nv)), [(0, 1), (2, 3)]),
        "ovvv": anti(rng.standard_normal((no, nv, nv, nv)), [(2, 3)]),
        "ovoo": anti(rng.standard_normal((no, nv, no, no)), [(2, 3)]),
        "occ_spins": occ_spins, "vir_spins": vir_spins,
    }


# ---------------------------------------------------------------- the driver
def config(**kw):
    base = dict(geometry=GEOM, n_active_atoms=1, basis="synthetic", xc_functional="none", convergence=1e-9,
                max_hf_cycles=80, run_ccsd_emb=True, virtual_localization="disable")
    base.update(kw)
    return NbedConfig(**base)


def occupied_of(scf_obj):
    mo_occ = np.asarray(scf_obj.mo_occ)
    if mo_occ.ndim == 1:
        mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
    return [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]


def needs_no_pyscf():
    try:
        import pyscf  # noqa: F401
    except ImportError:
        return
    pytest.skip("PySCF's own solver would run instead of nbed_amd.ccsd")


def test_driver_reports_ccsd_t_only_when_asked(monkeypatch):
    needs_no_pyscf()
    be = OracleBackend()
    monkeypatch.delenv("NBED_CCSD_TRIPLES", raising=False)
    monkeypatch.delenv("NBED_CCSD_SOLVER", raising=False)
    plain = nbed(config(), provider=SyntheticProvider(14, (5, 5), 5), backend=be)
    res0 = plain.mu if plain.mu is not None else plain.huzinaga
    assert "e_ccsd" in res0 and "e_ccsd_t" not in res0 and "ccsd_t_emb" not in res0

    monkeypatch.setenv("NBED_CCSD_TRIPLES", "1")
    drv = nbed(config(), provider=SyntheticProvider(14, (5, 5), 5), backend=be)
    res = drv.mu if drv.mu is not None else drv.huzinaga
    emb = drv.embedded_scf
    cc, _ = drv._run_emb_ccsd(emb)
    const, h1, h2 = HamiltonianBuilder(emb, emb.energy_nuc(), backend=be).build()
    want = ccsd.triples_correction(h1, h2, occupied_of(emb), cc.t1, cc.t2)
    assert abs(want) > 1e-8
    assert abs((res["e_ccsd_t"] - res["e_ccsd"]) - want) < 1e-10
    assert abs((res["ccsd_t_emb"] - res["ccsd_emb"]) - want) < 1e-10
    assert abs(res["e_ccsd"] - res0["e_ccsd"]) < 1e-12  # the switch leaves CCSD itself alone

    # the argument wins over the environment, either way
    monkeypatch.setenv("NBED_CCSD_TRIPLES", "0")
    on = nbed(config(), provider=SyntheticProvider(14, (5, 5), 5), backend=be, ccsd_triples=True)
    assert abs((on.mu if on.mu is not None else on.huzinaga)["e_ccsd_t"] - res["e_ccsd_t"]) < 1e-10
    monkeypatch.setenv("NBED_CCSD_TRIPLES", "1")
    off = nbed(config(), provider=SyntheticProvider(14, (5, 5), 5), backend=be, ccsd_triples=False)
    assert "e_ccsd_t" not in (off.mu if off.mu is not None else off.huzinaga)


def test_driver_refuses_an_unknown_switch_value(monkeypatch):
    needs_no_pyscf()
    monkeypatch.setenv("NBED_CCSD_TRIPLES", "2")
    with pytest.raises(NbedDriverError, match="NBED_CCSD_TRIPLES"):
        nbed(config(), provider=SyntheticProvider(14, (5, 5), 5), backend=OracleBackend())


def test_config_has_no_triples_field():
    with pytest.raises(Exception):
        NbedConfig(geometry=GEOM, n_active_atoms=1, basis="synthetic", xc_functional="none", ccsd_triples=True)


# ---------------------------------------------------------------- the memory plan of the device path
def test_triples_memory_plan():
    plan = ccsd_gpu.triples_memory_plan(26, 230, 4)
    assert plan["total"] == sum(v for k, v in plan.items() if k != "total")
    assert set(plan) == {"rotated", "work", "cubes", "partials", "total"}
    assert plan["cubes"] == 4 * 8 * 230**3 and 97e6 < plan["cubes"] / 4 < 98e6  # one cube at v = 230 is 97 MB
    totals = [ccsd_gpu.triples_memory_plan(26, 230, b)["total"] for b in (1, 2, 3, 7)]
    step = totals[1] - totals[0]
    assert step > 8 * 230**3 and totals[2] - totals[1] == step and totals[3] - totals[2] == 4 * step  # linear in batch
    with pytest.raises(ValueError):
        ccsd_gpu.triples_memory_plan(26, 230, 0)
    # the loop's own plan does not know about (T)
    assert set(ccsd_gpu.memory_plan(26, 230)) == {"blocks", "spatial", "amplitudes", "work", "total"}


def test_default_batch_fits_the_free_memory():
    one = ccsd_gpu.triples_memory_plan(26, 230, 1)
    assert ccsd_gpu.default_triples_batch(26, 230, one["total"]) == 1
    assert ccsd_gpu.default_triples_batch(26, 230, 10**12) == 64
    assert ccsd_gpu.default_triples_batch(3, 230, 10**12) == 1  # one triple
    b = ccsd_gpu.default_triples_batch(26, 230, one["total"] + 40 * 8 * 230**3)
    assert 1 < b <= 20 and ccsd_gpu.triples_memory_plan(26, 230, b)["total"] <= one["total"] + 40 * 8 * 230**3


def test_refusal_names_the_bytes():
    """Even one cube does not fit: ``NbedDriverError`` with the bytes needed and the bytes free."""
    class Full:
        ccsd_gather = None

        def free_bytes(self):
            return 1000

        def to_host(self, a):
            return np.asarray(a)

    blocks = random_blocks(np.random.default_rng(3), 3, 4)
    need = ccsd_gpu.triples_memory_plan(3, 4, 1)["total"]
    with pytest.raises(NbedDriverError, match=f"{need} bytes.*1000 are free"):
        ccsd_gpu.triples_from_blocks(**blocks, backend=Full())
