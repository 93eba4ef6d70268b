"""The device CCSD Lambda equations and one-particle density (nbed_amd/ccsd_gpu.py, csrc/ccsd_lambda.hip) against the
host solver nbed_amd/ccsd.py, against FCI for two electrons, and, kernel by kernel, against numpy.  The host solver's
own density is checked against energy derivatives in tests/test_host_ccsd_lambda.py."""

import numpy as np
import pytest

from nbed_amd import NbedConfig, ccsd, ccsd_gpu, fci, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.ham_builder import HamiltonianBuilder
from test_gpu_ccsd import MOLECULES, README_WATER, occupied_of

pytestmark = pytest.mark.gpu

KERNEL_SHAPES = [(1, 1), (2, 3), (3, 5), (5, 4)]
# nbx_ccsd_rdm1 needs no + nv even (2n spin orbitals): the two odd shapes get one more virtual; methyl's (9, 7) last
RDM1_SHAPES = [(1, 1), (2, 4), (3, 5), (5, 5), (9, 7)]


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@pytest.fixture(scope="module")
def provider(be):
    return BuiltinHFProvider(be)


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("no,nv", KERNEL_SHAPES)
def test_lambda_outer(be, no, nv):
    """r2 += alpha P(ij) P(ab) x_ia y_jb for either layout of either operand, to 1e-14 of the magnitudes involved (four
    products, three additions, one scaling, one accumulation: a few eps)."""
    rng = np.random.default_rng(100 * no + nv)
    x, y = rng.standard_normal((no, nv)), rng.standard_normal((no, nv))
    base = rng.standard_normal((no, no, nv, nv))
    d = np.einsum("ia,jb->ijab", x, y)
    outer = d - d.transpose(1, 0, 2, 3) - d.transpose(0, 1, 3, 2) + d.transpose(1, 0, 3, 2)
    for alpha, xt, yt in ((1.0, False, False), (-0.5, False, True), (2.0, True, False), (1.0, True, True)):
        r2 = be.asarray(base)
        got = be.ccsd_lambda_outer(be.asarray(x.T.copy() if xt else x), be.asarray(y.T.copy() if yt else y), r2, alpha,
                                   x_transposed=xt, y_transposed=yt)
        assert got is r2
        want = base + alpha * outer
        scale = np.abs(base).max() + 4 * abs(alpha) * np.abs(x).max() * np.abs(y).max()
        assert np.max(np.abs(be.to_host(r2) - want)) <= 1e-14 * scale, (alpha, xt, yt)
    if no != nv:
        with pytest.raises(ValueError):  # (a transposed operand that is not announced)
            be.ccsd_lambda_outer(be.asarray(x.T.copy()), be.asarray(y), be.asarray(base))
    with pytest.raises(ValueError):
        be.ccsd_lambda_outer(be.asarray(x), be.asarray(y), be.asarray(base.reshape(no, no, nv * nv)))


def spin_pattern(no, nv, seed):
    """Occupied and virtual spin orbitals that interleave: ceil(no / 2) alpha and floor(no / 2) beta occupied orbitals at
    seeded positions among the n = (no + nv) / 2 spatial ones.  (9, 7) is methyl's own: alpha 0-4, beta 0-3."""
    n = (no + nv) // 2
    if (no, nv) == (9, 7):
        occ = [2 * p for p in range(5)] + [2 * p + 1 for p in range(4)]
    else:
        rng = np.random.default_rng(seed)
        na = (no + 1) // 2
        occ = [2 * int(p) for p in rng.choice(n, na, replace=False)] + [2 * int(p) + 1 for p in rng.choice(n, no - na, replace=False)]
    occ = sorted(occ)
    return occ, [p for p in range(2 * n) if p not in occ]


def numpy_rdm1(occ, vir, goo, gov, gvo, gvv):
    nso = len(occ) + len(vir)
    g = np.zeros((nso, nso))
    g[np.ix_(occ, occ)], g[np.ix_(occ, vir)], g[np.ix_(vir, occ)], g[np.ix_(vir, vir)] = goo, gov, gvo, gvv
    cross = max(np.abs(g[0::2, 1::2]).max(), np.abs(g[1::2, 0::2]).max())
    s = 0.5 * (g + g.T)
    s[occ, occ] += 1.0
    return np.stack([s[0::2, 0::2], s[1::2, 1::2]]), cross


@pytest.mark.parametrize("no,nv", RDM1_SHAPES)
def test_rdm1_assembly(be, no, nv):
    """Every element of the (2, n, n) density, exactly (one addition, one halving, one occupation added), from blocks
    that are not symmetric and do couple the spins -- the diagnostic returns the largest such element, a planted one
    included -- and the same from spin-pure blocks, where it returns zero.  The output comes from ``be.empty``."""
    occ, vir = spin_pattern(no, nv, 7 * no + nv)
    rng = np.random.default_rng(no + 10 * nv)
    blocks = [rng.standard_normal(s) for s in ((no, no), (no, nv), (nv, no), (nv, nv))]
    so, sv = np.array(occ) & 1, np.array(vir) & 1
    masks = [so[:, None] == so[None, :], so[:, None] == sv[None, :], sv[:, None] == so[None, :], sv[:, None] == sv[None, :]]
    pure = [b * m for b, m in zip(blocks, masks)]
    planted = [b.copy() for b in pure]
    spot = np.argwhere(~masks[1])[0] if (~masks[1]).any() else None
    if spot is not None:
        planted[1][tuple(spot)] = -3.25e-7
    for case, want_zero in ((blocks, False), (pure, True), (planted, spot is None)):
        dm1, cross = be.ccsd_rdm1(occ, vir, *(be.asarray(b) for b in case))
        want, want_cross = numpy_rdm1(occ, vir, *case)
        assert np.array_equal(be.to_host(dm1), want)
        got_cross = float(be.read_scalars(cross)[0])
        assert got_cross == want_cross and (got_cross == 0.0) == want_zero
    if spot is not None:
        assert float(be.read_scalars(be.ccsd_rdm1(occ, vir, *(be.asarray(b) for b in planted))[1])[0]) == 3.25e-7
    with pytest.raises(ValueError, match="permutation"):
        be.ccsd_rdm1(occ, vir[:-1] + [occ[0]], *(be.asarray(b) for b in blocks))


# ---------------------------------------------------------------- the solver against the host solver
@pytest.fixture(scope="module")
def lambda_runs(be, provider):
    """Per molecule: the Hamiltonian and the host solver's Lambda after three cycles and at convergence, computed once
    (the cap of the host solver lifted for the 48 spin orbitals of water / cc-pVDZ)."""
    cache = {}

    def get(name):
        if name not in cache:
            geometry, basis, spin, nso, _ = MOLECULES[name]
            cfg = NbedConfig(geometry=geometry, n_active_atoms=1, basis=basis, xc_functional="hf", convergence=1e-11,
                             spin=spin)
            hf = provider.global_hf(cfg)
            const, h1, h2 = HamiltonianBuilder(hf, hf.energy_nuc(), backend=be).build()
            assert h1.shape[0] == nso
            occ = occupied_of(hf)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(ccsd, "MAX_SPIN_ORBITALS", 64)
                three = ccsd.solve(const, h1, h2, occ, max_cycle=3, density=True)
                full = ccsd.solve(const, h1, h2, occ, conv_tol=1e-11, density=True)
            cache[name] = (const, h1, h2, occ, three, full)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(MOLECULES))
def test_lambda_follows_the_host_solver(be, lambda_runs, name):
    """Three cycles of either loop (DIIS active: every term and the extrapolation) agree to 1e-10 in Lambda; converged
    to 1e-11 both report convergence and agree to 1e-9 in the density and its natural
    occupations -- the tolerances of test_iterates_follow_the_host_solver for T."""
    const, h1, h2, occ, three, full = lambda_runs(name)
    dev3 = ccsd_gpu.solve(const, h1, h2, occ, max_cycle=3, backend=be, density=True)
    d1, d2 = np.max(np.abs(dev3.l1 - three.l1)), np.max(np.abs(dev3.l2 - three.l2))
    stats = {}
    dev = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-11, backend=be, density=True, stats=stats)
    ddm = np.max(np.abs(dev.rdm1() - full.rdm1()))
    dno = np.max(np.abs(dev.natural_occupations() - full.natural_occupations()))
    print(f"{name}: 3 cycles max|dl1| {d1:.2e} max|dl2| {d2:.2e}; Lambda converged in {dev.lambda_iterations} / "
          f"{full.lambda_iterations} cycles, max|d rdm1| {ddm:.2e}, max|d occupations| {dno:.2e}, cross-spin "
          f"{stats['lambda_cross_spin']:.1e}")
    assert dev3.lambda_iterations == 3 and not np.array_equal(three.l2, three.t2)
    assert d1 < 1e-10 and d2 < 1e-10
    assert dev.lambda_converged and full.lambda_converged
    assert ddm < 1e-9 and dno < 1e-9
    nelec = (sum(1 for p in occ if p % 2 == 0), sum(1 for p in occ if p % 2))
    assert abs(np.trace(dev.rdm1()[0]) - nelec[0]) < 1e-10 and abs(np.trace(dev.rdm1()[1]) - nelec[1]) < 1e-10
    assert len(stats["lambda_cycle_seconds"]) == dev.lambda_iterations


def test_two_electrons_are_exact(be, provider):
    """H2 / cc-pVDZ, 20 spin orbitals: CCSD is exact, so its density is FCI's, element for element."""
    cfg = NbedConfig(geometry="2\n\nH 0 0 0\nH 0 0 0.74", n_active_atoms=1, basis="cc-pvdz", xc_functional="hf",
                     convergence=1e-11)
    hf = provider.global_hf(cfg)
    const, h1, h2 = HamiltonianBuilder(hf, hf.energy_nuc(), backend=be).build()
    assert h1.shape[0] == 20
    cc = ccsd_gpu.solve(const, h1, h2, [0, 1], conv_tol=1e-13, backend=be, density=True)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(fci, "MAX_SPIN_ORBITALS", 20)  # (100 determinants: the cap guards larger sectors)
        exact = fci.ground_state(const, h1, h2, (1, 1))
    diff = np.max(np.abs(cc.rdm1() - exact.rdm1()))
    print(f"H2 / cc-pVDZ: max |rdm1 - FCI| {diff:.2e}, E - E_FCI {cc.e_tot - exact.e_tot:.2e}")
    assert cc.converged and cc.lambda_converged
    assert diff < 1e-9
    assert np.max(np.abs(cc.natural_occupations() - exact.natural_occupations())) < 1e-9


def test_lambda_is_reproducible(be, lambda_runs):
    """Two runs on water / 6-31G: l2 and the density bit for bit (no atomics on the way)."""
    const, h1, h2, occ, _, _ = lambda_runs("water-631g")
    a = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-9, backend=be, density=True)
    b = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-9, backend=be, density=True)
    assert a.lambda_converged and a.lambda_iterations == b.lambda_iterations
    assert np.array_equal(a.l2, b.l2) and np.array_equal(a.l1, b.l1) and np.array_equal(a.rdm1(), b.rdm1())


def test_triples_leave_the_density_alone(be, lambda_runs):
    """``triples=True, density=True``: the density is CCSD's, the (T) energy that of a run without the density."""
    const, h1, h2, occ, _, _ = lambda_runs("methyl-sto3g")
    both = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-9, backend=be, density=True, triples=True)
    dens = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-9, backend=be, density=True)
    trip = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-9, backend=be, triples=True)
    assert np.array_equal(both.rdm1(), dens.rdm1()) and both.e_t == trip.e_t and dens.e_t is None
    with pytest.raises(ValueError, match="density=True"):
        trip.rdm1()


# ---------------------------------------------------------------- the driver
def _embedded_density_check(be, provider, monkeypatch, basis):
    cfg = NbedConfig(geometry=README_WATER, n_active_atoms=2, basis=basis, xc_functional="hf", projector="huzinaga",
                     convergence=1e-9, run_ccsd_emb=True)
    monkeypatch.delenv("NBED_CCSD_DENSITY", raising=False)
    plain = nbed(cfg, provider=provider, backend=be).huzinaga
    monkeypatch.setenv("NBED_CCSD_DENSITY", "1")
    drv = nbed(cfg, provider=provider, backend=be)
    res = drv.huzinaga
    assert "ccsd_rdm1" not in plain and "ccsd_natural_occupations" not in plain
    assert set(res) == set(plain) | {"ccsd_rdm1", "ccsd_natural_occupations"}
    assert abs(res["e_ccsd"] - plain["e_ccsd"]) < 1e-10
    emb = res["scf"]
    n = np.asarray(emb.mo_coeff).shape[-1]
    dm1 = res["ccsd_rdm1"]
    assert dm1.shape == (2, n, n) and res["ccsd_natural_occupations"].shape == (n,)
    na, nb = emb.mol.nelec
    assert abs(np.trace(dm1[0]) - na) < 1e-9 and abs(np.trace(dm1[1]) - nb) < 1e-9
    const, h1, h2 = HamiltonianBuilder(emb, emb.energy_nuc(), backend=be).build()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ccsd, "MAX_SPIN_ORBITALS", 64)
        host = ccsd.solve(const, h1, h2, occupied_of(emb), conv_tol=min(cfg.convergence, 1e-8), density=True)
    diff = np.max(np.abs(dm1 - host.rdm1()))
    print(f"embedded CCSD density ({basis}, {2 * n} spin orbitals): max |device - host| {diff:.2e}")
    assert host.lambda_converged and diff < 1e-9
    assert np.max(np.abs(res["ccsd_natural_occupations"] - host.natural_occupations())) < 1e-9
    return n


def test_driver_reports_the_embedded_density(be, provider, monkeypatch):
    """The README's water / cc-pVDZ with two active atoms (more than 40 spin orbitals, virtuals rotated by the
    concentric localisation): ``NBED_CCSD_DENSITY=1`` adds the two keys and nothing else, the density has the embedded
    electron counts and equals the host solver's with its cap lifted."""
    monkeypatch.delenv("NBED_CCSD_SOLVER", raising=False)
    n = _embedded_density_check(be, provider, monkeypatch, "cc-pVDZ")
    assert 2 * n > ccsd.MAX_SPIN_ORBITALS


def test_driver_device_density_forced_at_small_size(be, provider, monkeypatch):
    """The same at STO-3G size with ``NBED_CCSD_SOLVER=device``."""
    monkeypatch.setenv("NBED_CCSD_SOLVER", "device")
    _embedded_density_check(be, provider, monkeypatch, "STO-3G")
