"""The device CCSD (nbed_amd/ccsd_gpu.py, csrc/ccsd.hip) against the host solver nbed_amd/ccsd.py -- an independent
implementation of the same equations (dense numpy einsum) -- and, kernel by kernel, against numpy."""

import itertools

import numpy as np
import pytest

from nbed_amd import NbedConfig, ccsd, ccsd_gpu, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.exceptions import NbedDriverError
from nbed_amd.ham_builder import HamiltonianBuilder, SpatialHamiltonian

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
README_WATER = "3\n\nO 0 0 0.115\nH 0 0.754 -0.459\nH 0 -0.754 -0.459"
METHYL = "4\n\nC 0 0 0\nH 1.079 0 0\nH -0.5395 0.9344 0\nH -0.5395 -0.9344 0"  # planar CH3, r(CH) = 1.079 A

# (name, geometry, basis, spin, spin orbitals, E_corr of the host solver on the CPU with the numpy integral engine)
MOLECULES = {
    "methyl-sto3g": (METHYL, "sto-3g", 1, 16, -0.0576797669),
    "water-631g": (WATER, "6-31g", 0, 26, -0.1343584178),
    "water-ccpvdz": (WATER, "cc-pvdz", 0, 48, -0.2125425807),
}


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@pytest.fixture(scope="module")
def provider(be):
    return BuiltinHFProvider(be)


def occupied_of(scf_obj):
    mo_occ = np.asarray(scf_obj.mo_occ)
    if mo_occ.ndim == 1:
        mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
    return [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]


@pytest.fixture(scope="module")
def host_runs(be, provider):
    """Per molecule: the Hamiltonian and the host solver's amplitudes after three cycles and at convergence, computed
    once (the cap of the host solver lifted for the 48 spin orbitals of water / cc-pVDZ)."""
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
                three = ccsd.solve(const, h1, h2, occ, max_cycle=3)
                full = ccsd.solve(const, h1, h2, occ, conv_tol=1e-11)
            cache[name] = (const, h1, h2, occ, three, full)
        return cache[name]

    return get


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("extents", [(3, 5, 4, 7), (1, 1, 6, 2), (33, 2, 65, 3)])
def test_permute_all_24(be, extents):
    x = np.random.default_rng(7).standard_normal(extents)
    d = be.asarray(x)
    for perm in itertools.permutations(range(4)):
        got = be.to_host(be.permute4(d, list(perm)))
        want = np.transpose(x, perm).copy()
        assert got.shape == want.shape and np.array_equal(got, want), perm


def test_permute_accumulates(be):
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3, 5, 4, 7))
    for perm in ((1, 0, 3, 2), (0, 1, 3, 2), (2, 3, 0, 1), (0, 1, 2, 3)):
        y = rng.standard_normal(tuple(x.shape[p] for p in perm))
        out = be.asarray(y)
        be.permute4(be.asarray(x), list(perm), -1.0, 1.0, out)
        want = y - np.transpose(x, perm)
        assert np.max(np.abs(be.to_host(out) - want)) <= 2 * EPS * np.abs(x).max(), perm
    # lower ranks ride on leading extents of 1
    m = rng.standard_normal((6, 35))
    assert np.array_equal(be.to_host(be.permute4(be.asarray(m), [1, 0])), m.T)


@pytest.mark.parametrize("v", [2, 5, 33])
def test_pair_pack_unpack(be, v):
    rng = np.random.default_rng(v)
    iu = np.triu_indices(v, 1)
    for lead, trail in ((3, 1), (1, 4), (2, 3)):
        raw = rng.standard_normal((lead, v, v, trail))
        anti = raw - raw.transpose(0, 2, 1, 3)
        packed = be.pair_pack(be.asarray(anti), lead, v, trail)
        assert np.array_equal(be.to_host(packed), anti[:, iu[0], iu[1], :])
        assert np.array_equal(be.to_host(be.pair_unpack(packed, lead, v, trail)), anti)
        # not antisymmetric: the e < f element is the one taken
        assert np.array_equal(be.to_host(be.pair_pack(be.asarray(raw), lead, v, trail)), raw[:, iu[0], iu[1], :])
        # accumulate with the sign
        base = rng.standard_normal(anti.shape)
        out = be.asarray(base)
        be.pair_unpack(packed, lead, v, trail, -1.0, 1.0, out)
        assert np.max(np.abs(be.to_host(out) - (base - anti))) <= 2 * EPS * max(np.abs(base).max(), np.abs(anti).max())


def test_block_gather(be):
    """n = 5, occupied alpha {0, 2, 3} and beta {1, 4}: n_alpha != n_beta, occupied orbitals not the leading ones."""
    n = 5
    rng = np.random.default_rng(11)
    two = rng.standard_normal((3, n, n, n, n))
    two[np.abs(two) < 0.05] = 0.0  # (thresholded like build_spatial(): exact zeros among the entries)
    two *= 0.5
    ham = SpatialHamiltonian(0.0, rng.standard_normal((2, n, n)), two)
    g = ccsd.antisymmetrized(ham.h2())
    occ = sorted([2 * 0, 2 * 2, 2 * 3, 2 * 1 + 1, 2 * 4 + 1])
    vir = [p for p in range(2 * n) if p not in occ]
    lists = {"o": np.array(occ), "v": np.array(vir)}
    idx = {k: be.index_array(v, 2 * n) for k, v in lists.items()}
    tb = be.asarray(two)
    atol = 4 * EPS * np.abs(ham.h2()).max()
    for name in ("oovv", "oooo", "vvvv", "ovvo", "ovov", "ooov", "ovvv", "vvvo", "ovoo"):
        want = g[np.ix_(*(lists[c] for c in name))]
        got = be.to_host(be.ccsd_gather(tb, *(idx[c] for c in name)))
        assert got.shape == want.shape and np.max(np.abs(got - want)) <= atol, name
        if name[2] == name[3]:
            iu = np.triu_indices(want.shape[2], 1)
            got = be.to_host(be.ccsd_gather(tb, *(idx[c] for c in name), pack_last=True))
            assert np.max(np.abs(got - want[:, :, iu[0], iu[1]])) <= atol, name
            if name[0] == name[1]:
                il = np.triu_indices(want.shape[0], 1)
                got = be.to_host(be.ccsd_gather(tb, *(idx[c] for c in name), pack_first=True, pack_last=True))
                assert np.max(np.abs(got - want[:, :, iu[0], iu[1]][il[0], il[1]])) <= atol, name
    # the Fock matrix of the determinant, all spin orbitals
    h1 = ham.h1()
    want = h1 + np.einsum("piqi->pq", g[:, occ][:, :, :, occ])
    got = be.to_host(be.ccsd_fock(tb, be.asarray(h1), idx["o"]))
    assert np.max(np.abs(got - want)) <= 8 * len(occ) * EPS * np.abs(g).max()  # (a sum of len(occ) four-term elements)


def test_tau_and_update(be):
    rng = np.random.default_rng(5)
    no, nv = 3, 5
    t1, t2 = rng.standard_normal((no, nv)), rng.standard_normal((no, no, nv, nv))
    t2 = t2 - t2.transpose(1, 0, 2, 3)
    t2 = t2 - t2.transpose(0, 1, 3, 2)
    d1, d2 = be.asarray(t1), be.asarray(t2)
    direct, exch = np.einsum("ia,jb->ijab", t1, t1), np.einsum("ib,ja->ijab", t1, t1)
    scale = np.abs(t2).max() + 2 * np.abs(t1).max() ** 2
    for c2, cd, cx in ((1.0, 1.0, 1.0), (1.0, 0.5, 0.5), (0.5, 1.0, 0.0)):
        want = c2 * t2 + cd * direct - cx * exch
        assert np.max(np.abs(be.to_host(be.ccsd_tau(d1, d2, c2, cd, cx)) - want)) <= 4 * EPS * scale
    io, iv = np.triu_indices(no, 1), np.triu_indices(nv, 1)
    want = (t2 + direct - exch)[:, :, iv[0], iv[1]][io[0], io[1]]
    assert np.max(np.abs(be.to_host(be.ccsd_tau(d1, d2, 1.0, 1.0, 1.0, packed=True)) - want)) <= 4 * EPS * scale
    # t_new = r / D, err = t_new - t_old, max |err|
    eo, ev = -1.0 - rng.random(no), 0.5 + rng.random(nv)
    den = np.concatenate([(eo[:, None] - ev[None, :]).ravel(),
                          (eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None]
                           - ev[None, None, None, :]).ravel()])
    r, told = rng.standard_normal(den.size), rng.standard_normal(den.size)
    tnew, err, mx = be.empty(den.size), be.empty(den.size), be.empty(1)
    be.ccsd_update(no, nv, be.asarray(r), be.asarray(told), be.asarray(eo), be.asarray(ev), tnew, err, mx)
    got_t, got_e = be.to_host(tnew), be.to_host(err)
    assert np.all(np.abs(got_t - r / den) <= 2 * EPS * np.abs(r / den))  # (one division)
    assert np.array_equal(got_e, got_t - told)
    assert be.read_scalars(mx)[0] == np.abs(got_e).max()


# ---------------------------------------------------------------- the solver against the host solver
@pytest.mark.parametrize("name", list(MOLECULES))
def test_iterates_follow_the_host_solver(be, host_runs, name):
    """Three cycles (t1 != 0, DIIS active: every term and the extrapolation) agree to 1e-10; converged to 1e-11 both
    report convergence, agree to 1e-9 in E_corr and reproduce the host solver's CPU numbers to 1e-8."""
    const, h1, h2, occ, three, full = host_runs(name)
    dev3 = ccsd_gpu.solve(const, h1, h2, occ, max_cycle=3, backend=be)
    d1, d2 = np.max(np.abs(dev3.t1 - three.t1)), np.max(np.abs(dev3.t2 - three.t2))
    dev = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-11, backend=be)
    print(f"{name}: 3 cycles max|dt1| {d1:.2e} max|dt2| {d2:.2e}; converged {dev.iterations} / {full.iterations} cycles, "
          f"E_corr {dev.e_corr:.10f} / {full.e_corr:.10f}")
    assert np.abs(three.t1).max() > 0 and dev3.iterations == 3
    assert d1 < 1e-10 and d2 < 1e-10
    assert dev.converged and full.converged
    assert abs(dev.e_corr - full.e_corr) < 1e-9
    assert abs(dev.e_hf - full.e_hf) < 1e-10
    want = MOLECULES[name][4]
    assert abs(dev.e_corr - want) < 1e-8 and abs(full.e_corr - want) < 1e-8


def test_two_electrons_are_exact(be, provider):
    """H2 / cc-pVDZ, 20 spin orbitals: CCSD is exact, so the device solver reproduces the singlet ground state of the
    two-particle matrix (the check of test_ccsd_is_exact_for_two_electrons)."""
    cfg = NbedConfig(geometry="2\n\nH 0 0 0\nH 0 0 0.74", n_active_atoms=1, basis="cc-pvdz", xc_functional="hf",
                     convergence=1e-11)
    hf = provider.global_hf(cfg)
    const, h1, h2 = HamiltonianBuilder(hf, hf.energy_nuc(), backend=be).build()
    assert h1.shape[0] == 20
    cc = ccsd_gpu.solve(const, h1, h2, [0, 1], conv_tol=1e-12, backend=be)
    n = h1.shape[0] // 2
    ha = h1[0::2, 0::2]
    v = 2.0 * h2[0::2, 1::2, 1::2, 0::2]
    ham = (np.einsum("pr,qs->pqrs", ha, np.eye(n)) + np.einsum("qs,pr->pqrs", ha, np.eye(n))
           + v.transpose(0, 1, 3, 2)).reshape(n * n, n * n)
    assert cc.converged and abs(cc.e_hf - hf.e_tot) < 1e-10
    assert abs(cc.e_tot - (np.linalg.eigvalsh(0.5 * (ham + ham.T))[0] + const)) < 1e-9


# ---------------------------------------------------------------- the driver
def test_driver_runs_embedded_ccsd_past_the_host_cap(be, provider, monkeypatch):
    """The README's water / cc-pVDZ with two active atoms: more than 40 spin orbitals, virtuals rotated by the concentric
    localisation (the off-diagonal Fock terms matter).  The device result equals the host solver's with its cap lifted."""
    monkeypatch.delenv("NBED_CCSD_SOLVER", raising=False)
    cfg = NbedConfig(geometry=README_WATER, n_active_atoms=2, basis="cc-pVDZ", xc_functional="hf", projector="huzinaga",
                     convergence=1e-9, run_ccsd_emb=True)
    drv = nbed(cfg, provider=provider, backend=be)
    res = drv.huzinaga
    assert np.isfinite(res["e_ccsd"])
    emb = drv.embedded_scf
    assert 2 * np.asarray(emb.mo_coeff).shape[-1] > ccsd.MAX_SPIN_ORBITALS
    cc, e_corr = drv._run_emb_ccsd(emb)
    assert abs((res["e_ccsd"] - res["e_rhf"]) - (cc.e_tot - emb.e_tot)) < 1e-9
    const, h1, h2 = HamiltonianBuilder(emb, emb.energy_nuc(), backend=be).build()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ccsd, "MAX_SPIN_ORBITALS", 64)
        host = ccsd.solve(const, h1, h2, occupied_of(emb), conv_tol=min(cfg.convergence, 1e-8))
    print(f"embedded CCSD: device {cc.e_corr:.12f} host {host.e_corr:.12f}, {cc.iterations} / {host.iterations} cycles")
    assert cc.converged and host.converged
    assert abs(cc.e_corr - host.e_corr) < 1e-9 and abs(e_corr - host.e_corr) < 1e-9
    # the host solver forced: refused past its cap, as before
    monkeypatch.setenv("NBED_CCSD_SOLVER", "host")
    with pytest.raises(NbedDriverError, match="PySCF"):
        nbed(cfg, provider=provider, backend=be)


def test_driver_device_solver_forced_at_small_size(be, provider, monkeypatch):
    """Water / STO-3G (14 spin orbitals): NBED_CCSD_SOLVER=device agrees with the default (host) route."""
    cfg = NbedConfig(geometry=README_WATER, n_active_atoms=2, basis="STO-3G", xc_functional="hf", projector="huzinaga",
                     convergence=1e-9, run_ccsd_emb=True)
    monkeypatch.delenv("NBED_CCSD_SOLVER", raising=False)
    drv = nbed(cfg, provider=provider, backend=be)
    host, _ = drv._run_emb_ccsd(drv.embedded_scf)
    monkeypatch.setenv("NBED_CCSD_SOLVER", "device")
    dev, _ = drv._run_emb_ccsd(drv.embedded_scf)
    assert host.converged and dev.converged
    assert abs(dev.e_corr - host.e_corr) < 1e-9 and abs(dev.e_tot - host.e_tot) < 1e-9
