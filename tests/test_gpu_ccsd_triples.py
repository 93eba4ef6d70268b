"""The device (T) (nbed_amd/ccsd_gpu.py: ``triples_from_blocks``, ``solve(triples=True)``; csrc/ccsd_t.hip) against the
host oracle nbed_amd/ccsd.py on the same inputs.

The kernel tests hand random operands with the right antisymmetry, a non-diagonal Fock matrix and f_ov != 0 to the
device driver and to the oracle.  Their tolerance is the forward rounding bound 4 (o + v + 40) eps S, with
S = sum |w| (|w| + |t_d|) / |D| from the oracle's arithmetic on the absolute values of every operand: two dot
products of length v and o, nine signed terms on either side, and the product."""

import numpy as np
import pytest
from test_host_ccsd_triples import random_blocks

from nbed_amd import NbedConfig, ccsd, ccsd_gpu, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.ham_builder import HamiltonianBuilder

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
T = ccsd_gpu.TRIPLES_TILE[0]
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
README_WATER = "3\n\nO 0 0 0.115\nH 0 0.754 -0.459\nH 0 -0.754 -0.459"
METHYL = "4\n\nC 0 0 0\nH 1.079 0 0\nH -0.5395 0.9344 0\nH -0.5395 -0.9344 0"  # planar CH3, r(CH) = 1.079 A
MOLECULES = {
    "methyl-sto3g": (METHYL, "sto-3g", 1, 16),
    "water-631g": (WATER, "6-31g", 0, 26),
    "water-ccpvdz": (WATER, "cc-pvdz", 0, 48),
}
SHAPES = [(3, 3), (4, 3), (3, T - 1), (3, T), (3, T + 1), (5, 2 * T + 3)]


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@pytest.fixture(scope="module")
def provider(be):
    return BuiltinHFProvider(be)


_REFERENCE = {}


def reference(no, nv):
    """(operands, oracle E_T, rounding bound) of a shape, computed once and shared."""
    if (no, nv) not in _REFERENCE:
        blocks = random_blocks(np.random.default_rng(100 * no + nv), no, nv)
        sc = ccsd.semicanonical_blocks(**blocks)
        want = ccsd.triples_sum(sc)
        bound = 4 * (no + nv + 40) * EPS * ccsd.triples_sum(sc, absolute=True)
        _REFERENCE[(no, nv)] = (blocks, want, bound)
    return _REFERENCE[(no, nv)]


def occupied_of(scf_obj):
    mo_occ = np.asarray(scf_obj.mo_occ)
    if mo_occ.ndim == 1:
        mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
    return [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]


# ---------------------------------------------------------------- the kernel with the device driver around it
def test_tile_is_the_kernels(be):
    assert be.ccsd_triples_tile() == T


@pytest.mark.parametrize("no, nv", SHAPES)
def test_random_operands_against_the_oracle(be, no, nv):
    blocks, want, bound = reference(no, nv)
    stats = {}
    got = ccsd_gpu.triples_from_blocks(**blocks, backend=be, stats=stats)
    print(f"(o, v) = ({no}, {nv}): E_T {got:.15e} oracle {want:.15e} |diff| / bound {abs(got - want) / bound:.3f} "
          f"batch {stats['triples_batch']} of {stats['triples']} triples")
    assert abs(want) > 0 and np.isfinite(got)
    assert abs(got - want) <= bound


def test_no_triples_launch_nothing(be):
    """(o, v) = (2, 5): 0.0 exactly, and the backend is not asked for a single product or kernel."""
    blocks = random_blocks(np.random.default_rng(25), 2, 5)

    class Silent:
        ccsd_gather = None

        def to_host(self, a):
            return np.asarray(a)

        def __getattr__(self, name):
            raise AssertionError(f"{name} used although there is no triple")

    assert ccsd_gpu.triples_from_blocks(**blocks, backend=Silent()) == 0.0
    assert ccsd_gpu.triples_from_blocks(**blocks, backend=be) == 0.0
    few_virtuals = random_blocks(np.random.default_rng(26), 4, 2)
    assert ccsd_gpu.triples_from_blocks(**few_virtuals, backend=be) == 0.0
    # the entry point itself: no cubes, energy 0
    out = be.empty(1)
    ijk = be.int_array(np.zeros((0, 3)))
    z = be.zeros(1)
    be.ccsd_triples_energy(2, 5, z, ijk, be.zeros(10), be.zeros(10), be.zeros(100), be.zeros(100), be.zeros(2), be.zeros(5),
                           z, out)
    assert be.read_scalars(out)[0] == 0.0


# ---------------------------------------------------------------- batching
def test_batches_agree_and_repeat_bit_for_bit(be):
    no, nv = 5, 2 * T + 3  # 10 triples
    blocks, want, bound = reference(no, nv)
    runs = {}
    for batch in (1, 3, None):  # 3 does not divide 10: the last batch is short
        stats = {}
        runs[batch] = ccsd_gpu.triples_from_blocks(**blocks, batch=batch, backend=be, stats=stats)
        assert stats["triples_batch"] == (batch or 10)
        assert abs(runs[batch] - want) <= bound, batch
    assert abs(runs[1] - runs[3]) <= bound and abs(runs[3] - runs[None]) <= bound
    for batch in (1, 3, None):
        assert ccsd_gpu.triples_from_blocks(**blocks, batch=batch, backend=be) == runs[batch], batch
    with pytest.raises(ValueError):
        ccsd_gpu.triples_from_blocks(**blocks, batch=0, backend=be)


# ---------------------------------------------------------------- poison
def test_every_slot_read_was_written(monkeypatch):
    """NBED_POISON_EMPTY=1 fills every ``empty`` buffer with NaN: rotated operands, cubes, partial sums and per-batch
    energies must all have been written before they are read, the short last batch included."""
    from nbed_amd.backend import HipBackend

    monkeypatch.setenv("NBED_POISON_EMPTY", "1")
    poisoned = HipBackend()
    assert np.isnan(poisoned.to_host(poisoned.empty(4))).all()
    for (no, nv), batch in (((5, 2 * T + 3), 3), ((3, T + 1), None), ((4, 3), 1)):
        blocks, want, bound = reference(no, nv)
        got = ccsd_gpu.triples_from_blocks(**blocks, batch=batch, backend=poisoned)
        assert np.isfinite(got) and abs(got - want) <= bound, (no, nv)


# ---------------------------------------------------------------- converged molecules
@pytest.fixture(scope="module")
def host_runs(be, provider):
    """Per molecule: the Hamiltonian and the host solver's converged result with its (T), computed once (the cap of the
    host solver lifted for the 48 spin orbitals of water / cc-pVDZ)."""
    cache = {}

    def get(name):
        if name not in cache:
            geometry, basis, spin, nso = MOLECULES[name]
            cfg = NbedConfig(geometry=geometry, n_active_atoms=1, basis=basis, xc_functional="hf", convergence=1e-11,
                             spin=spin)
            hf = provider.global_hf(cfg)
            const, h1, h2 = HamiltonianBuilder(hf, hf.energy_nuc(), backend=be).build()
            assert h1.shape[0] == nso
            occ = occupied_of(hf)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(ccsd, "MAX_SPIN_ORBITALS", 64)
                full = ccsd.solve(const, h1, h2, occ, conv_tol=1e-11, triples=True)
            cache[name] = (const, h1, h2, occ, full)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(MOLECULES))
def test_converged_molecules(be, host_runs, name):
    """Device e_t against the host solver's at convergence (1e-11): 1e-9, the tolerance tests/test_gpu_ccsd.py uses for
    E_corr there.  Without the switch the result carries no (T)."""
    const, h1, h2, occ, full = host_runs(name)
    dev = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-11, backend=be, triples=True)
    print(f"{name}: E_T device {dev.e_t:.12f} host {full.e_t:.12f}, E_corr {dev.e_corr:.12f} / {full.e_corr:.12f}")
    assert dev.converged and full.converged
    assert full.e_t < 0.0 and abs(full.e_t) > 1e-7
    assert abs(dev.e_t - full.e_t) < 1e-9
    assert abs(dev.e_corr - full.e_corr) < 1e-9
    assert dev.e_tot_t == dev.e_tot + dev.e_t
    if name == "methyl-sto3g":
        plain = ccsd_gpu.solve(const, h1, h2, occ, conv_tol=1e-11, backend=be)
        assert plain.e_t is None and plain.e_tot_t is None and plain.e_corr == dev.e_corr


# ---------------------------------------------------------------- the driver
def test_driver_device_solver_with_triples(be, provider, monkeypatch):
    """Water / STO-3G, two active atoms: NBED_CCSD_SOLVER=device with NBED_CCSD_TRIPLES=1 reports e_ccsd_t, and
    e_ccsd_t - e_ccsd is the host oracle's (T) of the same embedded object to 1e-9."""
    cfg = NbedConfig(geometry=README_WATER, n_active_atoms=2, basis="STO-3G", xc_functional="hf", projector="huzinaga",
                     convergence=1e-9, run_ccsd_emb=True)
    monkeypatch.setenv("NBED_CCSD_SOLVER", "device")
    monkeypatch.delenv("NBED_CCSD_TRIPLES", raising=False)
    plain = nbed(cfg, provider=provider, backend=be).huzinaga
    assert "e_ccsd_t" not in plain and "ccsd_t_emb" not in plain
    monkeypatch.setenv("NBED_CCSD_TRIPLES", "1")
    drv = nbed(cfg, provider=provider, backend=be)
    res = drv.huzinaga
    emb = drv.embedded_scf
    const, h1, h2 = HamiltonianBuilder(emb, emb.energy_nuc(), backend=be).build()
    host = ccsd.solve(const, h1, h2, occupied_of(emb), conv_tol=min(cfg.convergence, 1e-8), triples=True)
    print(f"embedded (T): device {res['e_ccsd_t'] - res['e_ccsd']:.12f} host {host.e_t:.12f}")
    assert host.converged and abs(host.e_t) > 1e-7
    assert abs((res["e_ccsd_t"] - res["e_ccsd"]) - host.e_t) < 1e-9
    assert abs((res["ccsd_t_emb"] - res["ccsd_emb"]) - host.e_t) < 1e-9
    assert abs(res["e_ccsd"] - plain["e_ccsd"]) < 1e-9
