"""The CCSD Lambda equations and one-particle density of the host solver (nbed_amd/ccsd.py) against energy derivatives
of the amplitude solver (tests/ccsd_lambda_reference.py: no second implementation of the equations) and against FCI for
two electrons; csrc/ccsd_lambda.hip compiled for the host (tests/native/ccsd_host_shim.h) against numpy, by the kernel
tests of tests/test_gpu_ccsd_lambda.py themselves; and the device solver's Lambda algebra (nbed_amd/ccsd_gpu.py on
these kernels, products in numpy) against the host solver.  No GPU needed."""

import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import ccsd_lambda_reference as ref
from oracle_backend import OracleBackend
from synthetic_provider import SyntheticProvider
from test_gpu_ccsd import METHYL, occupied_of
from test_gpu_ccsd_lambda import (  # noqa: F401  (collected here with this module's ``be``: the emulated kernels, no gpu mark)
    test_lambda_outer,
    test_rdm1_assembly,
)
from test_host_ccsd_kernels import KERNELS, REPO, EmulatedKernels
from test_host_ccsd_triples import config, needs_no_pyscf

from nbed_amd import NbedConfig, _nbx, ccsd, ccsd_gpu, fci, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.exceptions import NbedDriverError
from nbed_amd.ham_builder import HamiltonianBuilder

LAMBDA_KERNELS = ("nbx_ccsd_lambda_outer", "nbx_ccsd_rdm1")


@pytest.fixture(scope="module")
def hamiltonian():
    """(const, h1, h2, occupied) of a molecule's global Hartree-Fock determinant in its own orbitals, computed once."""
    chk = OracleBackend()
    cache = {}

    def get(geometry, basis, spin=0):
        key = (geometry, basis, spin)
        if key not in cache:
            cfg = NbedConfig(geometry=geometry, n_active_atoms=1, basis=basis, xc_functional="hf", convergence=1e-11, spin=spin)
            hf = BuiltinHFProvider(chk).global_hf(cfg)
            cache[key] = HamiltonianBuilder(hf, hf.energy_nuc(), backend=chk).build() + (occupied_of(hf),)
        return cache[key]

    return get


# ---------------------------------------------------------------- 1. two electrons
@pytest.mark.parametrize("basis,nso", [("6-31g", 8), ("cc-pvdz", 20)])
def test_two_electrons_are_exact(hamiltonian, basis, nso):
    """H2: CCSD is FCI, so the Lambda-based density is the FCI density, element for element and in both spins."""
    const, h1, h2, occ = hamiltonian("2\n\nH 0 0 0\nH 0 0 0.74", basis)
    assert h1.shape[0] == nso and occ == [0, 1]
    cc = ccsd.solve(const, h1, h2, occ, conv_tol=ref.CONV, density=True)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(fci, "MAX_SPIN_ORBITALS", 20)  # (100 determinants: the cap guards larger sectors)
        exact = fci.ground_state(const, h1, h2, (1, 1))
    dm, want = cc.rdm1(), exact.rdm1()
    print(f"H2 / {basis}: max |rdm1 - FCI| {np.max(np.abs(dm - want)):.2e} after {cc.lambda_iterations} Lambda cycles, "
          f"E - E_FCI {cc.e_tot - exact.e_tot:.2e}")
    assert cc.converged and cc.lambda_converged is True
    assert dm.shape == (2, nso // 2, nso // 2) and np.max(np.abs(dm - want)) < 1e-9
    assert np.max(np.abs(cc.natural_occupations() - exact.natural_occupations())) < 1e-9
    assert abs(np.trace(dm[0]) - 1.0) < 1e-10 and abs(np.trace(dm[1]) - 1.0) < 1e-10
    assert cc.l1.shape == cc.t1.shape and cc.l2.shape == cc.t2.shape


# ---------------------------------------------------------------- 2. every element, closed shell
def test_every_element_is_an_energy_derivative(hamiltonian):
    """Linear H4 / STO-3G in Hartree-Fock orbitals: for every p <= q and both spins the stencil of V = E_pq + E_qp
    (E_pp on the diagonal) in that spin block equals (2 - delta_pq) dm1[s, p, q] to 1e-8: every element of the density,
    with both step sizes for every fourth."""
    const, h1, h2, occ = hamiltonian(ref.H4, "sto-3g")
    n = h1.shape[0] // 2
    assert n == 4 and len(occ) == 4
    dm = ccsd.solve(const, h1, h2, occ, conv_tol=ref.CONV, density=True).rdm1()
    assert np.array_equal(dm, dm.transpose(0, 2, 1))
    worst, count = 0.0, 0
    for s in range(2):
        for p in range(n):
            for q in range(p, n):
                v = ref.unit_direction(n, s, p, q)
                want = (2.0 - (p == q)) * dm[s, p, q]
                label = f"H4 s={s} p={p} q={q}"
                got = (ref.stencil_checked(const, h1, h2, occ, v, label) if count % 4 == 0
                       else ref.stencil(const, h1, h2, occ, v))
                worst = max(worst, abs(got - want))
                count += 1
                assert abs(got - want) < ref.TOL, (label, got, want)
    print(f"H4: {count} perturbations, worst |stencil - (2 - delta) dm1| {worst:.2e}")
    assert count == n * (n + 1)


# ---------------------------------------------------------------- 3. non-HF reference
def test_non_hf_reference(hamiltonian):
    """The same H4 with a fixed one-body term W added: f_ov != 0, f_oo and f_vv not diagonal -- every off-diagonal Fock
    term of the Lambda equations is live.  One random direction, different in the two spins, and ten single elements."""
    const, h1, h2, occ = hamiltonian(ref.H4, "sto-3g")
    n = h1.shape[0] // 2
    h1w = h1 + ref.spin_blocks_to_spin_orbitals(ref.non_hf_term(n, len(occ) // 2))
    cc = ccsd.solve(const, h1w, h2, occ, conv_tol=ref.CONV, density=True)
    dm = cc.rdm1()
    assert cc.lambda_converged and np.abs(cc.t1).max() > 1e-3 and np.abs(cc.l1 - cc.t1).max() > 1e-5
    v = ref.random_direction(n, 77)
    got = ref.stencil_checked(const, h1w, h2, occ, v, "H4 + W, random direction")
    print(f"H4 + W: stencil {got:.12f}  tr(V dm1) {np.sum(v * dm):.12f}")
    assert abs(got - np.sum(v * dm)) < ref.TOL
    rng = np.random.default_rng(78)
    for k in range(10):
        s, p, q = int(rng.integers(2)), int(rng.integers(n)), int(rng.integers(n))
        p, q = min(p, q), max(p, q)
        v = ref.unit_direction(n, s, p, q)
        got = ref.stencil_checked(const, h1w, h2, occ, v, f"H4 + W s={s} p={p} q={q}") if k < 2 else ref.stencil(const, h1w, h2, occ, v)
        assert abs(got - (2.0 - (p == q)) * dm[s, p, q]) < ref.TOL, (s, p, q)


# ---------------------------------------------------------------- 4. open shell
def test_open_shell(hamiltonian):
    """Methyl / STO-3G, 5 + 4 electrons in 16 spin orbitals."""
    const, h1, h2, occ = hamiltonian(METHYL, "sto-3g", 1)
    assert h1.shape[0] == 16 and len(occ) == 9
    cc = ccsd.solve(const, h1, h2, occ, conv_tol=ref.CONV, density=True)
    dm = cc.rdm1()
    v = ref.random_direction(8, 79)
    got = ref.stencil_checked(const, h1, h2, occ, v, "methyl, random direction")
    print(f"methyl: stencil {got:.12f}  tr(V dm1) {np.sum(v * dm):.12f}")
    assert cc.lambda_converged and abs(got - np.sum(v * dm)) < ref.TOL
    assert abs(np.trace(dm[0]) - 5.0) < 1e-10 and abs(np.trace(dm[1]) - 4.0) < 1e-10
    for s in range(2):
        occupations = np.linalg.eigvalsh(dm[s])
        assert occupations.min() > -1e-3 and occupations.max() < 1.0 + 1e-3
    nat = cc.natural_occupations()
    assert np.all(np.diff(nat) <= 0) and abs(nat.sum() - 9.0) < 1e-10


# ---------------------------------------------------------------- 5. the kernels on the host
class LambdaKernels(EmulatedKernels):
    """``EmulatedKernels`` with the wrappers of csrc/ccsd_lambda.hip's two kernels, argument checks included."""

    def ccsd_lambda_outer(self, x, y, r2, alpha=1.0, x_transposed=False, y_transposed=False):
        if r2.dim() != 4 or r2.shape[0] != r2.shape[1] or r2.shape[2] != r2.shape[3] or not r2.is_contiguous():
            raise ValueError("ccsd_lambda_outer: r2 must be a contiguous (no, no, nv, nv) tensor")
        no, nv = int(r2.shape[0]), int(r2.shape[2])
        for t, tr in ((x, x_transposed), (y, y_transposed)):
            if tuple(t.shape) != ((nv, no) if tr else (no, nv)) or not t.is_contiguous():
                raise ValueError("ccsd_lambda_outer: operand shapes")
        self._call("nbx_ccsd_lambda_outer", no, nv, float(alpha), self._p(x), self._p(y),
                   int(bool(x_transposed)) | (int(bool(y_transposed)) << 1), self._p(r2))
        return r2

    def ccsd_rdm1(self, occ, vir, goo, gov, gvo, gvv):
        occ, vir = [int(i) for i in occ], [int(i) for i in vir]
        no, nv = len(occ), len(vir)
        nso = no + nv
        if nso % 2 or nso == 0 or sorted(occ + vir) != list(range(nso)):
            raise ValueError("ccsd_rdm1: occ and vir must together be a permutation of the 2n spin-orbital indices")
        goo, gov, gvo, gvv = (t.contiguous() for t in (goo, gov, gvo, gvv))
        n = nso // 2
        dm1, cross = self.empty((2, n, n)), self.empty(1)
        d_occ, d_vir = self.index_array(occ, nso), self.index_array(vir, nso)
        self._call("nbx_ccsd_rdm1", n, no, nv, self._p(d_occ), self._p(d_vir), self._p(goo), self._p(gov), self._p(gvo),
                   self._p(gvv), self._p(dm1), self._p(cross))
        return dm1, cross


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host form of csrc/ccsd.hip and csrc/ccsd_lambda.hip")
    work = tmp_path_factory.mktemp("ccsd_lambda_host")
    for name in ("ccsd", "ccsd_lambda"):
        shutil.copy(REPO / "nbed_amd" / "csrc" / f"{name}.hip", work / f"{name}_host.cpp")
    shutil.copy(REPO / "tests" / "native" / "ccsd_host_shim.h", work / "nbx_common.h")  # (found before csrc's: same directory)
    subprocess.run([gxx, "-O1", "-std=c++17", "-fPIC", "-shared", f"-I{work}", str(work / "ccsd_host.cpp"),
                    str(work / "ccsd_lambda_host.cpp"), "-o", str(work / "libccsd_lambda_host.so")], check=True,
                   capture_output=True, timeout=300)
    lib = ctypes.CDLL(str(work / "libccsd_lambda_host.so"))
    for name in KERNELS + LAMBDA_KERNELS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _nbx.SIGNATURES[name]
    return LambdaKernels(lib)


def test_lambda_on_emulated_kernels_follows_the_host_solver(be, hamiltonian):
    """CH3 / STO-3G (16 spin orbitals): Lambda after three cycles to 1e-10, the converged density to 1e-9."""
    const, h1, h2, occ = hamiltonian(METHYL, "sto-3g", 1)
    host = ccsd.solve(const, h1, h2, occ, max_cycle=3, density=True)
    dev = ccsd_gpu.solve(const, h1, h2, occ, backend=be, max_cycle=3, density=True)
    assert dev.lambda_iterations == host.lambda_iterations == 3 and not dev.lambda_converged
    assert np.max(np.abs(dev.l1 - host.l1)) < 1e-10 and np.max(np.abs(dev.l2 - host.l2)) < 1e-10
    host = ccsd.solve(const, h1, h2, occ, conv_tol=1e-11, density=True)
    stats = {}
    dev = ccsd_gpu.solve(const, h1, h2, occ, backend=be, conv_tol=1e-11, density=True, stats=stats)
    print(f"methyl on the emulated kernels: max |d rdm1| {np.max(np.abs(dev.rdm1() - host.rdm1())):.2e}, "
          f"{dev.lambda_iterations} / {host.lambda_iterations} Lambda cycles")
    assert host.lambda_converged and dev.lambda_converged
    assert np.max(np.abs(dev.rdm1() - host.rdm1())) < 1e-9
    assert np.max(np.abs(dev.natural_occupations() - host.natural_occupations())) < 1e-9
    assert stats["lambda_iterations"] == dev.lambda_iterations == len(stats["lambda_cycle_seconds"])
    assert stats["plan"]["lambda"] > 0


def test_cross_spin_elements_are_not_dropped():
    """A density block that couples alpha and beta is an error on either route."""
    blocks = {"oo": np.zeros((2, 2)), "ov": np.zeros((2, 2)), "vo": np.zeros((2, 2)), "vv": np.zeros((2, 2))}
    dm, cross = ccsd.spin_resolved_density(blocks, [0, 1], [2, 3], 4)
    assert cross == 0.0 and np.array_equal(dm, np.stack([np.diag([1.0, 0.0])] * 2))
    blocks["ov"][0, 1] = 1e-9  # occupied alpha 0 with virtual beta 3
    with pytest.raises(ValueError, match="alpha and beta"):
        ccsd.spin_resolved_density(blocks, [0, 1], [2, 3], 4)


# ---------------------------------------------------------------- 6. interface
def test_no_density_without_the_switch(hamiltonian):
    const, h1, h2, occ = hamiltonian("2\n\nH 0 0 0\nH 0 0 0.74", "6-31g")
    cc = ccsd.solve(const, h1, h2, occ)
    assert cc.l1 is None and cc.l2 is None and cc.lambda_converged is None
    for method in (cc.rdm1, cc.natural_occupations):
        with pytest.raises(ValueError, match="density=True"):
            method()
    plain = ccsd.CCSDResult(-1.0, -0.1, cc.t1, cc.t2, True, 5)  # (the constructor of before: new arguments optional)
    assert plain.e_tot == -1.1 and plain.e_t is None and plain.l1 is None


def test_driver_switch(monkeypatch):
    """``NBED_CCSD_DENSITY`` / ``ccsd_density`` on the synthetic embedded problem of tests/test_host_ccsd_triples.py."""
    needs_no_pyscf()
    chk = OracleBackend()
    monkeypatch.delenv("NBED_CCSD_SOLVER", raising=False)

    def run(**kw):
        drv = nbed(config(), provider=SyntheticProvider(14, (5, 5), 5), backend=chk, **kw)
        return drv, (drv.mu if drv.mu is not None else drv.huzinaga)

    monkeypatch.setenv("NBED_CCSD_DENSITY", "2")
    with pytest.raises(NbedDriverError, match="NBED_CCSD_DENSITY='2'.*'0' or '1'"):
        run()
    monkeypatch.delenv("NBED_CCSD_DENSITY")
    _, plain = run()
    monkeypatch.setenv("NBED_CCSD_DENSITY", "1")
    drv, res = run()
    assert set(res) == set(plain) | {"ccsd_rdm1", "ccsd_natural_occupations"} and "ccsd_rdm1" not in plain
    emb = drv.embedded_scf
    n = np.asarray(emb.mo_coeff).shape[-1]
    na, nb = emb.mol.nelec
    dm = res["ccsd_rdm1"]
    assert dm.shape == (2, n, n) and res["ccsd_natural_occupations"].shape == (n,)
    assert abs(np.trace(dm[0]) - na) < 1e-9 and abs(np.trace(dm[1]) - nb) < 1e-9
    assert abs(res["e_ccsd"] - plain["e_ccsd"]) < 1e-12  # the switch leaves the energy alone
    const, h1, h2 = HamiltonianBuilder(emb, emb.energy_nuc(), backend=chk).build()
    want = ccsd.solve(const, h1, h2, occupied_of(emb), conv_tol=1e-9, density=True).rdm1()
    assert np.max(np.abs(dm - want)) < 1e-9
    # the argument wins over the environment, either way
    monkeypatch.setenv("NBED_CCSD_DENSITY", "0")
    assert np.array_equal(run(ccsd_density=True)[1]["ccsd_rdm1"], dm)
    monkeypatch.setenv("NBED_CCSD_DENSITY", "1")
    assert "ccsd_rdm1" not in run(ccsd_density=False)[1]


def test_memory_plan():
    """The default plan is today's (tests/test_host_ccsd_gpu_api.py pins its numbers); with the density it grows by the
    ``lambda`` group alone, and the refusal names that group."""
    for no, nv in ((10, 38), (9, 7), (66, 190)):
        base = ccsd_gpu.memory_plan(no, nv)
        assert base == ccsd_gpu.memory_plan(no, nv, 6, density=False) and "lambda" not in base
        n1 = no * nv
        assert base["amplitudes"] == 8 * (2 * (n1 + n1 * n1) + 12 * (n1 + n1 * n1) + 2 * n1 * n1
                                          + (no * (no - 1) // 2) * (nv * (nv - 1) // 2))
        dens = ccsd_gpu.memory_plan(no, nv, density=True)
        assert dens["total"] == base["total"] + dens["lambda"] and dens["lambda"] >= 8 * (n1 + n1 * n1 + 2 * no * nv**3)
        assert {k: v for k, v in dens.items() if k not in ("lambda", "total")} == {k: v for k, v in base.items() if k != "total"}

    class Full(EmulatedKernels):
        """A device with 1000 free bytes: the plan is refused before any kernel is asked for."""

        def __init__(self):
            super().__init__(None)

        def free_bytes(self):
            return 1000

    one, two = np.zeros((2, 4, 4)), np.zeros((3, 4, 4, 4, 4))
    with pytest.raises(NbedDriverError, match="Lambda amplitudes"):
        ccsd_gpu.solve_spatial((0.0, one, two), [0, 1], backend=Full(), density=True)
    with pytest.raises(NbedDriverError) as info:
        ccsd_gpu.solve_spatial((0.0, one, two), [0, 1], backend=Full())
    assert "Lambda" not in str(info.value)
