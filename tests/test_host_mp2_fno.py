"""nbed_amd.mp2 without a GPU: the host solver against the two references of tests/mp2_reference.py, csrc/mp2.hip
compiled for the host (tests/native/mp2_host_shim.h runs a launch with one thread per workgroup) under the kernel tests
of tests/test_gpu_mp2_fno.py themselves, the device solver and the frozen natural orbitals on the checker backend with
that host build as its ``mp2_pairs``, the Hamiltonian builder's and the driver's switches."""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mp2_reference as ref
from oracle_backend import OracleBackend
from test_gpu_ccsd import METHYL, WATER
from test_gpu_mp2_fno import (  # noqa: F401  (collected here with this module's ``be``: the emulated kernel, no gpu mark)
    assert_same_mp2,
    check_fno_end_to_end,
    check_mp2_switch_alone,
    check_restricted,
    fno_end_to_end,
    host_reference,
    test_bad_shapes_are_refused,
    test_empty_block,
    test_opposite_spin_every_element,
    test_same_spin_every_element,
    test_same_spin_slice_over_i,
    test_tile_is_the_kernels,
)

from nbed_amd import NbedConfig, _nbx, ccsd, mp2
from nbed_amd.driver import BuiltinHFProvider, NbedDriver
from nbed_amd.exceptions import HamiltonianBuilderError, NbedDriverError
from nbed_amd.ham_builder import HamiltonianBuilder

pytestmark = []  # (the imported tests carry no mark of their own; this module needs no GPU)
REPO = Path(__file__).resolve().parent.parent
KERNELS = ("nbx_mp2_pairs", "nbx_mp2_pairs_worksize", "nbx_mp2_pairs_tile")


class Mp2CheckerBackend(OracleBackend):
    """The checker backend plus ``HipBackend.mp2_pairs`` on the host build of csrc/mp2.hip; ``empty`` is NaN-filled."""

    def __init__(self, lib):
        super().__init__()
        self.lib = lib
        self._ctx = ctypes.c_int(0)

    def empty(self, *shape):
        size = shape[0] if len(shape) == 1 and not isinstance(shape[0], int) else shape
        return self.torch.full(tuple(size), float("nan"), dtype=self.torch.float64)

    def mp2_pairs_tile(self):
        return int(self.lib.nbx_mp2_pairs_tile())

    def mp2_pairs(self, v, eo1, ev1, eo2, ev2, same_spin):
        if v.dim() != 4 or not v.is_contiguous():
            raise ValueError("mp2_pairs: v must be a contiguous (no1, nv1, no2, nv2) tensor")
        no1, nv1, no2, nv2 = (int(s) for s in v.shape)
        if eo1.numel() != no1 or ev1.numel() != nv1 or eo2.numel() != no2 or ev2.numel() != nv2:
            raise ValueError("mp2_pairs: eigenvalue vectors do not match the block")
        if same_spin and (nv1 != nv2 or no1 > no2):
            raise ValueError("mp2_pairs: a same-spin block is (no1 <= no2, nv, no2, nv)")
        same = int(bool(same_spin))
        t, energy = self.empty((nv1, no1, no2, nv2)), self.empty(1)
        # (the emulated launch runs at most three workgroups: the partial sums of the others stay zero)
        work = self.torch.zeros(max(1, int(self.lib.nbx_mp2_pairs_worksize(no1, nv1, no2, nv2, same)) // 8), dtype=self.torch.float64)
        p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        rc = self.lib.nbx_mp2_pairs(ctypes.c_void_p(ctypes.addressof(self._ctx)), no1, nv1, no2, nv2, p(v), p(eo1), p(ev1),
                                    p(eo2), p(ev2), same, p(t), p(work), 8 * work.numel(), p(energy))
        assert rc == 0, rc
        return t, energy


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host form of csrc/mp2.hip")
    work = tmp_path_factory.mktemp("mp2_host")
    shutil.copy(REPO / "nbed_amd" / "csrc" / "mp2.hip", work / "mp2_host.cpp")
    shutil.copy(REPO / "tests" / "native" / "ccsd_host_shim.h", work / "ccsd_host_shim.h")
    shutil.copy(REPO / "tests" / "native" / "mp2_host_shim.h", work / "nbx_common.h")  # (found before csrc's: same directory)
    subprocess.run([gxx, "-O1", "-std=c++17", "-fPIC", "-shared", f"-I{work}", str(work / "mp2_host.cpp"), "-o",
                    str(work / "libmp2_host.so")], check=True, capture_output=True, timeout=300)
    lib = ctypes.CDLL(str(work / "libmp2_host.so"))
    for name in KERNELS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _nbx.SIGNATURES[name]
    return Mp2CheckerBackend(lib)


def config(geometry, basis, spin=0, **kw):
    return NbedConfig(geometry=geometry, n_active_atoms=1, basis=basis, xc_functional="hf", convergence=1e-11, spin=spin, **kw)


def hamiltonian(obj, chk):
    return HamiltonianBuilder(obj, obj.energy_nuc(), backend=chk).build() + (ref.occupied_of(obj),)


@pytest.fixture(scope="module")
def h4(be):
    return BuiltinHFProvider(be).global_hf(config(ref.H4, "sto-3g"))


@pytest.fixture(scope="module")
def methyl(be):
    return BuiltinHFProvider(be).global_hf(config(METHYL, "sto-3g", spin=1))


@pytest.fixture(scope="module")
def water(be):
    return BuiltinHFProvider(be).global_hf(config(WATER, "6-31g"))


# ---------------------------------------------------------------- mp2.solve against the references
@pytest.fixture(scope="module")
def h4_forms(h4):
    """H4 in HF orbitals; after a random orthogonal rotation inside the occupied and inside the virtual space of each
    spin; after, on top of that, a small occupied-virtual rotation (f_ov != 0)."""
    within, uv = ref.rotated(h4, 5, within=True)
    return {"hf": (h4, None), "within": (within, uv), "ov": (ref.rotated(h4, 6, within=True, angle=0.05)[0], None)}


@pytest.mark.parametrize("form", ["hf", "within", "ov"])
def test_host_solver_against_both_references(be, h4_forms, form):
    """Linear H4 / STO-3G.  (a) the longdouble loops: every energy part and every element of dvv to 1e-13.  (b) the FCI
    stencils at l = 0.004 and 0.002: E(2) and every element of D_vv within ten times the difference between the two step
    sizes, as measured with the reference alone on the CPU -- 6.3e-8 for E(2) and 7.9e-8 for D_vv at the worst of the
    three forms, so TOL_E = 6.3e-7 and TOL_D = 7.9e-7 -- and the reference's own two steps must agree that well."""
    tol_e, tol_d = 6.3e-7, 7.9e-7
    const, h1, h2, occ = hamiltonian(h4_forms[form][0], be)
    got = mp2.solve(const, h1, h2, occ)
    a = ref.loops(const, h1, h2, occ)
    for name in ("e_singles", "e_same", "e_opposite", "e_corr"):
        assert abs(getattr(got, name) - a[name]) < 1e-13, name
    assert max(np.max(np.abs(got.dvv[s] - a["dvv"][s])) for s in (0, 1)) < 1e-13
    assert got.dvv.shape == (2, 2, 2) and got.natural_occupations().shape == (2, 2)
    assert (abs(got.e_singles) > 1e-4) == (form == "ov") and abs(got.e_tot - got.e_scf - got.e_corr) < 1e-15
    b = ref.fci_second_order(const, h1, h2, occ)
    diff_e = abs(b["e_corr"][0] - b["e_corr"][1])
    diff_d = max(np.max(np.abs(b["dvv"][0][s] - b["dvv"][1][s])) for s in (0, 1))
    err_e = abs(got.e_corr - b["e_corr"][1])
    err_d = max(np.max(np.abs(got.dvv[s] - b["dvv"][1][s])) for s in (0, 1))
    print(f"H4 {form}: E(2) = {got.e_corr:.10f}; FCI stencil steps differ by {diff_e:.2e} (E), {diff_d:.2e} (D); "
          f"solver - stencil {err_e:.2e} (E), {err_d:.2e} (D)")
    assert 10 * diff_e <= tol_e * 1.001 and 10 * diff_d <= tol_d * 1.001
    assert err_e < tol_e and err_d < tol_d


def test_invariance_and_covariance_under_within_space_rotations(be, h4_forms):
    """E(2) is invariant to 1e-11 and dvv transforms covariantly, D' = U_v^T D U_v, under rotations inside the
    occupied and the virtual space."""
    plain = mp2.solve(*hamiltonian(h4_forms["hf"][0], be))
    obj, uv = h4_forms["within"]
    rot = mp2.solve(*hamiltonian(obj, be))
    for name in ("e_singles", "e_same", "e_opposite", "e_corr"):
        assert abs(getattr(rot, name) - getattr(plain, name)) < 1e-11, name
    for s in (0, 1):
        assert np.max(np.abs(rot.dvv[s] - uv[s].T @ plain.dvv[s] @ uv[s])) < 1e-11
        assert np.max(np.abs(rot.natural_occupations()[s] - plain.natural_occupations()[s])) < 1e-11


def test_host_solver_on_the_methyl_radical(be, methyl):
    """An open shell (5 + 4 electrons, 3 + 4 virtuals): the longdouble loops to 1e-13; dvv is a list of two blocks."""
    const, h1, h2, occ = hamiltonian(methyl, be)
    got, a = mp2.solve(const, h1, h2, occ), ref.loops(const, h1, h2, occ)
    for name in ("e_singles", "e_same", "e_opposite", "e_corr"):
        assert abs(getattr(got, name) - a[name]) < 1e-13, name
    assert [d.shape for d in got.dvv] == [(3, 3), (4, 4)] and got.e_corr < -0.03
    assert max(np.max(np.abs(got.dvv[s] - a["dvv"][s])) for s in (0, 1)) < 1e-13
    with pytest.raises(ValueError):
        mp2.solve(0.0, np.zeros((42, 42)), np.zeros((1, 1, 1, 1)), [0])


# ---------------------------------------------------------------- the device solver on the emulated kernel
def test_solve_scf_on_the_emulated_kernel(be, h4_forms, methyl):
    for form in ("hf", "ov"):
        obj = h4_forms[form][0]
        assert_same_mp2(mp2.solve_scf(obj, backend=be), host_reference(obj, be))
        assert_same_mp2(mp2.solve_scf(obj, backend=be, capacity=1), host_reference(obj, be))
    radical, _ = ref.rotated(methyl, 7, within=True, angle=0.03)
    assert_same_mp2(mp2.solve_scf(radical, backend=be, capacity=1), host_reference(radical, be))
    with pytest.raises(ValueError):
        mp2.solve_scf(methyl, backend=OracleBackend())  # no mp2_pairs: an error, not another route


def test_memory_plan_is_host_arithmetic():
    plan = mp2.memory_plan(10, 100)
    assert plan["row_bytes"] == 2 * 8 * 100 * 10 * 100 and plan["total_bytes"] == plan["fixed_bytes"] + 10 * plan["row_bytes"]
    assert plan["rows"] == 10 and plan["slices"] == 1
    assert mp2.memory_plan(10, 100, naux=500)["fixed_bytes"] == 2 * 8 * 100 * 100 + 2 * 8 * 500 * 10 * 100
    cut = mp2.memory_plan(10, 100, capacity=plan["fixed_bytes"] + 3 * plan["row_bytes"] + 5)
    assert cut["rows"] == 3 and cut["slices"] == 4
    assert mp2.memory_plan(10, 100, capacity=0)["rows"] == 1 and mp2.memory_plan(0, 5, capacity=0)["slices"] == 0


# ---------------------------------------------------------------- frozen natural orbitals
_CCSD = {}


def ccsd_of(obj, chk, **kw):
    """E_corr of the host CCSD on the Hamiltonian of ``obj``; the untruncated one of an object is solved once."""
    key = id(obj) if not kw else None
    if key not in _CCSD:
        const, h1, h2 = HamiltonianBuilder(obj, obj.energy_nuc(), backend=chk, **kw).build()
        e = ccsd.solve(const, h1, h2, ref.occupied_of(obj)).e_corr
        if key is None:
            return e
        _CCSD[key] = (obj, e)
    return _CCSD[key][1]


def test_fno_beats_truncation_by_order_on_water(be, water):
    """Water / 6-31G, global HF, k = 2: the CCSD error of the FNO space is below 0.25 of the by-order error (measured:
    0.042), and adding dE_FNO brings it below the FNO error (measured: 3.6e-4 against 2.0e-3)."""
    k = 2
    full = ccsd_of(water, be)
    builder = HamiltonianBuilder(water, water.energy_nuc(), n_frozen_virt=k, backend=be, virtual_selection="fno")
    const, h1, h2 = builder.build()
    info = builder.fno
    e_fno = ccsd.solve(const, h1, h2, ref.occupied_of(builder.scf_method)).e_corr
    e_order = ccsd_of(water, be, n_frozen_virt=k)
    err_order, err_fno, err_corrected = abs(e_order - full), abs(e_fno - full), abs(e_fno + info["e_correction"] - full)
    print(f"water / 6-31G, k = {k}: CCSD error by order {err_order:.3e}, FNO {err_fno:.3e}, FNO + dE_FNO {err_corrected:.3e}")
    assert err_fno < 0.25 * err_order
    assert err_corrected < err_fno
    assert info["n_virtual"] == 8 and info["n_kept"] == 6 and h1.shape[0] == 22
    with pytest.raises(HamiltonianBuilderError):
        HamiltonianBuilder(water, virtual_selection="natural")


@pytest.mark.parametrize("which", ["water", "methyl"])
def test_truncated_object(be, water, methyl, which):
    """C^T S C = 1 to 1e-12; the occupied columns are those of the input, bit for bit; f_vv is diagonal in the kept
    space and equals mo_energy to 1e-10; e_tot is unchanged; with k = 0 the CCSD energy is that of the untouched object
    to 1e-9; selectors: both, neither and k >= nv are ValueErrors; a threshold keeps the larger of the two spins'
    counts."""
    obj = {"water": water, "methyl": methyl}[which]
    k = 2 if which == "water" else 1
    red, info = mp2.frozen_natural_orbitals(obj, n_frozen_virt=k, backend=be)
    c, c0 = np.asarray(red.mo_coeff), np.asarray(obj.mo_coeff)
    occ0 = np.asarray(obj.mo_occ) > 0
    s = np.asarray(obj.get_ovlp())
    fock = np.asarray(red.get_fock())
    assert red.e_tot == obj.e_tot and c.shape[-1] == c0.shape[-1] - k
    for x in (0, 1):
        no = int(occ0[x].sum())
        assert np.max(np.abs(c[x].T @ s @ c[x] - np.eye(c.shape[-1]))) < 1e-12
        assert np.array_equal(c[x][:, :no], c0[x][:, occ0[x]])
        assert np.array_equal(np.asarray(red.mo_occ)[x], np.r_[np.ones(no), np.zeros(c.shape[-1] - no)])
        fvv = c[x][:, no:].T @ fock[x] @ c[x][:, no:]
        assert np.max(np.abs(fvv - np.diag(np.asarray(red.mo_energy)[x][no:]))) < 1e-10
        occs = info["occupations"][x]
        assert np.all(occs >= -1e-14) and np.all(occs <= 1.0) and np.all(np.diff(occs) <= 1e-15)
    assert abs(info["e_mp2_kept"] - mp2.solve_scf(red, backend=be).e_corr) < 1e-11
    assert abs(info["e_correction"] - (info["e_mp2_full"] - info["e_mp2_kept"])) < 1e-15 and info["e_correction"] < 0
    same, info0 = mp2.frozen_natural_orbitals(obj, n_frozen_virt=0, backend=be)
    assert abs(info0["e_correction"]) < 1e-11 and np.asarray(same.mo_coeff).shape == c0.shape
    assert abs(ccsd_of(same, be) - ccsd_of(obj, be)) < 1e-9
    nv = min(int((~occ0[x]).sum()) for x in (0, 1))
    for bad in (dict(), dict(n_frozen_virt=1, threshold=1e-3), dict(n_frozen_virt=nv), dict(n_frozen_virt=-1)):
        with pytest.raises(ValueError):
            mp2.frozen_natural_orbitals(obj, backend=be, **bad)
    thr = float(np.sort(np.concatenate([np.ravel(o) for o in info["occupations"]]))[-3]) * 0.999
    by_thr = mp2.frozen_natural_orbitals(obj, threshold=thr, backend=be)[1]
    counts = [int(np.sum(np.asarray(info["occupations"][x]) >= thr)) for x in (0, 1)]
    kept = by_thr["n_kept"] if isinstance(by_thr["n_kept"], tuple) else (by_thr["n_kept"],) * 2
    nvs = [int((~occ0[x]).sum()) for x in (0, 1)]
    assert max(kept) >= 1 and nvs[0] - kept[0] == nvs[1] - kept[1] == min(nvs[x] - counts[x] for x in (0, 1))
    assert mp2.frozen_natural_orbitals(obj, threshold=1.0, backend=be)[1]["n_kept"] in (1, (1, 2), (2, 1))


# ---------------------------------------------------------------- the driver
def test_driver_switches_and_their_errors(monkeypatch):
    cfg = config(WATER, "sto-3g")
    for name in ("NBED_MP2", "NBED_FNO_VIRTUALS", "NBED_FNO_THRESHOLD"):
        monkeypatch.delenv(name, raising=False)
    drv = NbedDriver(cfg, provider=object(), backend=object())
    assert drv._want_mp2() is False and drv._fno_selector() == {}
    assert NbedDriver(cfg, mp2=True)._want_mp2() is True
    assert NbedDriver(cfg, fno_virtuals=3)._fno_selector() == {"n_frozen_virt": 3}
    assert NbedDriver(cfg, fno_threshold=1e-4)._fno_selector() == {"threshold": 1e-4}
    monkeypatch.setenv("NBED_MP2", "1")
    monkeypatch.setenv("NBED_FNO_VIRTUALS", "2")
    assert drv._want_mp2() is True and drv._fno_selector() == {"n_frozen_virt": 2}
    assert NbedDriver(cfg, mp2=False, fno_virtuals=0)._want_mp2() is False
    assert NbedDriver(cfg, fno_virtuals=0)._fno_selector() == {}  # (nothing to drop: FNO off, the argument wins)
    assert NbedDriver(cfg, fno_virtuals=1)._fno_selector() == {"n_frozen_virt": 1}  # (the argument wins)
    monkeypatch.setenv("NBED_FNO_THRESHOLD", "1e-3")
    with pytest.raises(NbedDriverError):
        drv._fno_selector()  # both selectors
    monkeypatch.delenv("NBED_FNO_VIRTUALS")
    assert drv._fno_selector() == {"threshold": 1e-3}
    for name, value in (("NBED_MP2", "yes"), ("NBED_FNO_THRESHOLD", "small"), ("NBED_FNO_THRESHOLD", "2")):
        monkeypatch.setenv(name, value)
        with pytest.raises(NbedDriverError):
            drv._want_mp2() if name == "NBED_MP2" else drv._fno_selector()
        monkeypatch.setenv(name, "1" if name == "NBED_MP2" else "0.5")
    monkeypatch.delenv("NBED_FNO_THRESHOLD")
    for value in ("-1", "two", "1.5"):
        monkeypatch.setenv("NBED_FNO_VIRTUALS", value)
        with pytest.raises(NbedDriverError):
            drv._fno_selector()
    with pytest.raises(NbedDriverError):
        NbedDriver(cfg, fno_virtuals=1, fno_threshold=0.1)._fno_selector()
    with pytest.raises(NbedDriverError):
        NbedDriver(cfg, fno_virtuals=-2)._fno_selector()


def test_nbed_with_fno_on_the_checker_backend(be):
    """The end-to-end inequality of tests/test_gpu_mp2_fno.py on the CPU: water / 6-31G, two active atoms, mu
    projector, k = 2, checker backend, host CCSD; and ``mp2=True`` alone sets the MP2 keys without truncating."""
    provider = BuiltinHFProvider(be)
    full, fno, by_order = fno_end_to_end(be, provider, k=2)
    check_fno_end_to_end(full, fno, by_order, 2)
    check_mp2_switch_alone(be, provider, full, fno)


def test_restricted_object_on_the_emulated_kernel(be, h4):
    check_restricted(be, h4)


def test_spin_without_occupied_orbitals(be):
    """H2 / 6-31G as a triplet (2 + 0 electrons, 2 + 4 virtuals): D^beta = 0, so beta keeps its lowest-e_a virtuals --
    the span of the lowest eigenvectors of f_vv^beta -- and alpha its natural orbitals; host and device solver agree."""
    obj = BuiltinHFProvider(be).global_hf(config("2\n\nH 0 0 0\nH 0 0 0.74", "6-31g", spin=2))
    occ = np.asarray(obj.mo_occ) > 0
    assert (int(occ[0].sum()), int(occ[1].sum())) == (2, 0)
    dev = mp2.solve_scf(obj, backend=be)
    assert_same_mp2(dev, host_reference(obj, be))
    assert not np.any(dev.dvv[1]) and dev.e_opposite == 0.0 and dev.e_same < 0
    red, info = mp2.frozen_natural_orbitals(obj, n_frozen_virt=1, backend=be)
    assert info["n_virtual"] == (2, 4) and info["n_kept"] == (1, 3) and not np.any(info["occupations"][1])
    c, s = np.asarray(red.mo_coeff), np.asarray(obj.get_ovlp())
    assert c.shape[-1] == 3 and np.array_equal(c[0][:, :2], np.asarray(obj.mo_coeff)[0][:, occ[0]])
    cv = np.asarray(obj.mo_coeff)[1]
    fock = np.asarray(obj.get_fock())[1]
    e, u = np.linalg.eigh(cv.T @ fock @ cv)
    lowest = cv @ u[:, :3]
    overlap = lowest.T @ s @ c[1]  # (the kept beta orbitals span the three lowest: an orthogonal matrix)
    assert np.max(np.abs(overlap @ overlap.T - np.eye(3))) < 1e-10
    assert np.max(np.abs(np.asarray(red.mo_energy)[1] - e[:3])) < 1e-10 and e[3] - e[2] > 1e-3
