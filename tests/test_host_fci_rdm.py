"""The FCI densities without a GPU: the reference tests/fci_rdm_reference.py against hand-computed values; the host
solver object's methods (nbed_amd/fci.py) against it; the energy and <S^2> identities; the memory plan and the
refusals of nbed_amd/fci_gpu.py; the C ABI; and csrc/fci_rdm.hip compiled for the host beside csrc/fci.hip
(tests/native/fci_rdm_host_shim.h: one thread per workgroup, the GEMM in numpy), which runs the small-sector tests of
tests/test_gpu_fci_rdm.py themselves -- the index maps of the kernels and the chunk and slab arithmetic around them.
The wavefront butterfly, LDS staging across real wavefronts and the GEMM are exercised only by the GPU suite."""

import ctypes
import itertools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

import fci_reference as ref
import fci_rdm_reference as rref
from test_gpu_fci_rdm import (  # noqa: F401  (collected here with this module's ``be``: the emulated kernels, no gpu mark)
    energy_tolerance,
    integrals_norm,
    small,
    test_direct_rdm1,
    test_identities,
    test_rdm12_every_element,
    test_sampled_elements_n9_chunked,
    test_spin_square_of_single_determinants,
    unit_vectors,
)
from test_host_fci_kernels import EmulatedKernels

from nbed_amd import _nbx, fci, fci_gpu
from nbed_amd.backend import HipBackend
from nbed_amd.exceptions import NbedDriverError

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "nbx.h").read_text()
KERNELS = ("nbx_fci_gmat", "nbx_fci_gather", "nbx_fci_scatter", "nbx_fci_diag", "nbx_fci_precond", "nbx_fci_rdm_finish",
           "nbx_fci_rdm1")
HOST_SECTORS = [(2, 1, 1), (4, 4, 1), (5, 3, 0), (5, 3, 2), (6, 3, 3), (7, 5, 5)]


class EmulatedRdmKernels(EmulatedKernels):
    """EmulatedKernels with the density kernels from the host build and a ``gemm_raw`` for every layout, batched."""

    def zeros(self, *shape):
        size = shape[0] if len(shape) == 1 and not isinstance(shape[0], int) else shape
        return self.torch.zeros(tuple(size), dtype=self.torch.float64)

    def gemm_raw(self, ta, tb, m, n, k, alpha, a, lda, sa, b, ldb, sb, beta, c, ldc, sc, batch):
        av, bv, cv = a.numpy().reshape(-1), b.numpy().reshape(-1), c.numpy().reshape(-1)
        for z in range(batch):
            am = as_strided(av[z * sa:], (m, k) if ta == "N" else (k, m), (8 * lda, 8))
            bm = as_strided(bv[z * sb:], (k, n) if tb == "N" else (n, k), (8 * ldb, 8))
            cm = as_strided(cv[z * sc:], (m, n), (8 * ldc, 8))
            prod = alpha * ((am if ta == "N" else am.T) @ (bm if tb == "N" else bm.T))
            cm[...] = prod if beta == 0.0 else prod + beta * cm


for _name in ("fci_rdm_finish", "fci_rdm1"):  # the wrappers of nbed_amd/backend.py
    setattr(EmulatedRdmKernels, _name, getattr(HipBackend, _name))


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host form of csrc/fci.hip and csrc/fci_rdm.hip")
    work = tmp_path_factory.mktemp("fci_rdm_host")
    shutil.copy(REPO / "nbed_amd" / "csrc" / "fci.hip", work / "fci_host.cpp")
    shutil.copy(REPO / "nbed_amd" / "csrc" / "fci_rdm.hip", work / "fci_rdm_host.cpp")
    shutil.copy(REPO / "tests" / "native" / "fci_host_shim.h", work / "fci_host_shim.h")
    shutil.copy(REPO / "tests" / "native" / "fci_rdm_host_shim.h", work / "nbx_common.h")  # (found before csrc's: same directory)
    subprocess.run([gxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-DNBX_FCI_PT=1024", "-DNBX_RDM_WAVE=1", f"-I{work}",
                    str(work / "fci_host.cpp"), str(work / "fci_rdm_host.cpp"), "-o", str(work / "libfci_rdm_host.so")],
                   check=True, capture_output=True, timeout=300)
    lib = ctypes.CDLL(str(work / "libfci_rdm_host.so"))
    for name in KERNELS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _nbx.SIGNATURES[name]
    return EmulatedRdmKernels(lib)


# ---------------------------------------------------------------- the reference against hand-computed values
def test_reference_two_determinants_by_hand():
    """n = 2, (1, 1): |a_i b_j> = a+_ia a+_jb |0>, index 2 i + j.  For c = 0.6 |a0 b0> + 0.8 |a1 b1>:
    dm1 = diag(0.36, 0.64) for both spins; <c| a+_pa a+_qb a_rb a_sa |c> = c[p,q] c[s,r]; no same-spin pairs.  With the
    bra |a0 b1>: a_1a takes 0.8 |a1 b1> to 0.8 |b1>, so <b| a+_0a a_1a |c> = 0.8; a_0b takes 0.6 |a0 b0> to -0.6 |a0>
    and a+_1b puts the beta electron back behind the alpha one, sign restored: <b| a+_1b a_0b |c> = 0.6."""
    c = np.array([[0.6, 0.0], [0.0, 0.8]])
    dm1, dm2 = rref.rdm12(2, (1, 1), c)
    assert np.allclose(dm1, [np.diag([0.36, 0.64])] * 2, atol=1e-16)
    want = np.zeros((2, 2, 2, 2))
    want[0, 0, 0, 0], want[1, 1, 1, 1], want[0, 0, 1, 1], want[1, 1, 0, 0] = 0.36, 0.64, 0.48, 0.48
    assert np.allclose(dm2[2], want, atol=1e-16) and not dm2[0].any() and not dm2[1].any()
    bra = np.array([[0.0, 1.0], [0.0, 0.0]])
    t1, t2 = rref.rdm12(2, (1, 1), c, bra)
    want1 = np.zeros((2, 2, 2))
    want1[0, 0, 1], want1[1, 1, 0] = 0.8, 0.6
    assert np.array_equal(t1, want1)
    want2 = np.zeros((2, 2, 2, 2))  # <b| a+_pa a+_qb a_rb a_sa |c> = b[p,q] c[s,r]
    want2[0, 1, 0, 0], want2[0, 1, 1, 1] = 0.6, 0.8
    assert np.array_equal(t2[2], want2)
    sec = ref.Sector(2, (1, 1))
    assert rref.dm1_element(sec, c, bra, 0, 0, 1) == 0.8 and rref.dm1_element(sec, c, bra, 1, 1, 0) == 0.6
    assert rref.dm2_element(sec, c, c, 2, 0, 0, 1, 1) == 0.48 and rref.dm2_element(sec, c, bra, 2, 0, 1, 1, 1) == 0.8
    assert rref.dm2_element(sec, c, c, 0, 0, 1, 1, 0) == 0.0


def test_reference_single_elements_match_the_full_arrays():
    n, nelec = 5, (3, 2)
    sec = ref.Sector(n, nelec)
    b, c = unit_vectors(sec.shape, 5)
    dm1, dm2 = rref.rdm12(n, nelec, c, b)
    rng = np.random.default_rng(1)
    for _ in range(30):
        x, spin = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        p, q, r, s = (int(i) for i in rng.integers(0, n, 4))
        assert abs(rref.dm2_element(sec, c, b, x, p, q, r, s) - dm2[x, p, q, r, s]) <= 1e-15
        assert abs(rref.dm1_element(sec, c, b, spin, p, q) - dm1[spin, p, q]) <= 1e-15


# ---------------------------------------------------------------- the host solver object
def host_result(sector, seed):
    """An FCIResult with two random normalised vectors in the host solver's determinant order and operator convention."""
    n, na, nb = sector
    dets = []
    for occ_a in itertools.combinations(range(n), na):
        for occ_b in itertools.combinations(range(n), nb):
            dets.append(sum(1 << (2 * p) for p in occ_a) | sum(1 << (2 * p + 1) for p in occ_b))
    b, c = unit_vectors(len(dets), seed)
    return fci.FCIResult(0.0, np.zeros(2), np.stack([c, b], axis=1), dets, norb=n, nelec=(na, nb)), b, c


@pytest.mark.parametrize("sector", HOST_SECTORS)
def test_host_result_methods_against_the_reference(sector):
    n, na, nb = sector
    res, b, c = host_result(sector, 7 * n + na)
    signs = fci_gpu.interleave_signs(n, na, nb).ravel()
    tol = rref.rdm_tolerance(b.size, b, c)
    want = rref.rdm12(n, (na, nb), c * signs)
    got = res.rdm12(0)
    assert got[0].shape == (2, n, n) and got[1].shape == (3, n, n, n, n)
    assert np.all(np.abs(got[0] - want[0]) <= tol) and np.all(np.abs(got[1] - want[1]) <= tol)
    assert np.all(np.abs(res.rdm1(0) - want[0]) <= tol)
    want = rref.rdm12(n, (na, nb), c * signs, b * signs)  # bra: root 1, ket: root 0
    got = res.trans_rdm12(1, 0)
    assert np.all(np.abs(got[0] - want[0]) <= tol) and np.all(np.abs(got[1] - want[1]) <= tol)
    assert np.all(np.abs(res.trans_rdm1(1, 0) - want[0]) <= tol)
    occ = res.natural_occupations(0)
    assert occ.shape == (n,) and np.all(np.diff(occ) <= 0) and abs(occ.sum() - (na + nb)) <= 2 * n * tol + 1e-14


@pytest.mark.parametrize("sector", [(4, 4, 1), (5, 3, 2), (6, 3, 3)])
def test_host_energy_identity(sector):
    """<i|H|j> from the densities of the host solver's eigenvectors: the eigenvalue for i = j, zero otherwise.  eigh leaves
    the eigenpairs within dim eps |H| and |H| <= |constant| + the 1-norm of the integrals."""
    n, na, nb = sector
    ham = ref.synthetic(n, 100 * n + 10 * na + nb)
    res = fci.ground_state(*ham.to_dense(), (na, nb), nroots=2)
    assert res.norb == n and res.nelec == (na, nb)
    dim = len(res.determinants)
    tol = rref.rdm_tolerance(dim, [1.0], [1.0]) * integrals_norm(ham) + 10 * dim * ref.EPS * (abs(ham.constant) + integrals_norm(ham))
    e0 = fci_gpu.energy_from_rdm(ham, *res.rdm12(0))
    e1 = fci_gpu.energy_from_rdm(ham, *res.rdm12(1))
    e01 = fci_gpu.energy_from_rdm(ham, *res.trans_rdm12(0, 1), overlap=0.0)
    print(f"{sector}: E0 {res.energies[0]:.14f} from densities {e0:.14f}; <0|H|1> {e01:.2e}; bound {tol:.2e}")
    assert abs(e0 - res.energies[0]) <= tol and abs(e1 - res.energies[1]) <= tol and abs(e01) <= tol


def test_host_spin_square():
    """Single determinants in the host convention (spin orbital 2p + s): a0 a1 a2 b1 has S = 1; a0 b1 is half singlet,
    half triplet; and the formula of fci_gpu.spin_square on the host object's dm2."""
    dets = host_result((4, 3, 1), 0)[0].determinants
    ci = np.zeros((len(dets), 1))
    ci[dets.index(0b00011101), 0] = 1.0
    assert fci.FCIResult(0.0, [0.0], ci, dets, norb=4, nelec=(3, 1)).spin_square() == 2.0
    n, nelec = 2, (1, 1)
    res = fci.ground_state(*ref.synthetic(2, 3).to_dense(), nelec)
    ci = np.zeros((4, 1))
    ci[res.determinants.index(0b1001), 0] = 1.0  # alpha in orbital 0, beta in orbital 1
    mixed = fci.FCIResult(0.0, [0.0], ci, res.determinants, norb=n, nelec=nelec)
    assert mixed.spin_square() == 1.0 and fci_gpu.spin_square(mixed.rdm12()[1], nelec) == 1.0
    closed = np.zeros((4, 1))
    closed[res.determinants.index(0b0011), 0] = 1.0
    assert fci.FCIResult(0.0, [0.0], closed, res.determinants, norb=n, nelec=nelec).spin_square() == 0.0


def test_old_style_result_still_works_and_says_what_is_missing():
    res = fci.FCIResult(-1.0, np.array([-1.0]), np.ones((1, 1)), [0b11])
    assert res.e_tot == -1.0 and res.converged is True and res.determinants == [0b11] and res.norb is None and res.nelec is None
    for call in (res.rdm1, res.rdm12, res.spin_square, res.natural_occupations, lambda: res.trans_rdm1(0, 0),
                 lambda: res.trans_rdm12(0, 0)):
        with pytest.raises(ValueError, match="without norb and nelec"):
            call()
    full = fci.FCIResult(-1.0, np.array([-1.0]), np.ones((1, 1)), [0b11], norb=1, nelec=(1, 1))
    with pytest.raises(ValueError, match="root 1"):
        full.rdm12(1)
    with pytest.raises(ValueError, match="root -1"):
        full.trans_rdm1(0, -1)


# ---------------------------------------------------------------- plan, ABI, refusals
def test_memory_plan_rdm_arithmetic():
    """Water / 6-31G by hand: n = 13, (5, 5): 1287 strings per spin, 2 n^2 + 1 = 339 generators and the vector."""
    plan = fci_gpu.memory_plan_rdm(13, 5, 5, capacity=10**12)
    assert fci_gpu.default_slabs(13) == 29 and plan["slabs"] == 29  # 3 x 3 tiles of 128: 29 x 9 = 261 >= 256 workgroups
    assert plan["ndet"] == 1287 * 1287 and plan["chunk_rows"] == 1287 and plan["chunks"] == 1
    assert plan["vectors"] == 8 * 1287 * 1287
    assert plan["tables"] == 4 * 2 * 1287 * 169
    assert plan["direct"] == 8 * 1287 * 338
    assert plan["output"] == 8 * (338 + 3 * 13**4 + 1)
    assert plan["slab_partials"] == 8 * 29 * 339 * 339
    assert plan["d"] == 8 * 339 * 1287 * 1287
    assert plan["total"] == sum(plan[k] for k in ("vectors", "tables", "direct", "output", "slab_partials", "d"))
    trans = fci_gpu.memory_plan_rdm(13, 5, 5, transition=True, chunk_rows=100, slabs=4)
    assert trans["vectors"] == 2 * plan["vectors"] and trans["d"] == 2 * 8 * 339 * 100 * 1287 and trans["chunks"] == 13
    assert trans["slab_partials"] == 8 * 4 * 339 * 339 and trans["slabs"] == 4
    direct = fci_gpu.memory_plan_rdm(13, 5, 5, direct_only=True)
    assert direct["d"] == 0 and direct["slab_partials"] == 0 and direct["output"] == 8 * 338
    assert direct["total"] == direct["vectors"] + direct["tables"] + direct["direct"] + direct["output"]
    # n = 16 (8, 8): one D of all 12870 rows is 680 GB; the chunk shrinks to what is left of 0.9 x 288 GB
    big = fci_gpu.memory_plan_rdm(16, 8, 8)
    fixed = big["vectors"] + big["tables"] + big["direct"] + big["output"] + big["slab_partials"]
    per_row = 8 * 513 * 12870
    assert big["slabs"] == 11 and big["chunk_rows"] == (int(0.9 * fci_gpu.DEVICE_BYTES) - fixed) // per_row
    assert 1 <= big["chunk_rows"] < 12870 and big["total"] <= 0.9 * fci_gpu.DEVICE_BYTES
    assert big["chunk_rows"] * 12870 < 2**31
    assert fci_gpu.memory_plan_rdm(16, 8, 8, capacity=10**9)["chunk_rows"] == 1  # never fewer than one row
    assert fci_gpu.default_slabs(1) == 256 and fci_gpu.default_slabs(16) == 11 and fci_gpu.default_slabs(31) == 1
    for bad in ({"chunk_rows": 0}, {"chunk_rows": 1288}, {"slabs": 0}, {"slabs": 65536}):
        with pytest.raises(ValueError):
            fci_gpu.memory_plan_rdm(13, 5, 5, **bad)


def test_new_symbols_are_declared_and_bound():
    from ctypes import c_int, c_int64, c_void_p

    assert _nbx.SIGNATURES["nbx_fci_rdm_finish"] == (c_int, [c_void_p, c_int64, c_int64] + [c_void_p] * 4)
    assert _nbx.SIGNATURES["nbx_fci_rdm1"] == (c_int, [c_void_p, c_int64, c_int64, c_int64] + [c_void_p] * 6)
    assert ("int nbx_fci_rdm_finish(nbx_ctx* ctx, int64_t n, int64_t slabs, const double* d_graw, double* d_dm1, "
            "double* d_dm2,") in HEADER
    assert "int nbx_fci_rdm1(nbx_ctx* ctx, int64_t n, int64_t n_alpha_str, int64_t n_beta_str, const int* d_link_a," in HEADER
    if not _nbx.LIB_PATH.exists():
        pytest.fail(f"{_nbx.LIB_PATH} is not built; run __graft_entry__.build()")
    lib = _nbx.load_library()
    assert hasattr(lib, "nbx_fci_rdm_finish") and hasattr(lib, "nbx_fci_rdm1")
    assert callable(HipBackend.fci_rdm_finish) and callable(HipBackend.fci_rdm1)


class NoLaunch:
    """A backend that can only say how much memory is free: anything else would be a launch or an allocation."""

    def __init__(self, free):
        self._free = free

    def free_bytes(self):
        return self._free


def test_refusals_come_before_any_launch(be):
    with pytest.raises(NbedDriverError, match="24310 beta strings per row exceed the 13312 the kernels stage in LDS"):
        fci_gpu.RdmBuilder(NoLaunch(1 << 50), 17, (8, 8))
    with pytest.raises(NbedDriverError, match=r"densities of 13 orbitals with \(5, 5\) electrons, 1656369 determinants, need "
                                              r"\d+ bytes .* 1000000 are free"):
        fci_gpu.RdmBuilder(NoLaunch(10**6), 13, (5, 5))
    with pytest.raises(ValueError, match="chunk_rows"):
        fci_gpu.RdmBuilder(NoLaunch(1 << 50), 5, (3, 2), chunk_rows=11)
    with pytest.raises(ValueError, match="electrons per spin"):
        fci_gpu.RdmBuilder(NoLaunch(1 << 50), 5, (6, 2))
    # a planned D that fits, a second one that no longer does
    class Tight(EmulatedRdmKernels):
        free = fci_gpu.memory_plan_rdm(5, 3, 2, chunk_rows=10, slabs=1)["total"]

        def free_bytes(self):
            return self.free

    tight = Tight(be.lib)
    rb = fci_gpu.RdmBuilder(tight, 5, (3, 2), chunk_rows=10, slabs=1)
    b, c = unit_vectors((10, 10), 1)
    assert np.all(np.isfinite(rb.rdm12(c)[1].numpy()))
    tight.free = 8 * 51 * 100 - 1  # (less than the second D alone)
    with pytest.raises(NbedDriverError, match="for 2 D of 10 alpha rows"):
        rb.rdm12(c, b)
    # the bra
    rb = fci_gpu.RdmBuilder(be, 5, (3, 2))
    for bad in (np.zeros((10, 9)), np.zeros(99), np.zeros((10, 10, 1))):
        with pytest.raises(ValueError, match="bra: a vector of shape"):
            rb.rdm12(c, bad)
        with pytest.raises(ValueError, match="bra: a vector of shape"):
            rb.rdm1(c, bad)
    with pytest.raises(ValueError, match="ket: a vector of shape"):
        fci_gpu.rdm12(np.zeros((9, 10)), 5, (3, 2), backend=be)
    with pytest.raises(NbedDriverError, match="direct_only"):
        fci_gpu.RdmBuilder(be, 5, (3, 2), direct_only=True).rdm12(c)
    # the root
    res = fci_gpu.FCIGpuResult(NoLaunch(0), [-1.0, -0.5], None, True, 1, [0.0, 0.0], fci_gpu.strings(5, 3), fci_gpu.strings(5, 2), 5)
    assert res.nelec == (3, 2)
    for call in (lambda: res.rdm12(2), lambda: res.rdm1(-1), lambda: res.trans_rdm1(0, 2), lambda: res.trans_rdm12(2, 0),
                 lambda: res.spin_square(5), lambda: res.natural_occupations(2), lambda: res.rdm12(0.0)):
        with pytest.raises(ValueError, match="this result holds 2 root"):
            call()


def test_result_methods_on_the_emulated_kernels(be):
    """FCIGpuResult's methods end to end on the host build: device copy, then the host copy uploaded again."""
    n, nelec = 5, (3, 2)
    ham = ref.synthetic(n, 532)
    res = fci_gpu.solve_spatial(ham, nelec, conv_tol=1e-10, nroots=2, backend=be)
    assert res.converged
    dm1, dm2 = res.rdm12(0)
    c = res.ci
    assert res._ci_dev is None
    want = rref.rdm12(n, nelec, c[0])
    tol = rref.rdm_tolerance(100, c[0], c[0])
    assert np.all(np.abs(dm1 - want[0]) <= tol) and np.all(np.abs(dm2 - want[1]) <= tol)
    again = res.rdm12(0)
    assert np.array_equal(again[0], dm1) and np.array_equal(again[1], dm2)
    want = rref.rdm12(n, nelec, c[1], c[0])
    got = res.trans_rdm12(0, 1)
    assert np.all(np.abs(got[0] - want[0]) <= tol) and np.all(np.abs(got[1] - want[1]) <= tol)
    assert np.all(np.abs(res.trans_rdm1(0, 1) - want[0]) <= tol) and np.all(np.abs(res.rdm1(0) - dm1) <= tol)
    e0 = fci_gpu.energy_from_rdm(ham, dm1, dm2, overlap=float(np.vdot(c[0], c[0])))
    # (the bound of test_gpu_fci_rdm.py's water test: the identity's, and the Ritz value's own rounding)
    bound = energy_tolerance(ham, nelec, c[0], c[0]) + 13 * 100 * ref.EPS * (abs(ham.constant) + integrals_norm(ham))
    assert abs(e0 - res.energies[0]) <= bound
    assert abs(res.natural_occupations(0).sum() - 5.0) <= 1e-12
    host = fci.ground_state(*ham.to_dense(), nelec)
    assert abs(res.spin_square(0) - host.spin_square(0)) <= 1e-7  # (two solvers' vectors)
