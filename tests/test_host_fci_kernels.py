"""csrc/fci.hip compiled for the host (tests/native/fci_host_shim.h runs every workgroup with one thread) so that the
index arithmetic of its kernels -- the generator matrix, link-table lookups, chunk offsets, the order of the sums, the
diagonal -- and the Davidson solver on top of them (nbed_amd/fci_gpu.py, the product in numpy) are checked without a
GPU, by the small-sector tests of tests/test_gpu_fci.py themselves (against tests/fci_reference.py and the host solver)
and a few more.  LDS staging across real wavefronts, the GEMM and the large sectors are exercised only by the GPU
suite."""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fci_reference as ref
from oracle_backend import OracleBackend
from test_gpu_fci import (  # noqa: F401  (collected here with this module's ``be``: the emulated kernels, no gpu mark)
    small,
    test_diagonal,
    test_running_out_of_cycles_returns_the_current_ritz_pair,
    test_sigma_every_element,
    test_sigma_sampled_rows_n9,
    test_solver_matches_the_host_solver_synthetic,
    test_solver_matches_the_host_solver_water_sto3g,
)

from nbed_amd import NbedConfig, _nbx, fci_gpu
from nbed_amd.backend import HipBackend
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.ham_builder import HamiltonianBuilder

REPO = Path(__file__).resolve().parent.parent
KERNELS = ("nbx_fci_gmat", "nbx_fci_gather", "nbx_fci_scatter", "nbx_fci_diag", "nbx_fci_precond")


class EmulatedKernels:
    """The HipBackend methods ``fci_gpu`` uses, on torch CPU tensors: csrc/fci.hip's kernels from the host build,
    ``gemm_raw`` / ``dots`` / ``lincomb`` / ``axpby`` in numpy.  ``empty`` is NaN-filled."""

    def __init__(self, lib):
        import torch

        self.torch, self.lib = torch, lib
        self._ctx = ctypes.c_int(0)
        self.ctx = ctypes.c_void_p(ctypes.addressof(self._ctx))

    def _call(self, name, *args):
        assert getattr(self.lib, name)(self.ctx, *args) == 0, name

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr())

    def empty(self, *shape):
        size = shape[0] if len(shape) == 1 and not isinstance(shape[0], int) else shape
        return self.torch.full(tuple(size), float("nan"), dtype=self.torch.float64)

    def asarray(self, a):
        if isinstance(a, self.torch.Tensor):
            return a.contiguous()
        return self.torch.from_numpy(np.array(a, dtype=np.float64, order="C"))

    def int_array(self, a):
        return self.torch.from_numpy(np.array(a, dtype=np.int32, order="C"))

    def to_host(self, a):
        return a.numpy() if isinstance(a, self.torch.Tensor) else np.asarray(a)

    def read_scalars(self, d):
        return d.numpy().copy()

    def free_bytes(self):
        return 1 << 40

    def synchronize(self):
        pass

    def dots(self, x, vecs):
        return vecs.numpy().reshape(vecs.shape[0], -1) @ x.numpy().ravel()

    def lincomb(self, coef, vecs, out=None):
        assert len(coef) == vecs.shape[0]
        out.numpy()[...] = np.tensordot(np.asarray(coef, dtype=float), vecs.numpy(), 1).reshape(out.shape)
        return out

    def axpby(self, a, x, b, y):
        y.numpy()[...] = a * x.numpy() + b * y.numpy()
        return y

    def gemm_raw(self, ta, tb, m, n, k, alpha, a, lda, sa, b, ldb, sb, beta, c, ldc, sc, batch):
        assert (ta, tb) == ("N", "N") and lda == k and ldb == n and ldc == n and batch == 1 and beta == 0.0
        c.numpy().reshape(m, n)[...] = alpha * (a.numpy().reshape(m, k) @ b.numpy().reshape(k, n))


for _name in ("fci_gmat", "fci_gather", "fci_scatter", "fci_diag", "fci_precond"):  # the wrappers of nbed_amd/backend.py
    setattr(EmulatedKernels, _name, getattr(HipBackend, _name))


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host form of csrc/fci.hip")
    work = tmp_path_factory.mktemp("fci_host")
    shutil.copy(REPO / "nbed_amd" / "csrc" / "fci.hip", work / "fci_host.cpp")
    shutil.copy(REPO / "tests" / "native" / "fci_host_shim.h", work / "nbx_common.h")  # (found before csrc's: same directory)
    subprocess.run([gxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-DNBX_FCI_PT=1024", f"-I{work}", str(work / "fci_host.cpp"),
                    "-o", str(work / "libfci_host.so")], check=True, capture_output=True, timeout=300)
    lib = ctypes.CDLL(str(work / "libfci_host.so"))
    for name in KERNELS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _nbx.SIGNATURES[name]
    return EmulatedKernels(lib)


@pytest.fixture(scope="module")
def molecules():
    """test_gpu_fci.py's fixture with the checker backend doing the Hartree-Fock and the four-index transform."""
    chk = OracleBackend()
    cache = {}

    def get(geometry, basis):
        if (geometry, basis) not in cache:
            cfg = NbedConfig(geometry=geometry, n_active_atoms=1, basis=basis, xc_functional="hf", convergence=1e-11)
            hf = BuiltinHFProvider(chk).global_hf(cfg)
            cache[(geometry, basis)] = (hf, HamiltonianBuilder(hf, hf.energy_nuc(), backend=chk).build_spatial())
        return cache[(geometry, basis)]

    return get


def test_small_basis_and_two_roots(be, small):
    """A basis of four vectors (collapsed again and again) reaches the same state; two roots converge together."""
    ham, mat, _ = small((6, 3, 3))
    w = np.linalg.eigvalsh(mat)
    dev = fci_gpu.solve_spatial(ham, (3, 3), conv_tol=1e-10, space=4, backend=be)
    assert dev.converged and dev.residual_norm < 1e-10 and abs(dev.e_tot - w[0]) < 1e-9
    two = fci_gpu.solve_spatial(ham, (3, 3), conv_tol=1e-9, nroots=2, backend=be)
    assert two.converged and np.max(np.abs(two.energies - w[:2])) < 1e-9 and two.ci.shape == (2, 20, 20)


def test_single_determinant_and_precond_guard(be):
    ham = ref.synthetic(3, 5)
    one = fci_gpu.solve_spatial(ham, (3, 0), backend=be)
    assert one.converged and one.iterations == 0 and abs(one.e_tot - ref.dense(ham, (3, 0))[0, 0]) < 1e-13
    r, d = be.asarray(np.array([1.0, -2.0, 3.0])), be.asarray(np.array([0.5, 1.0 - 1e-12, 1.0 + 1e-12]))
    out = be.empty(3)
    be.fci_precond(r, d, 1.0, 1e-8, out)
    assert np.allclose(out.numpy(), [1.0 / -0.5, -2.0 / -1e-8, 3.0 / 1e-8], rtol=1e-15)
