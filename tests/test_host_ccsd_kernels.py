"""csrc/ccsd.hip compiled for the host (tests/native/ccsd_host_shim.h runs a launch thread by thread) so that the index
arithmetic of its grid-stride kernels -- spin selection and the four-term antisymmetriser of the gather, pair packing,
tau, the amplitude update -- is checked without a GPU, by the kernel tests of tests/test_gpu_ccsd.py themselves, and the
device solver's algebra (nbed_amd/ccsd_gpu.py on these kernels, products and tiled permutes in numpy) against the host
solver.  The tiled permute and the GEMMs are exercised only by the GPU suite."""

import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle_backend import OracleBackend
from test_gpu_ccsd import (  # noqa: F401  (collected here with this module's ``be``: the emulated kernels, no gpu mark)
    METHYL,
    occupied_of,
    test_block_gather,
    test_pair_pack_unpack,
    test_permute_accumulates,
    test_tau_and_update,
)

from nbed_amd import NbedConfig, _nbx, ccsd, ccsd_gpu
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.ham_builder import HamiltonianBuilder

REPO = Path(__file__).resolve().parent.parent
KERNELS = ("nbx_ccsd_gather", "nbx_ccsd_fock", "nbx_permute4", "nbx_pair_pack", "nbx_pair_unpack", "nbx_ccsd_tau",
           "nbx_ccsd_update")


class EmulatedKernels:
    """The HipBackend methods ``ccsd_gpu`` uses, on torch CPU tensors: csrc/ccsd.hip's kernels from the host build,
    ``gemm_raw`` / ``dots`` / ``lincomb`` and the tiled permute in numpy.  ``empty`` is NaN-filled."""

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

    def to_host(self, a):
        return a.numpy() if isinstance(a, self.torch.Tensor) else np.asarray(a)

    def copy(self, a):
        return a.clone()

    def index_array(self, idx, limit):
        h = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        assert h.size == 0 or (h.min() >= 0 and h.max() < limit)
        return self.torch.from_numpy(h.copy())

    def read_scalars(self, d):
        return d.numpy().copy()

    def free_bytes(self):
        return 1 << 40

    def dots(self, x, vecs):
        return vecs.numpy().reshape(vecs.shape[0], -1) @ x.numpy().ravel()

    def lincomb(self, coef, vecs, out=None):
        out.numpy()[...] = np.tensordot(np.asarray(coef, dtype=float), vecs.numpy(), 1)
        return out

    def gemm_raw(self, ta, tb, m, n, k, alpha, a, lda, sa, b, ldb, sb, beta, c, ldc, sc, batch):
        assert lda == (k if ta == "N" else m) and ldb == (n if tb == "N" else k) and ldc == n and batch == 1
        am = a.numpy().ravel()[: m * k].reshape((m, k) if ta == "N" else (k, m))
        bm = b.numpy().ravel()[: k * n].reshape((k, n) if tb == "N" else (n, k))
        prod = alpha * ((am if ta == "N" else am.T) @ (bm if tb == "N" else bm.T))
        cm = c.numpy().reshape(m, n)
        cm[...] = prod if beta == 0.0 else prod + beta * cm

    # the wrappers of nbed_amd/backend.py, on the host build
    def ccsd_gather(self, two_body, i1, i2, i3, i4, pack_first=False, pack_last=False):
        n = two_body.shape[-1]
        n1, n2, n3, n4 = (int(i.numel()) for i in (i1, i2, i3, i4))
        rows = (n1 * (n1 - 1) // 2,) if pack_first else (n1, n2)
        cols = (n3 * (n3 - 1) // 2,) if pack_last else (n3, n4)
        out = self.empty(rows + cols)
        self._call("nbx_ccsd_gather", n, self._p(two_body), self._p(i1), n1, self._p(i2), n2, self._p(i3), n3, self._p(i4),
                   n4, int(pack_first), int(pack_last), self._p(out))
        return out

    def ccsd_fock(self, two_body, h1, occ):
        n = two_body.shape[-1]
        out = self.empty((2 * n, 2 * n))
        self._call("nbx_ccsd_fock", n, self._p(two_body), self._p(h1), self._p(occ), int(occ.numel()), self._p(out))
        return out

    def permute4(self, x, perm, alpha=1.0, beta=0.0, out=None):
        nd = x.dim()
        if out is None:
            out = self.empty(tuple(int(x.shape[p]) for p in perm))
        if perm[-1] != nd - 1:  # the tiled kernel exchanges data across a barrier: numpy here
            o = out.numpy().reshape(tuple(int(x.shape[p]) for p in perm))
            v = alpha * np.transpose(x.numpy(), perm)
            o[...] = v if beta == 0.0 else v + beta * o
            return out
        ext = [1] * (4 - nd) + [int(s) for s in x.shape]
        p4 = list(range(4 - nd)) + [int(p) + 4 - nd for p in perm]
        self._call("nbx_permute4", (ctypes.c_int64 * 4)(*ext), (ctypes.c_int * 4)(*p4), float(alpha), self._p(x),
                   float(beta), self._p(out))
        return out

    def pair_pack(self, x, lead, n, trail):
        out = self.empty((lead, n * (n - 1) // 2, trail))
        self._call("nbx_pair_pack", lead, n, trail, self._p(x), self._p(out))
        return out

    def pair_unpack(self, packed, lead, n, trail, alpha=1.0, beta=0.0, out=None):
        if out is None:
            out = self.empty((lead, n, n, trail))
        self._call("nbx_pair_unpack", lead, n, trail, float(alpha), self._p(packed), float(beta), self._p(out))
        return out

    def ccsd_tau(self, t1, t2, c_t2, c_direct, c_exchange, packed=False):
        no, nv = int(t1.shape[0]), int(t1.shape[1])
        out = self.empty((no * (no - 1) // 2, nv * (nv - 1) // 2)) if packed else self.empty((no, no, nv, nv))
        self._call("nbx_ccsd_tau", no, nv, self._p(t1), self._p(t2), float(c_t2), float(c_direct), float(c_exchange),
                   int(packed), self._p(out))
        return out

    def ccsd_update(self, no, nv, r, t_old, eo, ev, t_new, err, maxerr):
        self._call("nbx_ccsd_update", no, nv, self._p(r), self._p(t_old), self._p(eo), self._p(ev), self._p(t_new),
                   self._p(err), self._p(maxerr))
        maxerr.numpy()[0] = np.abs(err.numpy()).max()  # (the workgroup reduction needs real wavefronts)


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host form of csrc/ccsd.hip")
    work = tmp_path_factory.mktemp("ccsd_host")
    shutil.copy(REPO / "nbed_amd" / "csrc" / "ccsd.hip", work / "ccsd_host.cpp")
    shutil.copy(REPO / "tests" / "native" / "ccsd_host_shim.h", work / "nbx_common.h")  # (found before csrc's: same directory)
    subprocess.run([gxx, "-O1", "-std=c++17", "-fPIC", "-shared", f"-I{work}", str(work / "ccsd_host.cpp"), "-o",
                    str(work / "libccsd_host.so")], check=True, capture_output=True, timeout=300)
    lib = ctypes.CDLL(str(work / "libccsd_host.so"))
    for name in KERNELS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _nbx.SIGNATURES[name]
    return EmulatedKernels(lib)


def test_solver_on_emulated_kernels_follows_the_host_solver(be):
    """CH3 / STO-3G (5 + 4 electrons, 16 spin orbitals): three cycles and the converged energy."""
    chk = OracleBackend()
    cfg = NbedConfig(geometry=METHYL, n_active_atoms=1, basis="sto-3g", xc_functional="hf", convergence=1e-11, spin=1)
    hf = BuiltinHFProvider(chk).global_hf(cfg)
    const, h1, h2 = HamiltonianBuilder(hf, hf.energy_nuc(), backend=chk).build()
    occ = occupied_of(hf)
    for kw in (dict(max_cycle=3), dict(conv_tol=1e-11)):
        host = ccsd.solve(const, h1, h2, occ, **kw)
        dev = ccsd_gpu.solve(const, h1, h2, occ, backend=be, **kw)
        assert dev.iterations == host.iterations and dev.converged == host.converged
        assert np.max(np.abs(dev.t1 - host.t1)) < 1e-10 and np.max(np.abs(dev.t2 - host.t2)) < 1e-10
        assert abs(dev.e_corr - host.e_corr) < 1e-9 and abs(dev.e_hf - host.e_hf) < 1e-10
    assert host.converged and abs(host.e_corr - (-0.0576797669)) < 1e-8
