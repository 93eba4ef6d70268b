"""SCF objects built on a factor of the integrals (``eri_factor=``, nbed_amd/scf/gpu_scf.py) without a GPU: the routing
of jk_device / kernel() / huzinaga_scf and the argument checks, on a checker backend whose ``jk_factor`` is numpy.  The
factor is a numpy full-pivoting Cholesky decomposition of water / STO-3G's tensor from the numpy engine; the device
decomposition and HipBackend.jk_factor are tested in tests/test_gpu_eri_cholesky.py."""

import numpy as np
import pytest

from oracle_backend import OracleLookaheadBackend

from nbed_amd import integrals
from nbed_amd.dist import Shards
from nbed_amd.scf import GpuRHF, GpuUHF, GpuUKS, Mole, huzinaga_scf

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
TOL = 1e-8
U = 2.0 ** -53


class FactorCheckerBackend(OracleLookaheadBackend):
    """The checker backend plus HipBackend.jk_factor, by its definition."""

    def jk_factor(self, b, dm):
        self._count("jk_factor")
        bn = self._np(b)
        d = self._np(dm).reshape(-1, dm.shape[-1], dm.shape[-1])
        out = np.empty((1 + d.shape[0],) + d.shape[1:])
        out[0] = np.einsum("lpq,l->pq", bn, np.einsum("lpq,pq->l", bn, d.sum(axis=0)))
        for x in range(d.shape[0]):
            out[1 + x] = np.einsum("lpq,qr,lrs->ps", bn, d[x], bn, optimize=True)
        return self.asarray(out)


def full_pivoting_cholesky(v, tol):
    """(rank, n^2) with v ~ L^T L and the residual's diagonal <= tol: the textbook algorithm, one column per step."""
    d = np.diag(v).copy()
    vecs = []
    while d.max() > tol:
        k = int(np.argmax(d))
        col = v[:, k] - sum(l * l[k] for l in vecs)
        vecs.append(col / np.sqrt(d[k]))
        d -= vecs[-1] ** 2
    return np.array(vecs)


@pytest.fixture(scope="module")
def water():
    m = integrals.molecule_integrals(WATER, "sto-3g", engine="numpy")
    n = m["nao"]
    v = m["eri"].reshape(n * n, n * n)
    b = full_pivoting_cholesky(v, TOL).reshape(-1, n, n)
    assert 1 <= b.shape[0] <= n * (n + 1) // 2 and np.abs(v - np.einsum("lx,ly->xy", *(b.reshape(-1, n * n),) * 2)).max() <= TOL
    np.testing.assert_allclose(b, b.transpose(0, 2, 1), rtol=0, atol=1e-14)
    m["factor"] = 0.5 * (b + b.transpose(0, 2, 1))
    return m


def _objects(cls, m, be):
    n = m["nao"]
    mol = lambda: Mole(n, (5, 5), e_nuc=m["e_nuc"])  # noqa: E731
    dense = cls(mol(), m["S"], m["hcore"], m["eri"], backend=be)
    factor = cls(mol(), m["S"], m["hcore"], backend=be, eri_factor=m["factor"])

    def forbidden():
        raise AssertionError("eri_device() was called on an object built on a factor")

    factor.eri_device = forbidden
    return dense, factor


def test_jk_device_routes_to_jk_factor_and_agrees_with_the_dense_object(water):
    be = FactorCheckerBackend()
    dense, factor = _objects(GpuUHF, water, be)
    n = water["nao"]
    rng = np.random.default_rng(95)
    c = np.stack([np.linalg.qr(rng.standard_normal((n, n)))[0] for _ in range(2)])
    dms = np.stack([c[0][:, :5] @ c[0][:, :5].T, c[1][:, :4] @ c[1][:, :4].T])
    want = be.to_host(dense.jk_device(be.asarray(dms)))
    got = be.to_host(factor.jk_device(be.asarray(dms)))
    assert be.calls["jk_factor"] == 1 and got.shape == want.shape == (3, n, n)
    vmax = np.einsum("pqpq->pq", water["eri"]).max()
    eps = TOL + 2e-13 + 2 * (water["factor"].shape[0] + 2) * U * vmax
    scale = np.abs(want).max()
    for x, weight in enumerate((np.abs(dms.sum(0)).sum(), np.abs(dms[0]).sum(), np.abs(dms[1]).sum())):
        assert np.abs(got[x] - want[x]).max() <= eps * weight + 1e-12 * scale
    assert factor.eri_packed_device() is None and factor.eri_rs_device() is None and factor.dts_device() is None
    assert not factor.fused_fock_available(be.zeros((2, n, n)))


def test_kernel_and_huzinaga_scf_run_step_by_step_without_the_tensor(water, monkeypatch):
    """On a backend that HAS the one-call-per-cycle entry points (mu_cycle, huz_cycle), which read the tensor."""
    monkeypatch.delenv("NBED_CYCLE_CALL", raising=False)
    be = FactorCheckerBackend()
    assert hasattr(be, "mu_cycle") and hasattr(be, "huz_cycle")
    dense, factor = _objects(GpuUHF, water, be)
    for mf in (dense, factor):
        mf.conv_tol = 1e-10
        mf.kernel()
        assert mf.converged
    assert dense.kernel_info is not None and factor.kernel_info is None  # (only the one-call loop records it)
    assert be.calls["jk_factor"] > 3
    sum_d = max(np.abs(mf.make_rdm1()).sum() for mf in (dense, factor))
    vmax = np.einsum("pqpq->pq", water["eri"]).max()
    eps = TOL + 2e-13 + 2 * (water["factor"].shape[0] + 2) * U * vmax
    assert abs(factor.e_tot - dense.e_tot) <= 0.75 * eps * sum_d ** 2 + 1e-9
    assert -75.1 < dense.e_tot < -74.8
    n = water["nao"]
    _, factor = _objects(GpuUHF, water, be)
    factor.max_cycle = 3
    before = be.calls["jk_factor"]
    hist = []
    c, e, d, hz, conv = huzinaga_scf(factor, np.zeros((2, n, n)), np.zeros((2, n, n)), history=hist)
    assert len(hist) == 3 and be.calls["jk_factor"] > before and abs(np.trace(d[0] @ water["S"]) - 5) < 1e-8
    _, rhf = _objects(GpuRHF, water, be)
    rhf.max_cycle, rhf.conv_tol = 60, 1e-10
    c, e, d, hz, conv = huzinaga_scf(rhf, np.zeros((n, n)), np.zeros((n, n)), dm_conv_tol=1e-8)
    assert conv and abs(rhf.energy_tot(d) - dense.e_tot) <= 0.75 * eps * np.abs(d).sum() ** 2 + 1e-8


def test_argument_checks(water):
    be = FactorCheckerBackend()
    n = water["nao"]
    args = (Mole(n, (5, 5)), water["S"], water["hcore"])
    with pytest.raises(ValueError, match="not both"):
        GpuUHF(*args, water["eri"], backend=be, eri_factor=water["factor"])
    with pytest.raises(ValueError, match="not both"):
        GpuRHF(*args, backend=be, eri_factor=water["factor"], eri_packed=be.zeros(4))
    with pytest.raises(ValueError, match="single rank"):
        GpuUKS(*args, backend=be, eri_factor=water["factor"], shards=Shards(n, world=2, rank=1))
    with pytest.raises(ValueError, match=r"expected \(naux, 7, 7\)"):
        GpuUHF(*args, backend=be, eri_factor=water["factor"][:, :, :5])
    with pytest.raises(ValueError, match="no jk_factor"):
        GpuUHF(*args, backend=OracleLookaheadBackend(), eri_factor=water["factor"])
    mf = GpuUHF(*args, backend=be, eri_factor=water["factor"])
    with pytest.raises(ValueError, match="without two-electron integrals"):
        mf.eri_device()
    # objects built without a factor are what they were
    assert GpuUHF(*args, water["eri"], backend=be)._eri_factor_d is None


def test_column_list_bookkeeping_under_the_sanitizers(tmp_path):
    """The host side of a column call (quartet lists, column offsets and pivots; nbx_eri::build_column_lists) in a
    stand-alone program built with AddressSanitizer and UBSan (tests/native/eri_cd_lists_check.hip): no device, no Python."""
    import shutil
    import subprocess
    from pathlib import Path

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.fail("no hipcc: the library this suite tests cannot have been built without it")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "eri_cd_lists_check"
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", f"-I{root / 'include'}", f"-I{root / 'nbed_amd' / 'csrc'}",
                    str(root / "tests" / "native" / "eri_cd_lists_check.hip"), "-pthread", "-o", str(exe)], check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("bad=0") == 6, r.stdout
