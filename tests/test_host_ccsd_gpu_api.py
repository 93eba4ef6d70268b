"""The host side of the device CCSD (nbed_amd/ccsd_gpu.py) that needs no GPU: import, the memory plan, the
contraction planner on a numpy stand-in, and the driver's routing between the two solvers."""

import numpy as np
import pytest

from oracle_backend import OracleBackend
from synthetic_provider import SyntheticProvider
from test_host_driver import config

from nbed_amd import ccsd, ccsd_gpu, nbed
from nbed_amd.exceptions import NbedDriverError


def test_imports_without_a_gpu_and_refuses_a_host_backend():
    assert callable(ccsd_gpu.solve) and callable(ccsd_gpu.solve_spatial)
    with pytest.raises(NbedDriverError, match="HipBackend"):
        ccsd_gpu.solve_spatial((0.0, np.zeros((2, 2, 2)), np.zeros((3, 2, 2, 2, 2))), [0, 1], backend=OracleBackend())


@pytest.mark.parametrize("no,nv", [(10, 38), (26, 230)])
def test_memory_plan_is_the_sum_of_the_blocks(no, nv):
    sizes = ccsd_gpu.block_sizes(no, nv)
    pairs = nv * (nv - 1) // 2
    want = {"oovv": no * no * nv * nv, "oooo": no**4, "ovvo": no * no * nv * nv, "ovov": no * no * nv * nv,
            "ooov": no**3 * nv, "ovvv": no * nv**3, "vvvo": no * nv**3, "ovoo": no**3 * nv, "vvvv": pairs * pairs}
    assert sizes == want
    plan = ccsd_gpu.memory_plan(no, nv)
    assert plan["blocks"] == 8 * sum(want.values())
    assert plan["spatial"] == 8 * 3 * ((no + nv) // 2) ** 4
    nvec = no * nv + (no * nv) ** 2
    assert plan["amplitudes"] >= 8 * (2 + 2 * 6) * nvec
    assert plan["total"] == plan["blocks"] + plan["spatial"] + plan["amplitudes"] + plan["work"]
    if (no, nv) == (26, 230):  # octane / 6-31G*: <vv||vv> over packed pairs is 5.5 GB, a sixteenth of the dense block
        assert 8 * want["vvvv"] == 5548257800 and plan["total"] < 64e9


def test_dense_input_must_have_the_spin_block_form():
    rng = np.random.default_rng(0)
    n = 2
    two = rng.standard_normal((3, n, n, n, n))
    h2 = np.zeros((2 * n,) * 4)
    h2[0::2, 0::2, 0::2, 0::2], h2[1::2, 1::2, 1::2, 1::2] = two[0], two[1]
    h2[0::2, 1::2, 1::2, 0::2], h2[1::2, 0::2, 0::2, 1::2] = two[2], two[2].transpose(1, 0, 3, 2)
    h1 = np.zeros((2 * n, 2 * n))
    h1[0::2, 0::2], h1[1::2, 1::2] = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    one, back = ccsd_gpu.spatial_from_dense(h1, h2)
    assert np.array_equal(back, two) and np.array_equal(one[1], h1[1::2, 1::2])
    h2[0, 1, 0, 1] = 0.3  # an (a, b, a, b) entry: not a Hamiltonian build() can return
    with pytest.raises(ValueError, match="spin-block"):
        ccsd_gpu.spatial_from_dense(h1, h2)


class _NumpyOps:
    """Just enough of a backend for ``Contractor``: permute4 and gemm_raw in numpy."""

    def empty(self, shape):
        import torch

        return torch.full(tuple(shape), float("nan"), dtype=torch.float64)

    def permute4(self, x, perm, alpha=1.0, beta=0.0, out=None):
        import torch

        v = alpha * np.transpose(x.numpy(), perm)
        if out is None:
            return torch.from_numpy(np.ascontiguousarray(v))
        o = out.numpy().reshape(v.shape)
        o[...] = v if beta == 0.0 else v + beta * o
        return out

    def gemm_raw(self, ta, tb, m, n, k, alpha, a, lda, sa, b, ldb, sb, beta, c, ldc, sc, batch):
        assert lda == (k if ta == "N" else m) and ldb == (n if tb == "N" else k) and ldc == n and batch == 1
        am = a.numpy().reshape(m, k) if ta == "N" else a.numpy().reshape(k, m).T
        bm = b.numpy().reshape(k, n) if tb == "N" else b.numpy().reshape(n, k).T
        cm = c.numpy().reshape(m, n)
        cm[...] = alpha * (am @ bm) if beta == 0.0 else alpha * (am @ bm) + beta * cm


@pytest.mark.parametrize("spec", ["mf,mafe->ae", "ijae,be->ijab", "imab,mj->ijab", "jnfb,mnef->mbej", "ma,imbj->ijab",
                                  "ie,abej->ijab", "mnae,nmie->ia", "ijef,maef->ijma", "ie,me->mi"])
def test_contraction_planner_matches_einsum(spec):
    import torch

    rng = np.random.default_rng(3)
    ext = dict(zip("ijmnabef", (3, 4, 2, 5, 6, 3, 4, 2)))
    ins, out = spec.split("->")
    la, lb = ins.split(",")
    a, b = (rng.standard_normal(tuple(ext[ch] for ch in letters)) for letters in (la, lb))
    c = ccsd_gpu.Contractor(_NumpyOps())
    got = c(spec, torch.from_numpy(a), torch.from_numpy(b), -0.5).numpy()
    want = -0.5 * np.einsum(spec, a, b)
    assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-13)
    base = rng.standard_normal(want.shape)
    acc = torch.from_numpy(base.copy())
    c(spec, torch.from_numpy(a), torch.from_numpy(b), 2.0, acc, 1.0)
    assert np.allclose(acc.numpy(), base + 2.0 * np.einsum(spec, a, b), rtol=0, atol=1e-13)


def test_host_only_backend_still_raises_past_the_cap(monkeypatch):
    monkeypatch.delenv("NBED_CCSD_SOLVER", raising=False)
    try:
        import pyscf  # noqa: F401

        pytest.skip("PySCF installed: its CCSD runs")
    except ImportError:
        pass
    assert 2 * 24 > ccsd.MAX_SPIN_ORBITALS
    for mode in (None, "device", "host"):
        if mode:
            monkeypatch.setenv("NBED_CCSD_SOLVER", mode)
        with pytest.raises(NbedDriverError, match="PySCF"):
            nbed(config(run_ccsd_emb=True, virtual_localization="disable"), provider=SyntheticProvider(24, (5, 5), 5),
                 backend=OracleBackend())


def test_unknown_solver_switch_is_refused(monkeypatch):
    monkeypatch.setenv("NBED_CCSD_SOLVER", "gpu")
    with pytest.raises(NbedDriverError, match="NBED_CCSD_SOLVER='gpu'.*'auto', 'host' or 'device'"):
        nbed(config(run_ccsd_emb=True, virtual_localization="disable"), provider=SyntheticProvider(14, (5, 5), 5),
             backend=OracleBackend())
