"""The four-index transform from a factor of the integrals on the device (csrc/ao2mo_factor.hip,
HipBackend.ao2mo_factor, HamiltonianBuilder on an SCF object built on a factor, BuiltinHFProvider(eri_engine="cholesky")).
References, bounds and their derivations: tests/ao2mo_factor_reference.py; every bound is held by numpy's own float64
against the same longdouble reference in tests/test_host_ao2mo_factor.py.

  1  stage 1 (the packed half transform), fused kernel and batched-GEMM route, against longdouble
  2  stage 3 (the pair expansion): exactly a gather, the four images of an integral one double
  3  the blocks against longdouble, both routes
  4  the same bits twice; nothing unwritten under NBED_POISON_EMPTY=1; refusals leave the outputs alone
  5  real molecules: the builder on a factor against the builder on the dense device tensor
  6  nbed(config) on the factor: the reference's known answers, the device route, no N^4 tensor, device CCSD
"""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import ao2mo_factor_reference as afr

from nbed_amd import NbedConfig, _nbx, integrals, nbed
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.ham_builder import HamiltonianBuilder
from nbed_amd.scf import GpuUHF, Mole

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@lru_cache(maxsize=None)
def _case(shape):
    b, cs = afr.inputs(shape)
    p_ref, mags = afr.half_reference(b, cs)
    blocks, bounds = afr.blocks_reference(b, cs)
    for a in (b, p_ref, mags, *cs, *blocks, *bounds):
        a.setflags(write=False)
    return b, cs, p_ref, mags, blocks, bounds


def _device_inputs(be, shape):
    """(b, ca, cb or None) on the device; the LAST coefficient matrix is a column slice of a wider one (ld = n + 3, two
    columns in: rows start at any 8-byte address)."""
    b, cs = _case(shape)[:2]
    big_n, n = shape[0], shape[1]
    dev = [be.asarray(c) for c in cs]
    wide = be.asarray(np.full((big_n, n + 3), 1e300))
    wide[:, 2:2 + n] = dev[-1]
    dev[-1] = wide[:, 2:2 + n]
    assert dev[-1].stride(0) == n + 3
    return be.asarray(b), dev[0], (dev[1] if len(dev) == 2 else None)


# ------------------------------------------------------------------------------------------ 1. stage 1
@pytest.mark.parametrize("half", ["fused", "gemm"])
@pytest.mark.parametrize("shape", afr.SHAPES, ids=str)
def test_half_transform_against_longdouble(be, shape, half):
    """|P - P_ref| <= 2 (N + 1) u (|C|^T |B_L| |C|)[i, j] on every element of P (nset, naux, n (n + 1) / 2)."""
    big_n, n, naux, nset = shape
    _, _, p_ref, mags, _, _ = _case(shape)
    b, ca, cb = _device_inputs(be, shape)
    p = be.to_host(be.ao2mo_factor_half(b, ca, cb, half=half))
    assert p.shape == (nset, naux, n * (n + 1) // 2) and np.all(np.isfinite(p))
    ratio = np.abs(p.astype(np.longdouble) - p_ref) / afr.half_bound(big_n, mags)
    print(f"{shape} {half}: worst |error| / bound = {float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0


# ------------------------------------------------------------------------------------------ 2. stage 3
@pytest.mark.parametrize("n", [1, 5, 17, 33])
def test_pair_expansion_is_a_gather(be, n):
    npair = n * (n + 1) // 2
    g = np.random.default_rng(n).standard_normal((npair, npair))  # (not symmetric: rows and columns must not be swapped)
    out = be.to_host(be.ao2mo_factor_expand(be.asarray(g), n))
    assert out.shape == (n, n, n, n)
    np.testing.assert_array_equal(out, afr.expand(g, n))
    for image in (out.transpose(1, 0, 2, 3), out.transpose(0, 1, 3, 2), out.transpose(1, 0, 3, 2)):
        np.testing.assert_array_equal(out, image)


# ------------------------------------------------------------------------------------------ 3. blocks
@pytest.mark.parametrize("half", ["fused", "gemm"])
@pytest.mark.parametrize("shape", afr.SHAPES, ids=str)
def test_blocks_against_longdouble(be, shape, half):
    """The stage-1 bound carried through the naux-term sum (tests/ao2mo_factor_reference.py) on every element of every
    block; (ij|kl) = (ji|kl) = (ij|lk) bit for bit, and aaaa, bbbb symmetric under (ij) <-> (kl) to rounding only."""
    big_n, n, naux, nset = shape
    _, _, _, _, ref, bounds = _case(shape)
    b, ca, cb = _device_inputs(be, shape)
    got = be.ao2mo_factor(b, ca, cb, half=half)
    got = [got] if nset == 1 else list(got)
    assert len(got) == (1 if nset == 1 else 3)
    for k, (g, r, bd) in enumerate(zip(got, ref, bounds)):
        g = be.to_host(g)
        assert g.shape == (n, n, n, n) and np.all(np.isfinite(g))
        ratio = np.abs(g.astype(np.longdouble) - r) / bd
        print(f"{shape} {half} block {k}: worst |error| / bound = {float(ratio.max()):.3f}")
        assert ratio.max() <= 1.0
        np.testing.assert_array_equal(g, g.transpose(1, 0, 2, 3))
        np.testing.assert_array_equal(g, g.transpose(0, 1, 3, 2))


# ------------------------------------------------------------------------------------------ 4. reproducibility and safety
def test_two_calls_give_the_same_bits(be):
    for shape in ((70, 13, 130, 2), (148, 40, 64, 2)):
        b, ca, cb = _device_inputs(be, shape)
        first = [be.to_host(x) for x in be.ao2mo_factor(b, ca, cb)]
        p_first = be.to_host(be.ao2mo_factor_half(b, ca, cb))
        be.release_workspaces()
        second = [be.to_host(x) for x in be.ao2mo_factor(b, ca, cb)]
        for x, y in zip(first, second):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(p_first, be.to_host(be.ao2mo_factor_half(b, ca, cb)))


def test_nothing_is_left_unwritten_under_poisoned_allocations(monkeypatch):
    """NBED_POISON_EMPTY=1: ``empty`` hands out NaN and every workspace starts from 0xff bytes; whatever a kernel does
    not write shows."""
    from nbed_amd.backend import HipBackend

    monkeypatch.setenv("NBED_POISON_EMPTY", "1")
    pbe = HipBackend()
    assert np.isnan(pbe.to_host(pbe.empty((3,)))).all()
    for shape in ((7, 1, 1, 1), (18, 5, 65, 2), (33, 33, 17, 1), (70, 13, 130, 2)):
        b, ca, cb = _device_inputs(pbe, shape)
        for half in ("fused", "gemm"):
            got = pbe.ao2mo_factor(b, ca, cb, half=half)
            for g in ([got] if shape[3] == 1 else got):
                assert np.all(np.isfinite(pbe.to_host(g))), (shape, half)
            assert np.all(np.isfinite(pbe.to_host(pbe.ao2mo_factor_half(b, ca, cb, half=half)))), (shape, half)
    assert np.all(np.isfinite(pbe.to_host(pbe.ao2mo_factor_expand(pbe.asarray(np.ones((15, 15))), 5))))


def test_refusals_leave_the_outputs_untouched(be):
    big_n, n, naux = 18, 5, 9
    b, cs = afr.inputs((big_n, n, naux, 2))
    b_d, ca, cb = be.asarray(b), be.asarray(cs[0]), be.asarray(cs[1])
    outs = [be.asarray(np.full((n,) * 4, 7.0)) for _ in range(3)]
    p_out = be.asarray(np.full((2, naux, n * (n + 1) // 2), 7.0))
    nbytes = int(be.lib.nbx_ao2mo_factor_worksize(big_n, naux, n, 2))
    work = be.asarray(np.full(nbytes // 8 + 1, 7.0))
    lib, P = be.lib, be._p
    null = ctypes.c_void_p(0)

    def full(nao=big_n, naux_=naux, nset=2, ldca=n, cb_=None, ldcb=n, n_=n, bbbb=None, wbytes=nbytes):
        return lib.nbx_ao2mo_factor(be.ctx, nao, naux_, P(b_d), nset, P(ca), ldca, P(cb) if cb_ is None else cb_, ldcb, n_,
                                    P(outs[0]), P(outs[1]) if bbbb is None else bbbb, P(outs[2]), P(work), wbytes)

    assert full(n_=362, ldca=362, ldcb=362) == _nbx.NBX_E_UNSUPPORTED
    assert "361" in lib.nbx_last_error().decode()
    assert full(naux_=0) == _nbx.NBX_E_INVALID
    assert full(nao=0) == _nbx.NBX_E_INVALID
    assert full(nset=3) == _nbx.NBX_E_INVALID and full(nset=0) == _nbx.NBX_E_INVALID
    assert full(ldca=n - 1) == _nbx.NBX_E_INVALID and full(ldcb=n - 1) == _nbx.NBX_E_INVALID
    assert full(cb_=null) == _nbx.NBX_E_INVALID and full(bbbb=null) == _nbx.NBX_E_INVALID
    assert full(wbytes=nbytes - 1) == _nbx.NBX_E_NOMEM
    assert lib.nbx_ao2mo_factor(be.ctx, big_n, naux, P(b_d), 2, P(ca), n, P(cb), n, n, P(outs[0]), P(outs[1]), P(outs[2]), null,
                                nbytes) == _nbx.NBX_E_NOMEM
    assert lib.nbx_ao2mo_factor_half(be.ctx, big_n, 0, P(b_d), 2, P(ca), n, P(cb), n, n, P(p_out)) == _nbx.NBX_E_INVALID
    assert lib.nbx_ao2mo_factor_half(be.ctx, big_n, naux, P(b_d), 2, P(ca), 362, P(cb), 362, 362, P(p_out)) == _nbx.NBX_E_UNSUPPORTED
    assert lib.nbx_ao2mo_factor_expand(be.ctx, 362, P(work), P(outs[0])) == _nbx.NBX_E_UNSUPPORTED
    assert lib.nbx_ao2mo_factor_expand(be.ctx, 0, P(work), P(outs[0])) == _nbx.NBX_E_INVALID
    be.synchronize()
    for t in (*outs, p_out, work):
        assert np.all(be.to_host(t) == 7.0)
    # ... and the same arguments, accepted, do write them
    assert full() == _nbx.NBX_OK
    ref, _ = afr.blocks_reference(b, cs, dtype=np.float64)
    for t, r in zip(outs, ref):
        np.testing.assert_allclose(be.to_host(t), r, rtol=0, atol=1e-9 * np.abs(r).max())
    with pytest.raises(ValueError, match="half='dense'"):
        be.ao2mo_factor(b_d, ca, cb, half="dense")
    with pytest.raises(ValueError, match="alpha but"):
        be.ao2mo_factor(b_d, ca, cb[:, :3])


# ------------------------------------------------------------------------------------------ 5. real molecules
NELEC = {"water-631gs": (5, 5), "h2o2-631gs": (9, 9)}


@lru_cache(maxsize=None)
def _molecule(name):
    from test_gpu_eri_cholesky import CASES  # the geometries

    xyz, basis, cart = CASES[name]
    assert not cart
    return integrals.molecule_integrals(xyz, basis, engine="native-1e")


_UHF = {}


def _dense_uhf(be, name):
    """The converged UHF object of the molecule on the dense device tensor, one per module."""
    if name not in _UHF:
        m = _molecule(name)
        mf = GpuUHF(Mole(m["nao"], NELEC[name], e_nuc=m["e_nuc"]), m["S"], m["hcore"], be.eri(m["basis"]), backend=be)
        mf.conv_tol = 1e-10
        mf.kernel()
        assert mf.converged
        _UHF[name] = mf
    return _UHF[name]


@pytest.mark.parametrize("tol", [1e-4, 1e-8])
@pytest.mark.parametrize("name", sorted(NELEC))
def test_builder_on_a_factor_against_the_dense_device_route(be, name, tol, monkeypatch):
    """|factor route - dense device route| <= (tol + 4e-13) ||c_i||_1 ||c_j||_1 ||c_k||_1 ||c_l||_1 on every element of
    aaaa, bbbb, aabb, C the converged UHF orbitals: the factor reproduces every (pq|rs) within tol, the engines agree
    within 2e-13 (ENGINE_ATOL) and both transforms round below 2e-13 at these sizes."""
    m = _molecule(name)
    dense = _dense_uhf(be, name)
    factor = GpuUHF(Mole(m["nao"], NELEC[name], e_nuc=m["e_nuc"]), m["S"], m["hcore"], backend=be,
                    eri_factor=be.eri_cholesky(m["basis"], tol=tol))
    factor.mo_coeff, factor.mo_occ = dense.mo_coeff, dense.mo_occ

    def forbidden(*a, **k):
        raise AssertionError("the factor route asked for (pq|rs)")

    monkeypatch.setattr(factor, "eri_device", forbidden, raising=False)
    want = be.to_host(HamiltonianBuilder(dense, backend=be)._two_body_device(blocks=3))
    got = be.to_host(HamiltonianBuilder(factor, backend=be)._two_body_device(blocks=3))
    c = np.asarray(dense.mo_coeff)
    for blk, (x, y) in enumerate(((0, 0), (1, 1), (0, 1))):
        bound = afr.molecule_bound(tol, c[x], c[y]).transpose(0, 2, 3, 1)  # chem_to_phys, nbed/ham_builder.py:133
        diff = np.abs(got[blk] - want[blk])
        print(f"{name} tol {tol:g} rank {be.eri_cholesky_info['rank']} block {blk}: max |difference| = {diff.max():.3e}, "
              f"worst difference / bound = {(diff / bound).max():.3e}")
        assert np.all(diff <= bound)


# ------------------------------------------------------------------------------------------ 6. nbed(config)
def test_reference_known_answers_on_the_factor_route(be, monkeypatch):
    """Water / STO-3G, the reference's own configuration and literals (tests/test_reference_kats.py, which runs them on the
    dense route): global HF and FCI at 1e-7, embedded FCI with both projectors at that file's 5e-6 (the reference's
    loosely converged inputs).  The yardstick is the reference's numbers, not the dense route; tol = 1e-10."""
    from test_reference_kats import NBED_ARGS

    monkeypatch.delenv("NBED_ERI_ENGINE", raising=False)
    provider = BuiltinHFProvider(be, eri_engine="cholesky", cholesky_tol=1e-10)
    for proj in ("mu", "huzinaga"):
        drv = nbed(NbedConfig(**dict(NBED_ARGS, projector=proj)), provider=provider, backend=be)
        if proj == "mu":
            assert abs(drv._global_hf.e_tot - (-74.96099960129165)) < 1e-7
            assert abs(drv._global_fci.e_tot - (-75.00912605315143)) < 1e-7
        res = getattr(drv, proj)
        fci = drv._run_emb_fci(drv.embedded_scf)
        e_emb = fci.e_tot + drv.e_env + drv.two_e_cross - res["correction"] - res["beta_correction"]
        print(f"{proj}: embedded FCI {e_emb:.10f}")
        assert abs(e_emb - (-75.12858550813999)) < 5e-6
        assert abs(res["e_fci"] - e_emb) < 1e-9
        assert drv._global_hf.eri_factor_device() is not None and drv.embedded_scf.eri_factor_device() is not None


WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"


@pytest.fixture(scope="module")
def water_631g_runs(be):
    """nbed(config), water / 6-31G, two active atoms, both projectors, embedded CCSD on the device: once on the factor
    (tol = 1e-8) with HipBackend.eri and eri_pack_rs raising, once on the dense device route."""
    cfg = NbedConfig(geometry=WATER, n_active_atoms=2, basis="6-31g", xc_functional="b3lyp", convergence=1e-9,
                     projector="both", max_hf_cycles=100, max_dft_cycles=100, run_ccsd_emb=True)
    spatial = {"calls": 0, "on_factor": 0}
    real = HamiltonianBuilder.build_spatial_device

    def counting(self):
        spatial["calls"] += 1
        spatial["on_factor"] += int(self.scf_method.eri_factor_device() is not None)
        return real(self)

    def forbidden(*a, **k):
        raise AssertionError("an N^4 tensor was asked for on the factor route")

    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("NBED_ERI_ENGINE", raising=False)
        mp.setenv("NBED_CCSD_SOLVER", "device")
        mp.setattr(HamiltonianBuilder, "build_spatial_device", counting)
        with mp.context() as inner:
            inner.setattr(type(be), "eri", forbidden)
            inner.setattr(type(be), "eri_pack_rs", forbidden)
            got = nbed(cfg, provider=BuiltinHFProvider(be, eri_engine="cholesky", cholesky_tol=1e-8), backend=be)
        on_factor = dict(spatial)
        ref = nbed(cfg, provider=BuiltinHFProvider(be, eri_engine="device"), backend=be)
    return got, ref, on_factor


def test_nbed_on_the_factor_makes_no_tensor_and_runs_the_device_ccsd(water_631g_runs):
    got, _, spatial = water_631g_runs  # (the run completed with eri / eri_pack_rs raising)
    assert spatial["calls"] == spatial["on_factor"] == 2  # embedded CCSD of either projector through build_spatial_device
    for proj in ("mu", "huzinaga"):
        res = getattr(got, proj)
        assert res["scf"].eri_factor_device() is not None and res["scf"].converged
        assert np.isfinite(res["e_ccsd"]) and res["e_ccsd"] < res["e_rhf"]
        assert res["second_quantised"][2].shape == (24,) * 4


def test_nbed_on_the_factor_against_the_device_route(water_631g_runs):
    """Embedded energies and second_quantised of the factor route (tol = 1e-8) against the device route, within TEN TIMES
    the difference measured between the two routes on the numpy checker backend (full-pivoting numpy Cholesky against
    the host tensor; E2E_MEASURED in tests/ao2mo_factor_reference.py, which also says why the tensors are compared through
    their rotation invariants): energies 2.9e-10, occupied-space invariants 3.9e-9 (h1) and 2.8e-10 (h2), whole-space
    invariants of the mu projector 1.8e-9 (h1) and 5.6e-8 (h2)."""
    got, ref, _ = water_631g_runs
    for proj, d in afr.e2e_differences(got, ref).items():
        print(proj, {k: f"{v:.2e}" for k, v in d.items()})
        for name, v in d.items():
            assert v <= 10 * afr.E2E_MEASURED[name], (proj, name, v)
