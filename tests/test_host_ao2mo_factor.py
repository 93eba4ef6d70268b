"""The four-index transform from a factor of the integrals without a GPU: the workspace arithmetic of
nbx_ao2mo_factor_worksize, the provider's ``eri_engine="cholesky"`` arguments, ``HamiltonianBuilder`` on an SCF object
built on a factor (numpy checker backend with a numpy ``ao2mo_factor``), the references of
tests/ao2mo_factor_reference.py against their own bounds, and ``nbed(config)`` on the factor route of the checker
backend -- the run whose differences set the tolerances of tests/test_gpu_ao2mo_factor.py."""

import numpy as np
import pytest

import ao2mo_factor_reference as afr
from oracle_backend import OracleLookaheadBackend

from nbed_amd import NbedConfig, _nbx, integrals, nbed
from nbed_amd.dist import Shards
from nbed_amd.driver import BuiltinHFProvider
from nbed_amd.exceptions import HamiltonianBuilderError, NbedDriverError
from nbed_amd.ham_builder import HamiltonianBuilder
from nbed_amd.scf import GpuRHF, GpuUHF, Mole

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
TOL = 1e-8


def _align(x):
    return (x + 255) & ~255


def test_worksize_is_host_arithmetic_and_does_not_overflow():
    lib = _nbx.load_library()
    for nao, naux, n, nset in ((7, 1, 1, 1), (148, 1203, 148, 2), (220, 1794, 60, 2), (400, 6400, 361, 2), (400, 6401, 361, 1)):
        npair, rows = n * (n + 1) // 2, (naux + 3) // 4 * 4
        want = _align(8 * nset * rows * npair) + _align(8 * npair * npair)
        assert lib.nbx_ao2mo_factor_worksize(nao, naux, n, nset) == want, (nao, naux, n, nset)
    assert lib.nbx_ao2mo_factor_worksize(400, 6400, 361, 2) > 2 ** 35  # (npair^2 alone is 4.3e9 doubles)
    for bad in ((400, 6400, 362, 2), (148, 0, 148, 2), (148, 10, 0, 1), (0, 10, 4, 1), (148, 10, 4, 3), (148, 10, 4, 0)):
        assert lib.nbx_ao2mo_factor_worksize(*bad) == 0, bad


def _config(basis):
    return NbedConfig(geometry=WATER, n_active_atoms=2, basis=basis, xc_functional="b3lyp", convergence=1e-9,
                      projector="both", max_hf_cycles=100, max_dft_cycles=100)


def test_provider_arguments_and_environment(monkeypatch):
    monkeypatch.delenv("NBED_ERI_ENGINE", raising=False)
    monkeypatch.delenv("NBED_CHOLESKY_TOL", raising=False)
    be = afr.FactorOracleBackend()
    p = BuiltinHFProvider(be, eri_engine="cholesky")
    assert p.eri_engine == "cholesky" and p.cholesky_tol == 1e-8
    assert p._eri_route(_config("cc-pvdz")) == "cholesky"
    assert BuiltinHFProvider(be, eri_engine="cholesky", cholesky_tol=1e-12).cholesky_tol == 1e-12
    monkeypatch.setenv("NBED_ERI_ENGINE", "cholesky")
    monkeypatch.setenv("NBED_CHOLESKY_TOL", "1e-6")
    p = BuiltinHFProvider(be)
    assert p.eri_engine == "cholesky" and p.cholesky_tol == 1e-6
    assert BuiltinHFProvider(be, cholesky_tol=1e-5).cholesky_tol == 1e-5  # the argument wins
    assert BuiltinHFProvider(be, eri_engine="host").eri_engine == "host"
    for bad in ("1e-13", "0", "-1e-8", "nan", "inf", "tight"):
        monkeypatch.setenv("NBED_CHOLESKY_TOL", bad)
        with pytest.raises(NbedDriverError, match="NBED_CHOLESKY_TOL"):
            BuiltinHFProvider(be)
    monkeypatch.delenv("NBED_CHOLESKY_TOL")
    for bad in (1e-13, 0.0, float("nan")):
        with pytest.raises(NbedDriverError, match="at least 1e-12"):
            BuiltinHFProvider(be, eri_engine="cholesky", cholesky_tol=bad)
    with pytest.raises(NbedDriverError, match="eri_engine='cholesky'.*l = 3"):
        BuiltinHFProvider(be, eri_engine="cholesky")._integrals(_config("cc-pvtz"))
    with pytest.raises(NbedDriverError, match="eri_engine='cholesky'.*no device integral engine"):
        BuiltinHFProvider(OracleLookaheadBackend(), eri_engine="cholesky")._integrals(_config("cc-pvdz"))
    # auto never takes the factor route, and the other settings are what they were
    monkeypatch.delenv("NBED_ERI_ENGINE")
    assert BuiltinHFProvider(be)._eri_route(_config("cc-pvdz")) == "host"
    monkeypatch.setenv("NBED_ERI_ENGINE", "gpu")
    with pytest.raises(NbedDriverError, match="NBED_ERI_ENGINE='gpu'.*'auto', 'host' or 'device'"):
        BuiltinHFProvider(be)


@pytest.mark.parametrize("shape", afr.SHAPES, ids=str)
def test_float64_numpy_stays_inside_the_bounds_the_gpu_tests_use(shape):
    """The bounds of tests/test_gpu_ao2mo_factor.py, held here by numpy's own float64 products against the longdouble
    reference at the same shapes and inputs: a bound numpy missed would be a wrong bound."""
    b, cs = afr.inputs(shape)
    p_ref, mags = afr.half_reference(b, cs)
    p64, _ = afr.half_reference(b, cs, dtype=np.float64)
    assert p_ref.dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63
    ratio = np.abs(p64 - p_ref) / afr.half_bound(shape[0], mags)
    print(f"{shape}: stage 1 worst |error| / bound = {float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0
    ref, bounds = afr.blocks_reference(b, cs)
    got, _ = afr.blocks_reference(b, cs, dtype=np.float64)
    for g, r, bd in zip(got, ref, bounds):
        assert g.shape == (shape[1],) * 4 and np.all(np.abs(g - r) <= bd)


@pytest.fixture(scope="module", params=["sto-3g", "6-31g"])
def water(request):
    m = integrals.molecule_integrals(WATER, request.param)
    m["factor"] = afr.factor_of(m["eri"], TOL)
    n = m["nao"]
    resid = m["eri"].reshape(n * n, n * n) - np.einsum("lx,ly->xy", *(m["factor"].reshape(-1, n * n),) * 2)
    assert np.abs(resid).max() <= TOL
    return m


def _pair(cls, m, be):
    """(dense object with converged orbitals; object on the factor with the same orbitals).  GpuRHF has no loop of its
    own: it is given the alpha orbitals of the unrestricted run."""
    n = m["nao"]
    mol = lambda: Mole(n, (5, 5), e_nuc=m["e_nuc"])  # noqa: E731
    uhf = GpuUHF(mol(), m["S"], m["hcore"], m["eri"], backend=be)
    uhf.conv_tol = 1e-10
    uhf.kernel()
    assert uhf.converged
    dense = uhf if cls is GpuUHF else cls(mol(), m["S"], m["hcore"], m["eri"], backend=be)
    factor = cls(mol(), m["S"], m["hcore"], backend=be, eri_factor=m["factor"])
    for obj in (dense, factor):
        if cls is GpuUHF:
            obj.mo_coeff, obj.mo_occ = uhf.mo_coeff, uhf.mo_occ
        else:
            obj.mo_coeff, obj.mo_occ = np.asarray(uhf.mo_coeff)[0], 2.0 * np.asarray(uhf.mo_occ)[0]
    return dense, factor


def _forbid_the_tensor(monkeypatch, obj):
    def forbidden(*a, **k):
        raise AssertionError("the factor route asked for (pq|rs)")

    monkeypatch.setattr(obj, "eri_device", forbidden, raising=False)
    monkeypatch.setattr(obj, "eri_rs_device", forbidden, raising=False)


@pytest.mark.parametrize("cls", [GpuUHF, GpuRHF])
def test_builder_takes_the_factor_and_reproduces_the_dense_route(water, cls, monkeypatch):
    be = afr.FactorOracleBackend()
    dense, factor = _pair(cls, water, be)
    assert factor.eri_factor_device() is not None and dense.eri_factor_device() is None
    _forbid_the_tensor(monkeypatch, factor)
    c = np.asarray(dense.mo_coeff)
    n = c.shape[-1]
    want = be.to_host(HamiltonianBuilder(dense, backend=be)._two_body_device(blocks=3))
    got = be.to_host(HamiltonianBuilder(factor, backend=be)._two_body_device(blocks=3))
    assert be.calls["ao2mo_factor"] == 1 and got.shape == want.shape == (3, n, n, n, n)
    cs = (c, c) if c.ndim == 2 else (c[0], c[1])
    for blk, (x, y) in enumerate(((0, 0), (1, 1), (0, 1))):
        bound = afr.molecule_bound(TOL, cs[x], cs[y]).transpose(0, 2, 3, 1)  # chem_to_phys, ham_builder.py:133
        ratio = np.abs(got[blk] - want[blk]) / bound
        print(f"block {blk}: worst |factor - dense| / bound = {ratio.max():.3e}, max |difference| = {np.abs(got[blk] - want[blk]).max():.2e}")
        assert ratio.max() <= 1.0
    # the whole build: four blocks, scatter, truncation; and the spatial form the device solvers read
    c4, h1, h2 = HamiltonianBuilder(factor, 1.25, backend=be).build()
    r4, g1, g2 = HamiltonianBuilder(dense, 1.25, backend=be).build()
    assert c4 == r4 == 1.25 and np.array_equal(h1, g1) and h2.shape == (2 * n,) * 4
    assert np.abs(h2 - g2).max() <= 0.5 * afr.molecule_bound(TOL, cs[0], cs[1]).max() + 1e-8  # (+ the 1e-8 truncation)
    _, _, two = HamiltonianBuilder(factor, 0.0, backend=be).build_spatial_device()
    assert tuple(two.shape) == (3, n, n, n, n)


def test_builder_refuses_a_factor_it_cannot_transform(water):
    from test_host_eri_cholesky import FactorCheckerBackend  # jk_factor, no ao2mo_factor

    be = FactorCheckerBackend()
    _, factor = _pair(GpuUHF, water, be)
    with pytest.raises(HamiltonianBuilderError, match="no ao2mo_factor"):
        HamiltonianBuilder(factor, backend=be).build()
    be = afr.FactorOracleBackend()
    _, factor = _pair(GpuUHF, water, be)
    with pytest.raises(HamiltonianBuilderError, match="single rank"):
        HamiltonianBuilder(factor, backend=be, shards=Shards(water["nao"], world=2, rank=0)).build()


def test_nbed_on_the_factor_route_of_the_checker_backend(monkeypatch):
    """nbed(config), water / 6-31G, two active atoms, both projectors: the factor route (numpy full-pivoting Cholesky at
    1e-8) against the dense route.  The figures printed here are E2E_MEASURED of tests/ao2mo_factor_reference.py; the
    assertion is the GPU test's (ten times those).  No SCF object of the factor run is given the tensor."""
    monkeypatch.delenv("NBED_ERI_ENGINE", raising=False)
    be = afr.FactorOracleBackend()
    cfg = _config("6-31g")
    on_factor = BuiltinHFProvider(be, eri_engine="cholesky", cholesky_tol=TOL)
    monkeypatch.setattr(integrals, "two_electron_native", _counting(integrals.two_electron_native))
    got = nbed(cfg, provider=on_factor, backend=be)
    assert be.calls["eri_cholesky"] == 1 and be.calls["ao2mo_factor"] == 2 and be.calls.get("ao2mo", 0) == 0
    assert _counting.calls == 1  # (the checker's eri_cholesky itself; nothing else asked for the tensor)
    ints = on_factor._cache[(cfg.geometry, "6-31g", str(cfg.unit))]
    assert "eri" not in ints
    with pytest.raises(KeyError):
        ints["eri"]
    ref = nbed(cfg, provider=BuiltinHFProvider(be, eri_engine="host"), backend=be)
    diffs = afr.e2e_differences(got, ref)
    for proj, d in diffs.items():
        print(proj, {k: f"{v:.2e}" for k, v in d.items()})
        for name, v in d.items():
            assert v <= 10 * afr.E2E_MEASURED[name], (proj, name, v)


def _counting(fn):
    _counting.calls = 0

    def wrapped(*a, **k):
        _counting.calls += 1
        return fn(*a, **k)

    return wrapped
