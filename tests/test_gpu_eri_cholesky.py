"""The diagonal and column sinks of the device integral engine (nbx_eri_diagonal, nbx_eri_columns; csrc/eri.hip), the
pivoted Cholesky decomposition built on them (nbx_eri_cholesky, csrc/eri_cd.hip; HipBackend.eri_cholesky), the J/K of a
density from the factor (HipBackend.jk_factor) and an SCF on it (``eri_factor=``).  The reference of every value is the
HOST engine's dense tensor (integrals.two_electron_native), never the device engine.

With u = 2^-53 and vmax = max (pq|pq) of the reference,

    eps(rank, tol) = tol + 2e-13 + 2 (rank + 2) u vmax

the decomposition's bound (the residual is positive semi-definite, so |R[pq][rs]| <= sqrt(R[pq][pq] R[rs][rs]) <= tol),
the tolerance the project holds between its integral engines, and the rounding of a rank-term sum whose absolute terms
sum to at most vmax (Cauchy-Schwarz on sum_L B_L[pq]^2 <= V[pq][pq]), once on the device and once in the check."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

from nbed_amd import _nbx, integrals

pytestmark = pytest.mark.gpu

WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
H2O2 = "4\n\nO   0.000  0.734  -0.052\nO   0.000  -0.734  -0.052\nH   0.839  0.881  0.419\nH   -0.839  -0.881  0.419"
H2 = "2\n\nH 0.0 0.0 0.0\nH 0.0 0.0 0.74"
H2_FAR = "2\n\nH 0 0 0\nH 0 0 12.0"

# the molecules of tests/test_gpu_eri.py: the smallest that reach every branch (the largest tensor: 32^4 doubles)
CASES = {
    "h2-sto3g": (H2, "sto-3g", False),
    "one-s-shell": ("1\n\nH 0 0 0", {"H": [(0, (0.5,), (1.0,))]}, False),
    "h2o2-sto3g": (H2O2, "sto-3g", False),
    "water-631gs": (WATER, "6-31g*", False),
    "water-631gs-cart": (WATER, "6-31g*", True),
    "h2o2-631gs": (H2O2, "6-31g*", False),
    "h2-12A-ccpvdz": (H2_FAR, "cc-pvdz", False),
}
F_TABLE = {"C": [(1, (0.38, 0.9), (0.7, 0.4)), (2, (1.097,), (1.0,)), (3, (0.761,), (1.0,))],
           "H": [(0, (0.3,), (1.0,)), (2, (1.057,), (1.0,)), (3, (0.9,), (1.0,))]}
U = 2.0 ** -53
ENGINE_ATOL = 2e-13  # the bound tests/test_gpu_eri.py holds between the device and the host engine


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@lru_cache(maxsize=None)
def _basis(name):
    xyz, basis, cart = CASES[name]
    return integrals.Basis(integrals.parse_geometry(xyz), basis, cart)


@lru_cache(maxsize=None)
def _ref(name):
    ref = integrals.two_electron_native(_basis(name), nthreads=4)
    ref.setflags(write=False)
    return ref


def _vmax(name):
    n = _ref(name).shape[0]
    return float(np.einsum("pqpq->pq", _ref(name)).max()) if n else 0.0


def eps(name, rank, tol):
    return tol + 2e-13 + 2 * (rank + 2) * U * _vmax(name)


def _shell_pairs(bs):
    return [(a, b) for a in range(len(bs.shells)) for b in range(a + 1)]


def _columns_of(bs, pairs):
    """(r, s) of every column of the listed shell pairs, in nbx_eri_columns' order."""
    nf = [int(sh.sph.shape[0]) for sh in bs.shells]
    ao0 = np.concatenate([[0], np.cumsum(nf)])
    return [(ao0[a] + x, ao0[b] + y) for a, b in pairs for x in range(nf[a]) for y in range(x + 1 if a == b else nf[b])]


_FACTOR = {}


def _factor(be, name, tol):
    """(B on the host, info) of one decomposition per (molecule, tol), shared by the tests."""
    if (name, tol) not in _FACTOR:
        b = integrals.cholesky_device(_basis(name), be, tol=tol)
        n = _basis(name).nao
        assert b.is_cuda and tuple(b.shape[1:]) == (n, n)
        b_h = be.to_host(b)
        b_h.setflags(write=False)
        _FACTOR[(name, tol)] = (b_h, dict(be.eri_cholesky_info))
    return _FACTOR[(name, tol)]


# ------------------------------------------------------------------------------------------ 1. diagonal and columns
def _check_diagonal_and_columns(backend, name, exact_zero_pattern):
    bs, ref = _basis(name), _ref(name)
    n = bs.nao
    diag = backend.to_host(backend.eri_diagonal(bs))
    want = np.einsum("pqpq->pq", ref)
    print(f"{name}: max |diag - host| = {np.abs(diag - want).max():.3e}")
    assert diag.shape == (n, n) and not np.isnan(diag).any()
    np.testing.assert_allclose(diag, want, rtol=0, atol=ENGINE_ATOL)
    np.testing.assert_array_equal(diag, diag.T)
    pairs = _shell_pairs(bs)
    cols = backend.to_host(backend.eri_columns(bs, pairs))
    rs = _columns_of(bs, pairs)
    assert cols.shape == (n * (n + 1) // 2, n, n) and len(rs) == cols.shape[0] and not np.isnan(cols).any()
    want = np.stack([ref[:, :, r, s] for r, s in rs])
    print(f"{name}: max |columns - host| = {np.abs(cols - want).max():.3e}, zero-pattern mismatches "
          f"{int(((cols == 0) != (want == 0)).sum())}")
    np.testing.assert_allclose(cols, want, rtol=0, atol=ENGINE_ATOL)
    np.testing.assert_array_equal(cols, cols.transpose(0, 2, 1))
    # Bit for bit the dense device tensor (nbx_eri_device), element by element: the three sinks store one double.
    dense = backend.to_host(backend.eri(bs))
    np.testing.assert_array_equal(cols, np.stack([dense[:, :, r, s] for r, s in rs]))
    np.testing.assert_array_equal(diag, np.einsum("pqpq->pq", dense))
    # Zero where the reference is zero.  DEVIATION from "on every case": asserted bit for bit where the zeros are screened
    # quartets (the stretched H2, as tests/test_gpu_eri.py does for the dense tensor).  Elsewhere an exact zero of the host
    # engine is a sum of terms that cancel by symmetry, and the device engine's other summation order leaves some of them
    # at <= 6e-16 (measured: 8 elements of h2o2-sto3g, 641 of water-631gs, 16 of water-631gs-cart, 1146 of h2o2-631gs) --
    # in the dense tensor too, which the lines above hold the columns equal to and which must not change.  There the
    # zeros are held to the engines' 2e-13, and to the dense tensor's own zero pattern exactly.
    if exact_zero_pattern:
        np.testing.assert_array_equal(cols == 0, want == 0)
        np.testing.assert_array_equal(diag == 0, np.einsum("pqpq->pq", ref) == 0)
    # the diagonal is the columns' own entry, the same double
    np.testing.assert_array_equal(np.array([cols[m, r, s] for m, (r, s) in enumerate(rs)]), np.array([diag[r, s] for r, s in rs]))
    return cols


@pytest.mark.parametrize("name", sorted(CASES))
def test_diagonal_and_columns_match_the_host_tensor(be, name):
    cols = _check_diagonal_and_columns(be, name, exact_zero_pattern=name == "h2-12A-ccpvdz")
    # a subset of the shell pairs, scrambled: the corresponding slices, bit for bit
    bs = _basis(name)
    pairs = _shell_pairs(bs)
    where, m = {}, 0
    for pr in pairs:
        k = len(_columns_of(bs, [pr]))
        where[pr] = (m, m + k)
        m += k
    pick = [pairs[i] for i in np.random.default_rng(5).permutation(len(pairs))[: max(1, (len(pairs) + 1) // 2)]]
    sub = be.to_host(be.eri_columns(bs, pick))
    np.testing.assert_array_equal(sub, np.concatenate([cols[slice(*where[pr])] for pr in pick]))


def test_nothing_is_left_unwritten_under_poisoned_allocations(monkeypatch):
    """Stretched H2 on a backend whose ``empty`` hands out NaN: memset and stores cover both outputs, and the quartets
    skipped are the ones the host engine skips."""
    from nbed_amd.backend import HipBackend

    monkeypatch.setenv("NBED_POISON_EMPTY", "1")
    poisoned = HipBackend()
    assert np.isnan(poisoned.to_host(poisoned.empty(3))).all()
    cols = _check_diagonal_and_columns(poisoned, "h2-12A-ccpvdz", exact_zero_pattern=True)
    assert 0.2 < (cols == 0).mean() < 0.99
    b = poisoned.to_host(poisoned.eri_cholesky(_basis("h2-12A-ccpvdz"), tol=1e-8))
    assert not np.isnan(b).any()


# ------------------------------------------------------------------------------------------ 2. the factor
FACTOR_CASES = [(name, tol) for name in sorted(CASES) for tol in (1e-4, 1e-8)] + [("water-631gs", 1e-11)]


@pytest.mark.parametrize("name,tol", FACTOR_CASES)
def test_factor_reproduces_the_tensor_within_the_bound(be, name, tol):
    b, info = _factor(be, name, tol)
    ref = _ref(name)
    n = ref.shape[0]
    rank = b.shape[0]
    assert rank == info["rank"] and info["resid"] <= tol and 1 <= rank <= n * (n + 1) // 2
    np.testing.assert_array_equal(b, b.transpose(0, 2, 1))
    b2 = b.reshape(rank, n * n)
    resid = ref.reshape(n * n, n * n) - b2.T @ b2
    bound = eps(name, rank, tol)
    print(f"{name} tol {tol:g}: rank {rank} of {n * (n + 1) // 2} pairs, steps {info['steps']}, columns {info['columns']}, "
          f"max |R| = {np.abs(resid).max():.3e}, min diag R = {np.diag(resid).min():.3e}, bound {bound:.3e}")
    assert np.abs(resid).max() <= bound
    assert np.diag(resid).min() >= -bound
    if name == "one-s-shell":
        assert rank == 1 and abs(b[0, 0, 0] ** 2 - ref[0, 0, 0, 0]) <= 4 * U * ref[0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ 3. it compresses
def test_block_pivoting_stays_close_to_full_pivoting(be):
    """h2o2 / 6-31G* at 1e-4: full pivoting in numpy needs 158 vectors for the 528 pairs; half the pairs is the cap."""
    b, info = _factor(be, "h2o2-631gs", 1e-4)
    print(f"h2o2-631gs tol 1e-4: rank {b.shape[0]} (numpy full pivoting: 158), steps {info['steps']}")
    assert b.shape[0] < 264


# ------------------------------------------------------------------------------------------ 4. determinism, max_rank
def _raw_cholesky(be, bs, tol, max_rank, buf, cutoff=1e-16):
    arrays = integrals._shell_arrays(bs)
    rank, resid = ctypes.c_int64(-7), ctypes.c_double(-7.0)
    rc = be.lib.nbx_eri_cholesky(be.ctx, len(bs.shells), *(a.ctypes.data_as(ctypes.c_void_p) for a in arrays), cutoff, tol,
                                 max_rank, be._p(buf), ctypes.byref(rank), ctypes.byref(resid))
    return rc, rank.value, resid.value


def test_two_calls_give_the_same_bits_and_max_rank_truncates(be):
    bs = _basis("h2o2-631gs")
    tol = 1e-8
    first, info = _factor(be, "h2o2-631gs", tol)
    again = be.to_host(be.eri_cholesky(bs, tol=tol))
    assert again.shape == first.shape
    np.testing.assert_array_equal(first, again)
    print(f"h2o2-631gs tol {tol:g}: {info['steps']} steps for {info['rank']} vectors, {info['columns']} columns")
    assert 0 < info["steps"] < info["rank"] <= info["columns"]
    steps, columns = ctypes.c_int64(), ctypes.c_int64()
    assert be.lib.nbx_eri_cholesky_steps(ctypes.byref(steps), ctypes.byref(columns)) == _nbx.NBX_OK
    assert (steps.value, columns.value) == (info["steps"], info["columns"])
    # room for 40 vectors only: not an error of the library, the residual says so; the slices past them are untouched
    buf = be.zeros((42, bs.nao, bs.nao))
    buf.fill_(-3.0)
    rc, rank, resid = _raw_cholesky(be, bs, tol, 40, buf)
    assert rc == _nbx.NBX_OK and rank == 40 and resid > tol
    got = be.to_host(buf)
    np.testing.assert_array_equal(got[:40], first[:40])
    assert (got[40:] == -3.0).all()
    with pytest.raises(ValueError, match=r"tol = 1e-08.*max_rank = 40"):
        be.eri_cholesky(bs, tol=tol, max_rank=40)


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_output_untouched(be):
    f_basis = integrals.Basis(integrals.parse_geometry("2\n\nC 0.1 -0.2 0.3\nH 0.9 0.5 -0.4"), F_TABLE)
    assert integrals.max_ang(f_basis) == 3
    water = _basis("water-631gs")
    for bs, tol, max_rank in ((f_basis, 1e-8, 100), (water, 1e-13, 100), (water, float("nan"), 100), (water, 1e-8, 0)):
        with pytest.raises(_nbx.NbxError) as err:
            be.eri_cholesky(bs, tol=tol, max_rank=max_rank)
        assert err.value.code == _nbx.NBX_E_INVALID
        buf = be.zeros((2, bs.nao, bs.nao))
        buf.fill_(-3.0)
        rc, rank, resid = _raw_cholesky(be, bs, tol, max_rank, buf)
        assert rc == _nbx.NBX_E_INVALID and (rank, resid) == (-7, -7.0)
        message = be.lib.nbx_last_error().decode()
        assert ("angular momentum" if bs is f_basis else "tol" if max_rank else "max_rank") in message, message
        assert (be.to_host(buf) == -3.0).all()
    # the f shells at the two other entry points, through the backend and through the library
    for method, args in ((be.eri_diagonal, ()), (be.eri_columns, ([(0, 0)],))):
        with pytest.raises(_nbx.NbxError) as err:
            method(f_basis, *args)
        assert err.value.code == _nbx.NBX_E_INVALID
    arrays = integrals._shell_arrays(f_basis)
    ptrs = [a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    buf = be.zeros((f_basis.nao, f_basis.nao))
    buf.fill_(-3.0)
    assert be.lib.nbx_eri_diagonal(be.ctx, len(arrays[0]), *ptrs, 1e-16, be._p(buf)) == _nbx.NBX_E_INVALID
    assert "angular momentum" in be.lib.nbx_last_error().decode()
    zero = np.zeros(1, dtype=np.int32)
    zp = zero.ctypes.data_as(ctypes.c_void_p)
    assert be.lib.nbx_eri_columns(be.ctx, len(arrays[0]), *ptrs, 1e-16, 1, zp, zp, be._p(buf)) == _nbx.NBX_E_INVALID
    assert "nbx_eri_columns" in be.lib.nbx_last_error().decode() and "angular momentum" in be.lib.nbx_last_error().decode()
    assert (be.to_host(buf) == -3.0).all()


# ------------------------------------------------------------------------------------------ 6. J/K from the factor
@pytest.mark.parametrize("name,nocc", [("water-631gs", (5, 4)), ("h2o2-631gs", (9, 8))])
def test_jk_from_the_factor_matches_jk_on_the_dense_tensor(be, name, nocc):
    tol = 1e-8
    b_h, _ = _factor(be, name, tol)
    ref = _ref(name)
    n = ref.shape[0]
    rng = np.random.default_rng(95)
    c = np.stack([np.linalg.qr(rng.standard_normal((n, n)))[0] for _ in range(2)])
    dms = np.stack([c[x][:, :nocc[x]] @ c[x][:, :nocc[x]].T for x in range(2)])
    b_d = be.asarray(b_h)
    want = be.to_host(be.jk(be.asarray(ref), be.asarray(dms)))
    from_dm = be.to_host(be.jk_factor(b_d, be.asarray(dms)))
    from_c = be.to_host(be.jk_df(b_d, be.asarray(c), nocc))
    assert from_dm.shape == from_c.shape == want.shape == (3, n, n)
    scale = np.abs(want).max()
    e = eps(name, b_h.shape[0], tol)
    weights = [np.abs(dms.sum(0)).sum(), np.abs(dms[0]).sum(), np.abs(dms[1]).sum()]
    for got, label in ((from_dm, "jk_factor"), (from_c, "jk_df")):
        for x in range(3):
            err = np.abs(got[x] - want[x]).max()
            print(f"{name} {label}[{x}]: max error {err:.3e}, bound {e * weights[x] + 1e-12 * scale:.3e}")
            assert err <= e * weights[x] + 1e-12 * scale
    assert np.abs(from_dm - from_c).max() <= 1e-12 * scale
    # one density, two dimensions
    one = be.to_host(be.jk_factor(b_d, be.asarray(dms[0])))
    assert one.shape == (2, n, n)
    np.testing.assert_allclose(one[1], from_dm[1], rtol=0, atol=1e-12 * scale)


# ------------------------------------------------------------------------------------------ 7. an SCF on the factor
def test_rhf_on_the_factor_reaches_the_dense_energy(be):
    """GpuRHF's SCF loop in this project is huzinaga_scf: with a zero embedding potential and an empty environment it is
    the plain RHF iteration.  |E_factor - E_dense| <= 0.75 eps max(sum|D|)^2 + 1e-9: the first-order error of
    E2 = 1/2 sum D (J - K/2) D at a fixed density, |dE2| <= 1/2 (1 + 1/2) eps (sum|D|)^2; both energies are variational
    minima, so the bound holds between the minima."""
    from nbed_amd.scf import GpuRHF, Mole, huzinaga_scf

    tol = 1e-8
    m = integrals.molecule_integrals(WATER, "6-31g*", engine="native-1e")
    bs = m["basis"]
    n = bs.nao
    zero = np.zeros((n, n))
    b = integrals.cholesky_device(bs, be, tol=tol)

    def run(**kw):
        mf = GpuRHF(Mole(n, (5, 5), e_nuc=m["e_nuc"]), m["S"], m["hcore"], backend=be, **kw)
        mf.max_cycle, mf.conv_tol = 100, 1e-10
        c, e, d, hz, conv = huzinaga_scf(mf, zero, zero, dm_conv_tol=1e-8)
        assert conv
        return mf.energy_tot(d), d, mf

    e_dense, d_dense, _ = run(eri=_ref("water-631gs"))
    e_factor, d_factor, mf = run(eri_factor=b)
    bound = 0.75 * eps("water-631gs", b.shape[0], tol) * max(np.abs(d_factor).sum(), np.abs(d_dense).sum()) ** 2 + 1e-9
    print(f"E dense {e_dense:.12f}, E factor {e_factor:.12f}, difference {abs(e_factor - e_dense):.3e}, bound {bound:.3e}")
    assert -76.1 < e_dense < -75.9
    assert abs(e_factor - e_dense) <= bound
    assert mf.eri_packed_device() is None and mf.eri_rs_device() is None and not mf.fused_fock_available(be.zeros((2, n, n)))
    with pytest.raises(ValueError, match="without two-electron integrals"):
        mf.eri_device()


def test_uhf_on_a_factor_never_asks_for_the_tensor(be, monkeypatch):
    from nbed_amd.dist import Shards
    from nbed_amd.scf import GpuUHF, GpuUKS, Mole, huzinaga_scf

    m = integrals.molecule_integrals(WATER, "6-31g*", engine="native-1e")
    n = m["basis"].nao
    b = be.asarray(_factor(be, "water-631gs", 1e-8)[0])
    mf = GpuUHF(Mole(n, (5, 5), e_nuc=m["e_nuc"]), m["S"], m["hcore"], backend=be, eri_factor=b)

    def forbidden():
        raise AssertionError("eri_device() was called on an object built on a factor")

    monkeypatch.setattr(mf, "eri_device", forbidden)
    mf.max_cycle = 3
    hist = []
    c, e, d, hz, conv = huzinaga_scf(mf, np.zeros((2, n, n)), np.zeros((2, n, n)), history=hist)
    assert len(hist) == 3 and np.isfinite(d).all() and abs(np.trace(d[0] @ m["S"]) - 5) < 1e-8
    # kernel() on the real backend: the step-by-step device loop, against the dense object's one-call-per-cycle loop
    monkeypatch.delenv("NBED_CYCLE_CALL", raising=False)
    dense = GpuUHF(Mole(n, (5, 5), e_nuc=m["e_nuc"]), m["S"], m["hcore"], _ref("water-631gs"), backend=be)
    on_factor = GpuUHF(Mole(n, (5, 5), e_nuc=m["e_nuc"]), m["S"], m["hcore"], backend=be, eri_factor=b)
    monkeypatch.setattr(on_factor, "eri_device", forbidden)
    for obj in (dense, on_factor):
        obj.conv_tol = 1e-10
        obj.kernel()
        assert obj.converged
    assert dense.kernel_info is not None and on_factor.kernel_info is None  # (only the one-call loop records it)
    sum_d = max(np.abs(obj.make_rdm1()).sum() for obj in (dense, on_factor))
    bound = 0.75 * eps("water-631gs", b.shape[0], 1e-8) * sum_d ** 2 + 1e-9
    print(f"kernel(): E dense {dense.e_tot:.12f}, E factor {on_factor.e_tot:.12f}, bound {bound:.3e}")
    assert abs(on_factor.e_tot - dense.e_tot) <= bound
    with pytest.raises(ValueError, match="not both"):
        GpuUHF(Mole(n, (5, 5)), m["S"], m["hcore"], _ref("water-631gs"), backend=be, eri_factor=b)
    with pytest.raises(ValueError, match="single rank"):
        GpuUKS(Mole(n, (5, 5)), m["S"], m["hcore"], backend=be, eri_factor=b, shards=Shards(n, world=2, rank=0))
