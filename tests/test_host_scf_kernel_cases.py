"""CPU checks of tests/scf_kernel_cases.py: the exact operands are exact, the real-valued bounds are ones a correct
float64 evaluation meets, every table entry reaches the kernel instance it is listed under by the library's own route
functions (the ones the launchers call; host arithmetic only), and the longdouble Pulay reference is right."""

import numpy as np
import pytest

import scf_kernel_cases as sk
from nbed_amd import _nbx

LD = sk.LD


@pytest.fixture(scope="module")
def lib():
    return _nbx.load_library()


def as_int(x):
    """Float64 array of integers -> Python integers (object dtype: no rounding anywhere)."""
    assert np.array_equal(x, np.rint(x))
    return np.vectorize(int, otypes=[object])(x)


# ------------------------------------------------------------------------------------------ routes
def test_route_ids_mirror_the_header():
    header = (_nbx.LIB_PATH.parent.parent / "include" / "nbx.h").read_text()
    for prefix, names in (("NBX_CYCLE_SCALARS", sk.SC_NAMES), ("NBX_DIIS", sk.DIIS_NAMES), ("NBX_VO_SUMSQ", sk.VO_NAMES)):
        for value, name in names.items():
            assert f"#define {prefix}_{name} {value}" in header, (prefix, name)
    assert (_nbx.CYCLE_SCALARS_REFUSED, _nbx.CYCLE_SCALARS_T32, _nbx.CYCLE_SCALARS_T16, _nbx.CYCLE_SCALARS_T16_DENS) == \
        (sk.SC_REFUSED, sk.SC_T32, sk.SC_T16, sk.SC_T16_DENS)
    assert (_nbx.DIIS_REFUSED, _nbx.DIIS_FUSED, _nbx.DIIS_GENERAL) == (sk.DIIS_REFUSED, sk.DIIS_FUSED, sk.DIIS_GENERAL)
    assert (_nbx.VO_SUMSQ_REFUSED, _nbx.VO_SUMSQ_ONE_WG, _nbx.VO_SUMSQ_32_WG) == (sk.VO_REFUSED, sk.VO_ONE_WG, sk.VO_32_WG)


def test_every_table_entry_reaches_its_instance_and_every_instance_has_one(lib):
    for table, fn, names in ((sk.SCALARS_TABLE, lib.nbx_cycle_scalars_route, sk.SC_NAMES),
                             (sk.DIIS_TABLE, lib.nbx_diis_route, sk.DIIS_NAMES),
                             (sk.VO_TABLE, lib.nbx_vo_sumsq_route, sk.VO_NAMES)):
        assert set(table) == set(names) and all(len(v) >= 1 for v in table.values())
        for inst, entries in table.items():
            for entry in entries:
                assert names[fn(*entry)] == names[inst], entry


def test_the_gpu_tests_shapes_are_in_the_tables():
    """What tests/test_gpu_scf_kernels.py parametrises over is what the tables hold (no shape tested off the record)."""
    listed = {e for entries in sk.SCALARS_TABLE.values() for e in entries}
    assert {(n, -1, -1) for n in sk.ASYNC_T16 + sk.ASYNC_T32 + sk.DTS_SIZES + [sk.REFUSED_SIZE]} <= listed
    assert {(n, a, b) for n, (a, b) in sk.CHAIN_CASES} <= listed
    assert sorted(sk.CHAIN_CASES) == sorted(sk.CHAIN_FUSED + sk.CHAIN_TWO_LAUNCH)
    diis = {e for entries in sk.DIIS_TABLE.values() for e in entries}
    assert {(n, nd) for n in sk.DIIS_NS for space in sk.DIIS_SPACES for _, nd in sk.diis_schedule(space)} <= diis
    assert {(n, a, b) for n, (a, b) in sk.VO_CASES} <= {e for entries in sk.VO_TABLE.values() for e in entries}


def test_route_edges(lib):
    """The thresholds themselves, from both sides."""
    sc, di, vo = lib.nbx_cycle_scalars_route, lib.nbx_diis_route, lib.nbx_vo_sumsq_route
    assert [sc(n, -1, -1) for n in (0, 1, 496, 497, 992, 993)] == [sk.SC_REFUSED, sk.SC_T16, sk.SC_T16, sk.SC_T32, sk.SC_T32,
                                                                    sk.SC_REFUSED]
    assert sc(70, 64, 64) == sc(70, 1, 64) == sc(496, 64, 1) == sk.SC_T16_DENS
    assert sc(70, 65, 64) == sc(70, 64, 65) == sc(70, 0, 5) == sc(70, 5, 0) == sk.SC_T16  # the two-launch fallback
    assert sc(497, 5, 5) == sk.SC_T32 and sc(993, 5, 5) == sk.SC_REFUSED
    assert sc(70, -1, 5) == sk.SC_T16  # (no density asked for)
    assert [di(4096, nd) for nd in (0, 1, 7, 8, 16, 17)] == [sk.DIIS_REFUSED, sk.DIIS_FUSED, sk.DIIS_FUSED, sk.DIIS_GENERAL,
                                                             sk.DIIS_GENERAL, sk.DIIS_REFUSED]
    assert di(65535 * 256, 3) == sk.DIIS_FUSED and di(65535 * 256 + 1, 3) == sk.DIIS_GENERAL  # (the fused kernel's grid)
    assert vo(256, 128, 127) == sk.VO_ONE_WG and vo(256, 128, 128) == sk.VO_ONE_WG and vo(257, 128, 128) == sk.VO_32_WG
    assert vo(16385, 1, 1) == sk.VO_ONE_WG and vo(16386, 1, 1) == sk.VO_32_WG  # nvir * nocc = 16384 | 16385
    assert vo(5, 0, 5) == sk.VO_ONE_WG and vo(5, 6, 0) == sk.VO_REFUSED


def test_dtot_table_layout_restatement_fills_the_librarys_table(lib):
    """scf_kernel_cases.dts_layout: one slot per pair (row, col <= row), no slot twice, inside the table whose size
    the library reports (nbx_jk_dts_bytes is host arithmetic)."""
    for N in sk.DTS_SIZES[:2]:
        idx, size = sk.dts_layout(N)
        live = idx[np.tril_indices(N)]
        assert size * 8 == lib.nbx_jk_dts_bytes(N)
        assert live.min() == 0 and live.max() < size and np.unique(live).size == live.size == N * (N + 1) // 2
        assert (idx[np.triu_indices(N, 1)] == -1).all()


def test_diis_schedule_wraps_and_crosses_the_solvers(lib):
    for space in sk.DIIS_SPACES:
        sched = sk.diis_schedule(space)
        assert len(sched) == space + 3 and sched[space] == (0, space) and sched[-1] == (2 % space, space)
        routes = [lib.nbx_diis_route(256, nd) for _, nd in sched]
        if space >= 8:  # the same ring goes from the fused kernel to the general one
            assert routes[6] == sk.DIIS_FUSED and routes[7] == sk.DIIS_GENERAL
        else:
            assert set(routes) == {sk.DIIS_FUSED}


# ------------------------------------------------------------------------------------------ exact operands
def test_exact_bits_is_the_largest_that_keeps_the_budget():
    budgets = [sk.BUDGETS["fock"](37), sk.BUDGETS["huzinaga"](241), sk.BUDGETS["trace"](2016), sk.BUDGETS["scalars"](992),
               sk.BUDGETS["dots"](32769), sk.BUDGETS["diis"](300001), sk.BUDGETS["vo"](129 * 128), sk.lincomb_budget(16)]
    for b in budgets:
        p = sk.exact_bits(b)
        assert 8 <= p <= sk.MAX_BITS and b(2 ** p) < 2 ** 52
        assert p == sk.MAX_BITS or b(2 ** (p + 1)) >= 2 ** 52


def test_magnitude_budget_holds_for_every_case():
    """The operands of every exact case stay within 2^p, and the budget evaluated at their largest magnitude < 2^52."""
    def mx(*xs):
        return max([float(np.max(np.abs(x[~np.isnan(x)]), initial=0.0)) for x in xs])

    for N in (1, 15, 16, 17, 37):
        assert sk.BUDGETS["fock"](N)(mx(*sk.fock_operands("exact", N))) < 2 ** 52
    for N in sk.HUZ_SIZES:
        for batch in (1, 2):
            assert sk.BUDGETS["huzinaga"](N)(mx(*sk.huz_operands("exact", N, batch))) < 2 ** 52
    for N in sk.TRACE_SIZES:
        assert sk.BUDGETS["trace"](N)(mx(*sk.trace_operands("exact", N))) < 2 ** 52
    for N in sorted(set(sk.SYNC_SIZES + sk.ASYNC_T16 + sk.ASYNC_T32 + sk.DTS_SIZES)):
        assert sk.BUDGETS["scalars"](N)(mx(*sk.scalars_operands("exact", N))) < 2 ** 52
    for n in sk.VEC_NS:
        for nvec in sk.VEC_NVECS:
            x, vecs, coef = sk.vec_operands("exact", n, nvec)
            assert sk.BUDGETS["dots"](n)(mx(x, vecs)) < 2 ** 52 and sk.lincomb_budget(nvec)(mx(vecs)) < 2 ** 52
            assert np.abs(coef).max() <= sk.CMAX and np.array_equal(2 * coef, np.rint(2 * coef))
    for N, nocc in sk.VO_CASES:
        total = max((N - k) * k for k in nocc)
        assert sk.BUDGETS["vo"](total)(mx(sk.vo_operands("exact", N, nocc))) < 2 ** 52
    for n in sk.DIIS_NS:
        x, e = sk.diis_vectors(16, n, 3)
        scale = 2.0 ** sk.diis_bits_and_shift(n)[1]  # e is integers times ONE power of two
        assert np.array_equal(e * scale, np.rint(e * scale))
        assert sk.BUDGETS["diis"](n)(mx(e * scale)) < 2 ** 52 and np.array_equal(x, np.rint(x))
    for N, _ in sk.CHAIN_CASES:
        hv, jk, ds, dm_in, _, _ = sk.chain_operands(N)
        fmax = mx(hv) + 2 * mx(jk)
        assert 2 * N * fmax * mx(ds) + fmax < 2 ** 52 and sk.BUDGETS["scalars"](N)(max(fmax, mx(dm_in))) < 2 ** 52


def test_exact_references_are_exact():
    """Float64 numpy summed in two different orders and Python-integer arithmetic agree bit for bit."""
    # the Huzinaga operator: 2 hz / kappa as integers
    for N, kappa in ((17, 1.0), (81, 0.5)):
        f, ds = sk.huz_operands("exact", N, 2)
        hz, fo, _, _ = sk.huz_fused_reference(f, ds, kappa)
        t = np.matmul(as_int(f), as_int(ds))
        want2 = -(t + np.swapaxes(t, -1, -2))  # hz / kappa
        fwd = -kappa * (np.matmul(f, ds) + np.swapaxes(np.matmul(f, ds), -1, -2))
        rev = -kappa * (np.matmul(f[..., ::-1], ds[:, ::-1, :]) + np.swapaxes(np.matmul(f[..., ::-1], ds[:, ::-1, :]), -1, -2))
        assert np.array_equal(fwd, rev) and np.array_equal(fwd, hz.astype(np.float64)) and np.all(hz == hz.astype(np.float64))
        assert np.array_equal(as_int(fwd / kappa), want2)
        assert np.array_equal(as_int(2 * fo.astype(np.float64)), 2 * as_int(f) + as_int(2 * kappa * np.ones(1))[0] * want2)
    # the cycle's scalars: 2 E as an integer, the squared norm as an integer
    for N in (33, 148):
        h3, vemb, vhf, hz, dm, dm_old = sk.scalars_operands("exact", N)
        energy, _, sumsq, _ = sk.scalars_reference(h3, vemb, vhf, hz, dm, dm_old)
        ham2 = 2 * as_int(h3) + as_int(vhf) + 2 * as_int(hz) + 2 * as_int(vemb)
        dt = np.swapaxes(as_int(dm), -1, -2)
        want2 = [int(np.sum(ham2[x] * dt[x])) for x in range(2)]
        ham = h3 + 0.5 * vhf + hz + vemb
        fwd = np.array([np.sum(ham[x] * dm[x].T) for x in range(2)])
        rev = np.array([np.sum((ham[x] * dm[x].T)[::-1, ::-1].T.copy()) for x in range(2)])
        assert np.array_equal(fwd, rev) and np.array_equal(fwd, energy.astype(np.float64))
        assert [int(2 * float(e)) for e in energy] == want2 and all(LD(float(e)) == e for e in energy)
        dd = as_int(dm) - as_int(dm_old)
        assert [int(float(s)) for s in sumsq] == [int(np.sum(dd[x] * dd[x])) for x in range(2)]
        table = sk.dts_restatement(dm)
        tot = as_int(dm[0]) + as_int(dm[1])
        assert int(table[5, 3]) == tot[5, 3] + tot[3, 5] and int(table[4, 4]) == tot[4, 4] and table[3, 5] == 0
    # dots, lincomb, trace, vo_sumsq
    x, vecs, coef = sk.vec_operands("exact", 32769, 5)
    assert np.array_equal(vecs @ x, vecs[:, ::-1] @ x[::-1]) and list(as_int(vecs @ x)) == [int(np.sum(as_int(v) * as_int(x))) for v in vecs]
    lin = sk.lincomb_reference(coef, vecs)[0]
    assert np.array_equal(coef @ vecs, coef[::-1] @ vecs[::-1]) and np.array_equal(coef @ vecs, lin.astype(np.float64))
    assert np.array_equal(as_int(2 * (coef @ vecs)), np.sum(as_int(2 * coef)[:, None] * as_int(vecs), axis=0))
    a, b = sk.trace_operands("exact", 33)
    tr = sk.trace_reference(a, b)[0]
    assert [int(float(t)) for t in tr] == [int(np.sum(as_int(a[z]) * as_int(b[z]).T)) for z in range(2)]
    fmo = sk.vo_operands("exact", 37, (10, 9))
    ref = sk.vo_reference(fmo, (10, 9))[0]
    assert [int(float(r)) for r in ref] == [int(np.sum(as_int(fmo[x, k:, :k]) ** 2)) for x, k in enumerate((10, 9))]
    assert np.isnan(fmo[0, :10]).all() and np.isnan(fmo[0, 10:, 10:]).all() and not np.isnan(fmo[0, 10:, :10]).any()
    # the Pulay matrix of a DIIS sequence, in units of 4^-s
    host = sk.DiisHost(6, 257)
    for t, (slot, nd) in enumerate(sk.diis_schedule(6)):
        xv, e = sk.diis_vectors(6, 257, t)
        hs = host.push(slot, nd, xv, e)
        assert np.array_equal(hs, hs.T)
    scale = 2.0 ** sk.diis_bits_and_shift(257)[1]
    ei = as_int(host.es * scale)
    assert np.array_equal(as_int(host.h[1:, 1:] * scale * scale), ei @ ei.T)


# ------------------------------------------------------------------------------------------ real-valued operands
def test_float64_numpy_stays_inside_every_real_bound():
    """Numpy's float64 evaluation of every kind of real-valued case against the longdouble reference: the bound is one
    a correct float64 evaluation meets (and the reference alone passes: it is compared with itself at ratio 0)."""
    worst = {}
    for N in (17, 37):
        h3, vemb, jk = sk.fock_operands("real", N)
        fock, vhf, bf, bv = sk.fock_reference(h3, vemb, jk)
        v64 = jk[0] - jk[1:]
        worst["fock"] = max(worst.get("fock", 0), sk.worst_ratio(h3 + v64 + vemb, fock, bf), sk.worst_ratio(v64, vhf, bv))
    for N in (17, 81, 161):
        f, ds = sk.huz_operands("real", N, 2)
        hz, fo, bh, bf = sk.huz_fused_reference(f, ds, 0.5)
        t = np.matmul(f, ds)
        hz64 = -0.5 * (t + np.swapaxes(t, -1, -2))
        worst["huzinaga"] = max(worst.get("huzinaga", 0), sk.worst_ratio(hz64, hz, bh), sk.worst_ratio(f + hz64, fo, bf))
        hz2, fo2, bh2, bf2 = sk.huz_sym_reference(t, 0.5, f)
        worst["huzinaga_sym"] = max(worst.get("huzinaga_sym", 0), sk.worst_ratio(hz64, hz2, bh2), sk.worst_ratio(f + hz64, fo2, bf2))
    for N in (33, 148):
        ops = sk.scalars_operands("real", N)
        ref = sk.scalars_reference(*ops)
        h3, vemb, vhf, hz, dm, dm_old = ops
        ham = h3 + 0.5 * vhf + hz + vemb
        got = np.concatenate([np.einsum("xij,xji->x", ham, dm), np.linalg.norm(dm - dm_old, axis=(-2, -1))])
        worst["scalars"] = max(worst.get("scalars", 0), sk.check_scalars(got, ref, exact=False))
        a, b = sk.trace_operands("real", N)
        tr, bt = sk.trace_reference(a, b)
        worst["trace"] = max(worst.get("trace", 0), sk.worst_ratio(np.einsum("xij,xji->x", a, b), tr, bt))
    x, vecs, coef = sk.vec_operands("real", 32769, 16)
    worst["dots"] = sk.worst_ratio(vecs @ x, *sk.dots_reference(x, vecs))
    worst["lincomb"] = sk.worst_ratio(coef @ vecs, *sk.lincomb_reference(coef, vecs))
    worst["axpby"] = sk.worst_ratio(1.5 * x - 0.75 * vecs[0], *sk.axpby_reference(1.5, x, -0.75, vecs[0]))
    fmo = sk.vo_operands("real", 257, (128, 128))
    got = np.array([np.sum(fmo[z, 128:, :128] ** 2) for z in range(2)])
    worst["vo_sumsq"] = sk.worst_ratio(got, *sk.vo_reference(fmo, (128, 128)))
    rng = np.random.default_rng(5)
    c = sk.real_entries(rng, (2, 40, 40))
    d, bd = sk.density_reference(c, (17, 0))
    worst["density"] = sk.worst_ratio(np.stack([c[0][:, :17] @ c[0][:, :17].T, np.zeros((40, 40))]), d, bd)
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert all(0 < v <= 1.0 for v in worst.values()), worst
    # cancellation is there: some results are far smaller than the terms that made them
    h3, vemb, jk = sk.fock_operands("real", 37)
    fock, _, bf, _ = sk.fock_reference(h3, vemb, jk)
    assert np.min(np.abs(fock.astype(np.float64)) / (bf / (8 * sk.EPS))) < 0.05


# ------------------------------------------------------------------------------------------ DIIS
def test_pulay_reference_matches_mpmath():
    mpmath = pytest.importorskip("mpmath")
    for space, n in ((7, 255), (16, 257), (16, 300001), (2, 1)):
        host = sk.DiisHost(space, n)
        for t, (slot, nd) in enumerate(sk.diis_schedule(space)):
            hs = host.push(slot, nd, *sk.diis_vectors(space, n, t)).copy()
        c = sk.pulay_solve(hs)
        with mpmath.workdps(40):
            rhs = mpmath.matrix([1] + [0] * nd)
            sol = mpmath.lu_solve(mpmath.matrix(hs.tolist()), rhs)
            want = np.array([LD(mpmath.nstr(v, 30)) for v in sol])
        kappa = np.linalg.cond(hs, 2)
        assert np.max(np.abs(c - want)) <= 8 * (nd + 1) * kappa * float(np.finfo(LD).eps) * np.max(np.abs(want)), (space, n)
        assert abs(float(np.sum(c[1:])) - 1.0) < 1e-12


def test_diis_coefficient_constant_is_the_calibrated_one():
    """DIIS_K from numpy's float64 solve over exactly the sequences the GPU test runs (module docstring)."""
    worst, where = 0.0, None
    for space in sk.DIIS_SPACES:
        for n in sk.DIIS_NS:
            host = sk.DiisHost(space, n)
            for t, (slot, nd) in enumerate(sk.diis_schedule(space)):
                hs = host.push(slot, nd, *sk.diis_vectors(space, n, t)).copy()
                if sk.diis_singular_by_construction(n, nd):
                    continue
                m = nd + 1
                kappa = float(np.linalg.cond(hs, 2))
                assert kappa < 1e6, (space, n, t, kappa)  # far from collinear: no eigenvalue anywhere near 1e-14
                c_ref = sk.pulay_solve(hs)
                rhs = np.zeros(m)
                rhs[0] = 1.0
                c = np.linalg.solve(hs, rhs)
                r = float(np.max(np.abs(c.astype(LD) - c_ref))) / (m * kappa * sk.EPS * float(np.max(np.abs(c_ref))))
                if r > worst:
                    worst, where = r, (space, n, t)
                assert float(np.max(np.abs(c.astype(LD) - c_ref))) <= sk.diis_coef_bound(hs, c_ref)
    print(f"numpy float64 solve: worst ratio {worst:.4f} at (space, n, update) = {where}; K = {sk.diis_k_from_ratio(worst)}")
    assert worst > 0 and sk.diis_k_from_ratio(worst) <= sk.DIIS_K == sk.diis_k_from_ratio(sk.DIIS_NUMPY_WORST_RATIO)


def test_spinorb_restatement_and_threshold_operands():
    tol = 1e-8
    one, two = sk.spinorb_operands(2, tol)
    below = np.nextafter(tol, 0.0)
    for v in (tol, -tol, below, -below):
        assert (two == v).any()
    h1, h2 = sk.spinorb_restatement(one, two, tol, 0.5)
    assert h2[0, 1, 1, 0] == (0.0 if abs(two[2, 0, 0, 0, 0]) < tol else 0.5 * two[2, 0, 0, 0, 0])
    assert h2[1, 2, 2, 1] == (0.0 if abs(two[3, 0, 1, 1, 0]) < tol else 0.5 * two[3, 0, 1, 1, 0])
    assert h2[0, 1, 0, 1] == 0.0 and h1[0, 1] == 0.0 and h1[3, 1] == (0.0 if abs(one[1, 1, 0]) < tol else one[1, 1, 0])
    kept = np.abs(two) >= tol
    assert np.count_nonzero(h2) == np.count_nonzero(two[kept]) and (np.abs(h2[h2 != 0]) >= 0.5 * tol).all()
