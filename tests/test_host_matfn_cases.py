"""CPU checks of tests/matfn_cases.py: every reference carries a certificate of 1e-17 ||A|| or better, the float64
emulations of SP2 purification and of the coupled Newton-Schulz iteration are accepted exactly where the case tables
say and stay inside the derived bounds with room to spare (the worst ratio is printed), both parities of the
purification's step count occur, and the bound formulas give the numbers they are documented with.  A case of
tests/test_gpu_matfn.py therefore cannot fail on the device because of its reference or its bound."""

import numpy as np
import pytest

import matfn_cases as mc

LD = mc.LD
# what a correct float64 evaluation is allowed to use of a bound here: a quarter (measured: 0.10 purification,
# 0.12 Newton-Schulz, 0.12 LAPACK); the rest is for a different order of summation
HEADROOM = 0.25
WORST = {}


def note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print(f"{what}: |got - ref| / bound = {ratio:.3e} (worst so far {WORST[what]:.3e})")
    assert ratio <= HEADROOM, (what, ratio)


def certified(ref, label):
    orth, off = ref.cert
    print(f"{label}: max|I - X^T X| = {orth:.2e}, max|offdiag X^T A X| = {off:.2e}, ||A|| = {ref.norm:.3g}")
    assert orth <= mc.CERTIFICATE * ref.norm and off <= mc.CERTIFICATE * ref.norm, (label, ref.cert, ref.norm)
    assert np.all(np.diff(ref.lam) > 0), label  # the refined levels kept the constructed order
    assert np.max(np.abs(ref.lam.astype(np.float64) - ref.lam0)) <= 4 * ref.n * mc.EPS * ref.norm, label


# ------------------------------------------------------------------------------------------ construction
def test_construction():
    q = mc.householder_q(37, 5)
    assert q.dtype == LD and float(np.max(np.abs(q.T @ q - np.eye(37, dtype=LD)))) < 1e-18
    assert np.all(q != 0)  # dense: no tile of the operand is trivially zero
    f, ref, lam = mc.purify_matrix(37, 5, 0.3, 0)
    assert f.dtype == np.float64 and np.array_equal(f, f.T)
    assert np.all(np.diff(lam) > 0) and abs((lam[5] - lam[4]) - 0.3) < 1e-14
    assert -12.5 < lam[0] and lam[-1] < 10.5 and lam[-1] - lam[0] > 20
    # the same arguments give the same (cached, read-only) operand; another index another matrix
    assert mc.purify_matrix(37, 5, 0.3, 0)[0] is f and not f.flags.writeable
    assert not np.array_equal(mc.purify_matrix(37, 5, 0.3, 1)[0], f)
    lam0 = mc.fock_spectrum(64, 7, 0.0, 3)
    assert lam0[7] == lam0[6]
    s, sref = mc.power_matrix(16, 1e4)
    assert abs(sref.lam0[-1] / sref.lam0[0] - 1e4) < 1e-8 and np.array_equal(s, s.T)


def test_the_case_tables_cover_the_kernels_switches():
    sizes = [c[0] for c in mc.PURIFY_CASES]
    a = mc.PUR_ALL_AT_ONCE_MAX_N
    assert {a, a + 1} <= set(sizes) and any(n > a and n % 16 == 0 for n in sizes)          # loop edge; loop without tail
    assert {mc.PUR_INIT_GRID_SWITCH - 1, mc.PUR_INIT_GRID_SWITCH, mc.PUR_INIT_GRID_SWITCH + 1} <= set(sizes)
    assert {len(c[1]) for c in mc.PURIFY_CASES} == {1, 2, 3}
    assert any(0 in c[1] and c[0] in c[1] for c in mc.PURIFY_CASES)
    assert {mc.NS_T_GRID_SWITCH - 1, mc.NS_T_GRID_SWITCH} <= set(mc.POWER_SIZES)
    assert -(-(mc.NS_T_GRID_SWITCH - 1) ** 2 // 256) == 128 and -(-mc.NS_T_GRID_SWITCH ** 2 // 256) > 128
    assert mc.PUR_ALL_AT_ONCE_MAX_N in mc.EIGEN_SIZES and mc.PUR_ALL_AT_ONCE_MAX_N + 1 in mc.EIGEN_SIZES


def test_bound_formulas():
    assert 2 * mc.PUR_IDEM == 4e-12
    assert mc.purify_bound(100, [0.0, 0.0], 1.0) == 4e-12                      # no width: the stopping rule's share alone
    assert mc.purify_bound(100, [-12.0, 10.0], 0.02) == pytest.approx(4e-12 + 100 * 2.0**-52 * 22 / 0.02, rel=1e-15)
    assert mc.purify_bound(100, [-12.0, 10.0], 0.02) == pytest.approx(2.84e-11, rel=5e-3)
    assert mc.purify_bound(230, [-12.0, 10.0], 0.02) == pytest.approx(6.02e-11, rel=5e-3)
    assert mc.purify_bound(64, [-12.0, 10.0], 0.0) == float("inf")
    ref = np.array([[2.0, -0.5], [-0.5, 1.0]])
    assert mc.power_bound(37, 1e4, -0.5, ref) == 37 * mc.EPS * 1e4 * 2.0
    assert mc.power_bound(37, 1e4, -1.0, ref) == 37 * mc.EPS * 1e4 * 2.0
    assert mc.power_bound(37, 1e4, 0.5, ref) == 37 * mc.EPS * 1e2 * 2.0
    assert mc.worst_ratio(np.array([1.0, np.nan]), np.array([1.0, 1.0]), 1.0) == float("inf")
    assert mc.worst_ratio(np.array([1.0, 1.5]), np.array([1.0, 1.0], dtype=LD), 2.0) == 0.25


# ------------------------------------------------------------------------------------------ purification
@pytest.mark.parametrize("case", mc.PURIFY_CASES, ids=mc.purify_id)
def test_purification_cases(case):
    n, nocc, gap = case
    f, p_ref, bounds, refs = mc.purify_case(case)
    for b, k in enumerate(nocc):
        certified(refs[b], f"{mc.purify_id(case)}[{b}]")
        # the reference is a projector of rank k that commutes with F
        pr = p_ref[b]
        assert float(np.max(np.abs(pr @ pr - pr))) < 1e-17 and abs(float(np.trace(pr)) - k) < 1e-16 * max(n, 1)
        fl = f[b].astype(LD)
        assert float(np.max(np.abs(fl @ pr - pr @ fl))) < 1e-16 * refs[b].norm
        p, st = mc.purify_emulated(f[b], k)
        print(f"{mc.purify_id(case)}[{b}]: emulation accepted after {st} steps")
        assert 8 <= st <= 54, st
        note("purify_emulated", mc.worst_ratio(p, pr, bounds[b]))
        note("purify_emulated trace", abs(float(np.trace(p)) - k) / (n * bounds[b]))
        assert np.max(np.abs(p - p.T)) <= 1e-13
        assert mc.purify_emulated(f[b], k, max_iter=st - 1)[1] == -1


def test_purification_step_counts_of_both_parities():
    steps = [mc.purify_emulated(mc.purify_matrix(n, k, gap, i)[0], k)[1] for n, nocc, gap in mc.PURIFY_CASES
             for i, k in enumerate(nocc)]
    assert all(s > 0 for s in steps)
    assert {s & 1 for s in steps} == {0, 1}, steps


@pytest.mark.parametrize("n,k", mc.LADDER_SIZES)
def test_purification_gap_ladder(n, k):
    for gap in mc.LADDER_GAPS:
        f, ref, lam = mc.purify_matrix(n, k, gap)
        p, st = mc.purify_emulated(f, k)
        print(f"N={n} gap={gap:g}: emulation status {st}")
        if gap > 0:
            certified(ref, f"ladder N={n} gap={gap:g}")
        if gap in mc.LADDER_ACCEPTED:
            assert (55 <= st <= 58) if gap == 1e-2 else (66 <= st <= 69), (gap, st)
            note("purify_emulated", mc.worst_ratio(p, ref.projector(k), mc.purify_bound(n, lam, gap)))
        else:
            assert st == -1, (gap, st)


def test_purification_degenerate_inputs():
    assert mc.purify_emulated(3.0 * np.eye(5), 2)[1] == -2
    assert mc.purify_emulated(np.array([[1.5]]), 1)[1] == -2
    f = mc.purify_matrix(16, 3, 0.3, 0)[0].copy()
    f[2, 9] = np.nan
    assert mc.purify_emulated(f, 3)[1] < 0
    f[2, 9] = np.inf
    assert mc.purify_emulated(f, 3)[1] < 0
    d = np.diag(mc.fock_spectrum(20, 4, 0.3, 9))
    p, st = mc.purify_emulated(d, 4)
    assert st > 0 and np.all(p[~np.eye(20, dtype=bool)] == 0)
    assert np.max(np.abs(np.diag(p) - np.r_[np.ones(4), np.zeros(16)])) <= 4e-12


# ------------------------------------------------------------------------------------------ powers
@pytest.mark.parametrize("kappa", mc.KAPPAS)
@pytest.mark.parametrize("n", sorted(set(mc.POWER_SIZES + mc.EIGEN_SIZES)))
def test_power_cases(n, kappa):
    s, ref = mc.power_matrix(n, kappa)
    certified(ref, f"N={n} kappa={kappa:g}")
    sl = s.astype(LD)
    for p in mc.POWERS:
        r, bound = mc.power_reference(n, kappa, p)
        # the reference is the power: (S^-1/2)^2 S = I, (S^1/2)^2 = S, S^-1 S = I, to the longdouble level times kappa
        prod = {-0.5: r @ r @ sl, 0.5: r @ r, -1.0: r @ sl}[p]
        want = sl if p == 0.5 else np.eye(n, dtype=LD)
        assert float(np.max(np.abs(prod - want))) <= 1e-17 * kappa * n, (n, kappa, p)
        note("LAPACK eigh route", mc.worst_ratio(mc.eigh_power(s, p), r, bound))
        if n not in mc.POWER_SIZES:
            continue
        for ce, mi in ((1, mc.NS_MAX_ITER), (mc.NS_CHECK_EVERY, mc.NS_MAX_ITER), (7, 35)):
            got, it = mc.newton_schulz_emulated(s, p, max_iter=mi, check_every=ce)
            print(f"N={n} kappa={kappa:g} p={p} check_every={ce}: {it} steps")
            assert got is not None and 9 <= it <= mi, (ce, it)
            if ce == mc.NS_CHECK_EVERY:
                assert it <= 25
            note("newton_schulz_emulated", mc.worst_ratio(got, r, bound))
            assert np.max(np.abs(got - got.T)) == 0.0


def test_power_inputs_the_iteration_refuses():
    for s in (mc.refused_ill_conditioned(), mc.refused_indefinite()):
        assert np.array_equal(s, s.T)
        for p in mc.POWERS:
            assert mc.newton_schulz_emulated(s, p) == (None, -1)
    w = np.linalg.eigvalsh(mc.refused_indefinite())
    assert w[0] < -0.5 and w[-1] > 0.5
    w = np.linalg.eigvalsh(mc.refused_ill_conditioned())
    assert w[-1] / abs(w[0]) > 1e8
    # exact powers of a multiple of the identity
    for p, want in ((0.5, 2.0), (-0.5, 0.5), (-1.0, 0.25)):
        got, it = mc.newton_schulz_emulated(4.0 * np.eye(16), p)
        assert it > 0 and np.all(got[~np.eye(16, dtype=bool)] == 0) and np.max(np.abs(np.diag(got) - want)) <= 4 * mc.EPS
