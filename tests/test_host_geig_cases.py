"""tests/geig_cases.py on the host: every reference of a pencil is certified, every group can be judged, float64
LAPACK (scipy.linalg.eigh(F, S)) passes every bound with room to spare, the float64 twin of refine_e_kernel with the
kernel's constants keeps the rule the device is held to (refused, or inside all four bounds; the well separated
spectra accepted), and the twin with the constants as shipped, or with one of three mutations, fails by a printed
factor.  tests/test_gpu_geig_refine.py holds nbx_geig_refine itself to the same bounds."""

import numpy as np
import pytest
import scipy.linalg

import geig_cases as gc

LAPACK_MAX = 0.25
WORST = dict.fromkeys(gc.BOUNDS, 0.0)
TABLE = gc.TABLE + [(n, name, 1.0e2) for n in gc.BATCH_FIVE_SIZES for name in gc.SPECTRA[:2]]


def show(r) -> str:
    return " ".join(f"{k} {x:.2e}" for k, x in r.items())


@pytest.mark.parametrize("entry", TABLE, ids=gc.table_id)
def test_every_case_is_certified_and_passed_by_lapack(entry):
    n, name, kappa = entry
    keys = [k for k in gc.all_case_keys() if (k[1], k[0], k[2]) == entry]
    assert len(keys) >= 2
    for key in keys:
        c = gc.case(*key)
        assert c.cert[0] <= c.cert_limits[0] and c.cert[1] <= c.cert_limits[1], (c.ident(), c.cert)
        assert np.array_equal(c.f, c.f.T) and np.array_equal(c.s, c.s.T)
        sizes = [b - a for a, b in c.groups]
        assert sum(sizes) == n
        assert max(c.subspace_bounds) < gc.SUBSPACE_MAX, (c.ident(), max(c.subspace_bounds))
        assert min(c.gamma) >= gc.GROUP * c.nrm * (1 - 1e-6)
        # the reference is S-orthonormal and its levels are the constructed ones to the rounding of F and S
        assert gc.worst_ratio(c.lam, c.lam0, np.max(c.eigenvalues)) <= 1.0
        w, v = scipy.linalg.eigh(c.f, c.s)
        ratios = c.ratios(w, v)
        print(f"{c.ident()}: groups {len(sizes)} (largest {max(sizes)}), certificate {c.cert[0]:.1e} {c.cert[1] / c.nrm:.1e} nrm, "
              f"orthonormality bound {c.orthonormality:.1e}, worst subspace bound {max(c.subspace_bounds):.1e}, "
              f"LAPACK / bound {show(ratios)}")
        for k, r in ratios.items():
            WORST[k] = max(WORST[k], r)
            assert r <= LAPACK_MAX, (c.ident(), k, r)
    print("LAPACK worst ratio per bound so far: " + show(WORST))


@pytest.mark.parametrize("entry", gc.TABLE, ids=gc.table_id)
def test_twin_with_the_kernels_constants_keeps_the_rule(entry):
    """The float64 twin (BLAS summation order) under the rule of tests/test_gpu_geig_refine.py: refused or inside the
    bounds; spread and graded accepted from (a), (b) with one iteration and from (a) .. (c) with three; (d) refused
    with one iteration, and with three where 0.3 exceeds the mean level distance 22 / (N - 1) (below N = 75 the start
    is far but contracting: at N = 2, 3 a first update of at most 0.3 / 11 = 0.03, which rightly converges)."""
    n, name, kappa = entry
    c = gc.case(name, n, kappa, 0)
    for label in gc.STARTS:
        for iters in (1, 3):
            w, v, st, log = gc.refine_twin(c.f, c.s, c.start(label), iters, norm_part=gc.pair_route(n, 2))
            line = f"twin {c.ident()} from ({label}), {iters} iteration(s): status {st}, max |E| {log[-1][0]:.1e}"
            if st > 0:
                assert np.all(np.diff(w) >= 0)
                r = c.ratios(w, v)
                print(line + " error / bound " + show(r))
                assert max(r.values()) <= 1.0, (c.ident(), label, iters, r)
            else:
                print(line)
            if name in gc.MUST_ACCEPT and (label in "ab" or (label == "c" and iters >= 2)):
                assert st > 0, (c.ident(), label, iters, st)
            if label == "d" and (iters == 1 or 0.3 > 22.0 / (n - 1)):
                assert st <= 0, (c.ident(), iters, st)


def test_twin_direct_and_sorted_paths_agree_on_ascending_levels():
    c = gc.case("spread", 37, 1.0e2, 0)
    w1, v1, st1, _ = gc.refine_twin(c.f, c.s, c.start("b"), 1, direct=True)
    w2, v2, st2, _ = gc.refine_twin(c.f, c.s, c.start("b"), 1, direct=False)
    assert st1 == st2 == 1001
    np.testing.assert_array_equal(w1, w2)
    np.testing.assert_array_equal(v1, v2)
    swapped = c.start("b").copy()
    swapped[:, [2, 3]] = swapped[:, [3, 2]]
    w3, v3, st3, _ = gc.refine_twin(c.f, c.s, swapped, 1, direct=True)
    assert st3 == -3
    w4, v4, st4, _ = gc.refine_twin(c.f, c.s, swapped, 1, direct=False)
    assert st4 == 1001 and np.all(np.diff(w4) >= 0) and max(c.ratios(w4, v4).values()) <= 1.0


# ------------------------------------------------------------------------------------------ what must fail
def test_shipped_constants_deliver_outside_the_bounds():
    """G unsymmetrised and the noise exit at max |E| < 1e-3, on pairs N = 148 kappa = 1e2 from the constructed C: the
    twin ACCEPTS (1001) with |C^T S C - I| of 1e-6 .. 1e-5, millions of bounds; with the limit alone lowered to 5e-7
    it accepts after three iterations and still misses by thousands (the unsymmetric G, first order in noise / gap);
    with both changes whatever it accepts is inside."""
    c = gc.case("pairs", 148, 1.0e2, 0)
    c0 = c.start("a")
    w, v, st, _ = gc.refine_twin(c.f, c.s, c0, 1, gc.SHIPPED_NOISE_EMAX_PENCIL, False, norm_part=True)
    r = c.ratios(w, v)
    print(f"shipped constants: status {st}, |C^T S C - I| = {c.gram_defect(v):.2e} = {r['orthonormality']:.3e} bounds; {show(r)}")
    assert st == 1001 and r["orthonormality"] > 1.0e3
    w, v, st, _ = gc.refine_twin(c.f, c.s, c0, 3, gc.RF_NOISE_EMAX, False, norm_part=True)
    r = c.ratios(w, v)
    print(f"limit 5e-7, G unsymmetrised: status {st}, |C^T S C - I| = {c.gram_defect(v):.2e} = {r['orthonormality']:.3e} bounds")
    assert st <= 0 or r["orthonormality"] > 10.0
    for iters in (1, 3, 6):
        w, v, st, _ = gc.refine_twin(c.f, c.s, c0, iters, norm_part=True)
        r = c.ratios(w, v)
        print(f"G symmetrised, limit 5e-7, {iters} iteration(s): status {st}, |C^T S C - I| = {c.gram_defect(v):.2e}")
        assert st <= 0 or max(r.values()) <= 1.0


def test_mutant_without_the_cluster_test_is_caught():
    """cmax ignored.  The start is the constructed C with the two vectors of the pair at a gap of 1.2e-10 rotated into
    each other by 45 degrees: equal Rayleigh quotients, so the kernel cannot rotate them back (gap below omega), and a
    coupling of half the gap, 6e-11, which it must refuse.  The mutant accepts and hands out the mean level twice.
    (LAPACK's vectors of a moved pencil do NOT serve: they diagonalise the perturbation inside a degenerate level.)"""
    c = gc.case("pairs", 37, 1.0e2, 0)
    c0 = c.start("a").copy()
    lo, hi = c0[:, 35].copy(), c0[:, 36].copy()
    c0[:, 35], c0[:, 36] = (lo - hi) / np.sqrt(2.0), (lo + hi) / np.sqrt(2.0)
    w, v, st, _ = gc.refine_twin(c.f, c.s, c0, 3)
    assert st <= 0, st
    w, v, st, _ = gc.refine_twin(c.f, c.s, c0, 3, ignore_cmax=True)
    r = c.ratios(w, v)
    print(f"cluster test removed: status {st} (the kernel's rule: refused), error / bound {show(r)}")
    assert st > 0 and max(r.values()) > 1.0


def nearly_normalised(c0, seed, size):
    """C0 (I + size K), K symmetric with unit entries at most: G = I + 2 size K + ..., so R is NOT zero."""
    n = c0.shape[0]
    k = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n))
    return c0 @ (np.eye(n) + size * 0.5 * (k + k.T))


def test_mutant_with_the_sign_of_lambda_g_flipped_is_caught():
    """num = S~_ij + lambda_j G_ij: invisible from an S-orthonormal start (G_ij = 0), so the start is C (I + 1e-7 K).
    The kernel's rule accepts at the second iteration inside the bounds; the mutant's iterate is outside them by the
    printed factor (and it never accepts: a must-accept matrix refused)."""
    c = gc.case("spread", 37, 1.0e2, 0)
    c0 = nearly_normalised(c.start("a"), 11, 1.0e-7)
    w, v, st, _ = gc.refine_twin(c.f, c.s, c0, 3)
    assert st == 1002 and max(c.ratios(w, v).values()) <= 1.0
    w, v, st, _ = gc.refine_twin(c.f, c.s, c0, 3, flip_sign=True)
    r = c.ratios(w, v)
    print(f"sign flipped: status {st} (the kernel's rule: 1002), the iterate's error / bound {show(r)}")
    assert max(r.values()) > 1.0
    assert st <= 0  # (were it accepted, the line above is the failure)


def test_mutant_without_the_division_by_g_is_caught():
    """lambda_i = T_ii instead of T_ii / G_ii, from C scaled to G_ii = 1 + 1e-6: the eigenvalues handed out are those
    of the vectors BEFORE the update, off by 1e-6 |l_i|.  Judged on the eigenvalues of the first iteration, whatever
    the verdict (max |E| = 5e-7 is at the limit of the noise exit; refused, the twin leaves the vectors as they came)."""
    c = gc.case("spread", 37, 1.0e2, 0)
    c0 = c.start("a") * np.sqrt(1.0 + 1.0e-6)
    assert abs(c.gram_defect(c0) - 1.0e-6) < 1.0e-9
    w, v, st, _ = gc.refine_twin(c.f, c.s, c0, 1)
    r = c.ratios(w, v)
    print(f"with the division: status {st}, error / bound {show(r)}")
    assert r["eigenvalues"] <= 1.0
    w, v, st_m, _ = gc.refine_twin(c.f, c.s, c0, 1, no_division=True)
    r = c.ratios(w, v)
    print(f"division removed: status {st_m}, error / bound {show(r)}")
    assert st_m == st and r["eigenvalues"] > 1.0e3
