"""nbx_geig_refine on the MI355X against tests/geig_cases.py: the pencil refinement behind every settled SCF cycle,
the one solver with no fallback queued behind it, on pencils with close pairs, exactly degenerate clusters and a 1e6
block, an overlap of condition 1e2 and 1e4, from four starts (the constructed C; LAPACK's vectors of the pencil moved
by 1e-9, 1e-6 and 0.3) and on its four paths: one iteration with separate output (no sort, the verdict straight to the
caller's word), one iteration in place, three and six iterations with the sorting pass.

The rule: every matrix is either REFUSED (status <= 0) or meets all four bounds of geig_cases against the certified
longdouble reference of the rounded pencil, with w ascending; F, S and C0 are bit-identical afterwards.  So that
refusing cannot hide a failure, the well separated spectra (spread, graded) must be ACCEPTED from every start but the
last, which must be refused wherever it is out of reach (must_refuse_d).  The float64 twin's verdict is printed beside
the device's and asserted equal on spread only; the twin never judges.  The worst error / bound per path and per bound
is kept and printed."""

import ctypes

import numpy as np
import pytest

import geig_cases as gc

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
WORST = {}
SENTINEL = -7.25e77
PATHS = {"direct": (1, False), "in-place": (1, True), "sorted-3": (3, False), "sorted-6": (6, False)}


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    yield HipBackend()
    print("\nnbx_geig_refine: worst error / bound per path and per bound:")
    for (path, bound), ratio in sorted(WORST.items()):
        print(f"  {path:10s} {bound:15s} {ratio:.3e}")


def judge(path, c, w, v, what):
    r = c.ratios(w, v)
    for bound in gc.BOUNDS:
        WORST[path, bound] = max(WORST.get((path, bound), 0.0), r[bound])
    print(f"{path} {what} {c.ident()}: |C^T S C - I| = {c.last_defect:.2e}, error / bound "
          + " ".join(f"{b} {r[b]:.3e}" for b in gc.BOUNDS))
    assert np.all(np.diff(w) >= 0), (path, what, c.ident())
    for bound in gc.BOUNDS:
        assert r[bound] <= 1.0, (path, what, c.ident(), bound, r[bound])


def refine(be, f, s, c0, path):
    """One call on `path` -> (w, c, status words), host arrays (batch, ...).  direct and the sorted paths go through
    be.geig_refine; in place through the C ABI with d_c == d_c0.  Asserts that F, S and C0 come back bit-identical
    (in place: C0 of a refused matrix) and that an accepted matrix has been written completely."""
    iters, in_place = PATHS[path]
    f_d, s_d, c0_d = be.asarray(f), be.asarray(s), be.asarray(c0)
    batch, n = f.shape[0], f.shape[-1]
    if in_place:
        torch = be.torch
        w_d = torch.full((batch, n), SENTINEL, dtype=torch.float64, device=be.device)
        st_d = torch.full((batch,), -77, dtype=torch.int32, device=be.device)
        nbytes = int(be.lib.nbx_geig_refine_worksize(n, batch))
        work = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=be.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        be._call("nbx_geig_refine", n, batch, p(f_d), p(s_d), p(c0_d), p(w_d), p(c0_d), p(st_d), p(work), work.numel(), iters)
        be.synchronize()
        c_d = c0_d
    else:
        w_d, c_d = be.geig_refine(f_d, s_d, c0_d, refine_iters=iters)
        st_d = be.last_eigh_status_d
    st = [int(x) for x in be.to_host(st_d)]
    w, c = be.to_host(w_d), be.to_host(c_d)
    np.testing.assert_array_equal(be.to_host(f_d), f)
    np.testing.assert_array_equal(be.to_host(s_d), s)
    assert -77 not in st, st
    if in_place:
        for b in range(batch):
            if st[b] <= 0:
                np.testing.assert_array_equal(c[b], c0[b])
                assert np.all(w[b] == SENTINEL)
            else:
                assert not np.any(w[b] == SENTINEL)
    else:
        np.testing.assert_array_equal(be.to_host(c0_d), c0)
    return w, c, st


def run(be, cases, labels, path, what=""):
    """The cases of one call from the starts `labels` (one per matrix) on `path`: the rule for every matrix, the
    twin's verdict beside the device's -> (w, status words, twin's status words)."""
    f, s = np.stack([c.f for c in cases]), np.stack([c.s for c in cases])
    c0 = np.stack([c.start(label) for c, label in zip(cases, labels)])
    w, v, st = refine(be, f, s, c0, path)
    iters, in_place = PATHS[path]
    pair = gc.pair_route(cases[0].n, len(cases))
    twin = [gc.refine_twin(c.f, c.s, c0[b], iters, norm_part=pair, direct=(iters == 1 and not in_place))[2]
            for b, c in enumerate(cases)]
    print(f"{path} {what} {[c.ident() for c in cases]} from {list(labels)}: status {st}, float64 twin {twin}")
    for b, c in enumerate(cases):
        assert st[b] <= 0 or st[b] in range(1001, 1001 + iters), st
        if st[b] > 0:
            judge(path, c, w[b], v[b], f"{what} from ({labels[b]}) status {st[b]}")
    return w, st, twin


def must_refuse_d(n, iters):
    """Start (d), the pencil moved by 0.3 P with ||P||_2 = 1.  One iteration can never accept it: the first update is
    1e-2 .. 1e-1, far above RF_TOL and every noise limit.  With more iterations it must be refused where 0.3 exceeds
    the mean level distance 22 / (N - 1), N >= 75: levels have crossed and the columns no longer belong to them.
    Below that the start is far but CONTRACTING (a first update of 0.3 / 11 = 0.03 < RF_GIVE_UP at N = 3): converging
    from it inside the bounds is no failure (the float64 twin does, at N = 2, 3 in three iterations and at 16, 17,
    37 in four or five), so there the matrix falls under the rule like any other."""
    return iters == 1 or 0.3 > 22.0 / (n - 1)


def hold_to_the_table(be, cases, path):
    """Starts (a) .. (d) for one batch of cases of ONE spectrum: the rule, and what has to be accepted or refused."""
    iters = PATHS[path][0]
    name, n = cases[0].name, cases[0].n
    for label in gc.STARTS:
        _, st, twin = run(be, cases, label * len(cases), path)
        if name in gc.MUST_ACCEPT and (label in "ab" or (label == "c" and iters >= 2)):
            assert all(x > 0 for x in st), (name, n, label, path, st)
        if label == "d" and must_refuse_d(n, iters):
            assert all(x <= 0 for x in st), (name, n, path, st)
        if name == "spread":
            assert st == twin, (n, label, path, st, twin)


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("entry", gc.TABLE, ids=gc.table_id)
def test_geig_refine(be, entry, path):
    """Batch 2, two seeds in one call, every start."""
    n, name, kappa = entry
    hold_to_the_table(be, [gc.case(name, n, kappa, 0), gc.case(name, n, kappa, 1)], path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", gc.SPECTRA[:2])
def test_geig_refine_one_matrix(be, name, path):
    """Batch 1 at the benchmark size (the paired small GEMM up to N = 256)."""
    hold_to_the_table(be, [gc.case(name, 148, 1.0e2, 0)], path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", gc.BATCH_FIVE_SIZES)
def test_geig_refine_batch_of_five(be, n, path):
    """Batch 5: N = 112 is the last size on the paired small GEMM, 113 the first on the general ones.  Spread and
    pairs alternate in the call; spread must be accepted beside whatever happens to pairs."""
    cases = [gc.case(name, n, 1.0e2, index) for name, index in gc.BATCH_FIVE]
    assert gc.pair_route(n, 5) == (n == 112)
    for label in gc.STARTS:
        _, st, _ = run(be, cases, label * 5, path)
        for b, c in enumerate(cases):
            if c.name == "spread" and (label in "ab" or (label == "c" and PATHS[path][0] >= 2)):
                assert st[b] > 0, (n, label, path, st)
            if label == "d":
                assert st[b] <= 0, (n, path, st)


# ------------------------------------------------------------------------------------------ mixed batch
@pytest.mark.parametrize("path", PATHS)
def test_mixed_batch_is_gated_per_matrix(be, path):
    """N = 148, [spread from (b), spread from (d), pairs from (a)] in ONE call: the middle matrix is refused, the
    others meet their own bounds (spread is accepted), and in the reversed order every matrix has the same status and
    the same eigenvalues to the bit."""
    cases = [gc.case("spread", 148, 1.0e2, 0), gc.case("spread", 148, 1.0e2, 1), gc.case("pairs", 148, 1.0e2, 0)]
    labels = "bda"
    w, st, _ = run(be, cases, labels, path, "mixed")
    assert st[0] > 0 and st[1] <= 0, st
    w_r, st_r, _ = run(be, cases[::-1], labels[::-1], path, "mixed, reversed")
    assert st_r == st[::-1], (st, st_r)
    for b in range(3):
        if st[b] > 0:
            np.testing.assert_array_equal(w_r[2 - b], w[b])


# ------------------------------------------------------------------------------------------ chain
@pytest.mark.parametrize("size", gc.CHAIN_DRIFTS)
@pytest.mark.parametrize("name", gc.SPECTRA[:2])
def test_chain_of_single_iterations_accumulates_nothing(be, name, size):
    """Eight calls with ONE iteration at N = 148, each from the previous output, F drifting by `size` of a fixed
    symmetric matrix of spectral norm one per step (a settled SCF): every accepted step meets the bounds of ITS
    pencil's reference, judged in longdouble like the rest, so nothing accumulates.  A refused step hands its start
    on.  On spread every step is accepted WHERE ONE ITERATION CAN: where the update the step asks for, evaluated from
    the references, is below RF_TOL / 2.  A drift of 1e-7 asks for 4e-6 .. 9e-6 (the vectors of an overlap with
    kappa = 1e2 have entries of 10) and RF_TOL = 3e-8 has to refuse it; 1e-10 asks for 1e-8 at most, which is a
    condition on the inputs asserted here, and there every step of spread must be accepted."""
    base = [gc.case(name, 148, 1.0e2, 0), gc.case(name, 148, 1.0e2, 1)]
    drift = [gc.unit_symmetric(148, 991 + b) for b in range(2)]
    s = np.stack([c.s for c in base])
    c0 = np.stack([c.start("a") for c in base])
    pencils, behind = base, [0, 0]
    for step in range(1, gc.CHAIN_STEPS + 1):
        pencils = [gc.Drifted(c, step * size * d, x0=p.x) for c, d, p in zip(base, drift, pencils)]
        f = np.stack([p.f for p in pencils])
        w, v, st = refine(be, f, s, c0, "direct")
        asked = [p.first_update((k + 1) * size * d) for p, d, k in zip(pencils, drift, behind)]
        print(f"chain {name} drift {size:g} step {step}: status {st}, update asked for " + " ".join(f"{x:.1e}" for x in asked))
        for b, p in enumerate(pencils):
            if st[b] > 0:
                judge("chain", p, w[b], v[b], f"drift {size:g} step {step}")
            if name == "spread" and size == gc.CHAIN_DRIFTS[-1]:
                assert asked[b] < 0.5 * gc.RF_TOL, (step, asked)
            if name == "spread" and asked[b] < 0.5 * gc.RF_TOL:
                assert st[b] == 1001, (step, st, asked)
            behind[b] = 0 if st[b] > 0 else behind[b] + 1
        c0 = np.stack([v[b] if st[b] > 0 else c0[b] for b in range(2)])
