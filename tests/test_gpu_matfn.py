"""The two matrix functions the SCF takes without an eigensolver, and the eigen route behind them, on the MI355X against
tests/matfn_cases.py: nbx_purify (SP2 purification, nbed_amd/csrc/purify.hip), nbx_sym_pow_ns (coupled Newton-Schulz,
nbed_amd/csrc/eigh.hip) and nbx_sym_pow.  Results are compared with the certified longdouble reference of the rounded
operand against bounds derived from eps, N, the spectrum and the stopping rule (the worst error / bound per routine is
printed); the routines' own verdicts -- status words, *h_iters, None -- are asserted at every exit: accepted, step
limit (-1), no usable bounds (-2), refused.

Sizes: purification N <= 196 (all operands requested at once) and N = 197, 200, 208, 230 (the 16-wide loop with tails
of 5, 8, 0 and 6), N = 63 / 64 / 65 (one | eight workgroups build P0), batches of 1, 2 and 3; Newton-Schulz N = 181 /
182 (ns_t_kernel: a block per 256 elements | a grid-stride loop); the eigen route N = 196 / 197 (LDS solver |
tridiagonal route)."""

import ctypes

import numpy as np
import pytest

import matfn_cases as mc
from nbed_amd import _nbx

# (the shared operands are read-only numpy arrays; they are only ever copied to the device)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
LD = mc.LD
WORST = {}


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


def judge(routine, got, ref, bound, what=""):
    """|got - ref| <= bound everywhere; the worst ratio per routine is kept and printed."""
    ratio = mc.worst_ratio(got, ref, bound)
    WORST[routine] = max(WORST.get(routine, 0.0), ratio)
    print(f"{routine} {what}: worst |got - ref| / bound = {ratio:.3e} (routine so far {WORST[routine]:.3e})")
    assert ratio <= 1.0, (routine, what, ratio)


def run_purify(be, f, nocc, max_iter=0):
    p_d, st_d = be.purify(be.asarray(f), nocc, max_iter)
    return be.to_host(p_d), st_d.cpu().numpy()


def purify_direct(be, f, nocc, work_fill, status_fill, max_iter=0):
    """nbx_purify through the C entry, on a workspace, a status tensor and an output the test filled itself."""
    torch = be.torch
    batch, n = f.shape[0], f.shape[-1]
    nbytes = int(be.lib.nbx_purify_worksize(n, batch))
    assert nbytes % 8 == 0
    work = torch.full((nbytes // 8,), work_fill, dtype=torch.float64, device=be.device)
    status = torch.full((batch,), status_fill, dtype=torch.int32, device=be.device)
    p = torch.full((batch, n, n), float("nan"), dtype=torch.float64, device=be.device)
    f_d = be.asarray(f)
    rc = be.lib.nbx_purify(be.ctx, n, batch, be._p(f_d), int(nocc[0]), int(nocc[-1]), be._p(p), be._p(work), nbytes,
                           int(max_iter), be._p(status))
    assert rc == _nbx.NBX_OK, (rc, be.lib.nbx_last_error())
    be.synchronize()
    return be.to_host(p), status.cpu().numpy()


# ------------------------------------------------------------------------------------------ purification
@pytest.mark.parametrize("case", mc.PURIFY_CASES, ids=mc.purify_id)
def test_purify_cases(be, case):
    n, nocc, gap = case
    f, p_ref, bounds, _ = mc.purify_case(case)
    p, st = run_purify(be, f, nocc)
    print(f"{mc.purify_id(case)}: device steps {st.tolist()}")
    assert p.shape == f.shape and st.shape == (len(nocc),)
    assert np.all(st > 0) and np.all(st <= mc.PUR_MAX_ITER), st
    for b, k in enumerate(nocc):
        judge("nbx_purify", p[b], p_ref[b], bounds[b], f"{mc.purify_id(case)}[{b}]")
        assert np.max(np.abs(p[b] - p[b].T)) <= 1e-13
        tr = float(np.sum(np.diag(p[b]).astype(LD)))
        assert abs(tr - k) <= n * bounds[b], (b, tr, k)
    # the same bits again
    p2, st2 = run_purify(be, f, nocc)
    np.testing.assert_array_equal(p2, p)
    np.testing.assert_array_equal(st2, st)
    # a limit one below the steps the slowest matrix took: that one reports -1, a quicker one is what it was
    m = int(st.max())
    p3, st3 = run_purify(be, f, nocc, max_iter=m - 1)
    for b in range(len(nocc)):
        if st[b] == m:
            assert st3[b] == -1, (b, st, st3)
        else:
            assert st3[b] == st[b]
            np.testing.assert_array_equal(p3[b], p[b])
    # ... and a limit of exactly that many steps is enough
    p4, st4 = run_purify(be, f, nocc, max_iter=m)
    np.testing.assert_array_equal(st4, st)
    np.testing.assert_array_equal(p4, p)


def test_purify_takes_step_counts_of_both_parities(be):
    """The result is in d_p whatever the parity of the accepting step (the iterates alternate between d_p and the
    workspace): both parities occur among the cases, and test_purify_cases holds every one of them to its bound."""
    steps = []
    for n, nocc, gap in mc.PURIFY_CASES:
        f = np.stack([mc.purify_matrix(n, k, gap, i)[0] for i, k in enumerate(nocc)])
        steps += run_purify(be, f, nocc)[1].tolist()
    print("device step counts:", steps)
    assert all(0 < s <= mc.PUR_MAX_ITER for s in steps)
    assert {s & 1 for s in steps} == {0, 1}, steps


@pytest.mark.parametrize("case", [c for c in mc.PURIFY_CASES if c[0] in (64, 197, 200) or len(c[1]) == 3], ids=mc.purify_id)
def test_purify_does_not_depend_on_what_its_buffers_held(be, case):
    n, nocc, gap = case
    f = np.stack([mc.purify_matrix(n, k, gap, i)[0] for i, k in enumerate(nocc)])
    p, st = run_purify(be, f, nocc)
    assert np.all(st > 0)
    # a call of another size in between leaves its iterates and traces in the shared workspace
    other = mc.purify_matrix(20, 1, 0.4, 0)[0]
    assert run_purify(be, other[None], (1,))[1][0] > 0
    p1, st1 = run_purify(be, f, nocc)
    np.testing.assert_array_equal(p1, p)
    np.testing.assert_array_equal(st1, st)
    # workspace of NaN, of large numbers, of zeros; status words that look like a verdict or like a step in progress
    for work_fill, status_fill in ((float("nan"), -1), (1.0e300, -2), (0.0, int(st[0])), (float("inf"), 1), (-7.5, 2**31 - 1)):
        p2, st2 = purify_direct(be, f, nocc, work_fill, status_fill)
        np.testing.assert_array_equal(st2, st, err_msg=f"{work_fill} {status_fill}")
        np.testing.assert_array_equal(p2, p, err_msg=f"{work_fill} {status_fill}")


@pytest.mark.parametrize("n,k", mc.LADDER_SIZES)
def test_purify_verdicts_down_the_gap_ladder(be, n, k):
    """Accepted and right, or refused; never accepted and wrong."""
    for gap in mc.LADDER_GAPS:
        f, ref, lam = mc.purify_matrix(n, k, gap)
        p, st = run_purify(be, f[None], (k,))
        s = int(st[0])
        print(f"N={n} gap={gap:g}: device status {s}")
        if gap == 0.0:
            assert s < 0
        elif s > 0:
            assert s <= mc.PUR_MAX_ITER
            judge("nbx_purify", p[0], ref.projector(k), mc.purify_bound(n, lam, gap), f"ladder N={n} gap={gap:g}")
        else:
            assert s == -1
        if gap == 1e-2:
            assert s > 0


def test_purify_degenerate_inputs(be):
    nan, inf = float("nan"), float("inf")
    # no usable Gershgorin bounds: a multiple of the identity, N = 1
    for f, k in ((3.0 * np.eye(16), 4), (np.zeros((5, 5)), 2), (np.array([[1.5]]), 1), (np.array([[1.5]]), 0)):
        assert run_purify(be, f[None], (k,))[1].tolist() == [-2], (f.shape, k)
    good = mc.purify_case((16, (3, 3), 0.3))[0]
    p_good, st_good = run_purify(be, good, (3, 3))
    assert np.all(st_good > 0)
    for bad_value, at in ((nan, (2, 9)), (inf, (2, 9)), (-inf, (9, 2)), (inf, (5, 5)), (nan, (0, 0))):
        bad = good[0].copy()
        bad[at] = bad_value
        assert run_purify(be, bad[None], (3,))[1][0] < 0, (bad_value, at)
        # one matrix of two fails, in either slot: the other is what it is alone
        for slot in (0, 1):
            pair = good.copy()
            pair[slot] = bad
            p, st = run_purify(be, pair, (3, 3))
            assert st[slot] < 0 and st[1 - slot] == st_good[1 - slot], (bad_value, at, slot, st)
            np.testing.assert_array_equal(p[1 - slot], p_good[1 - slot])
    pair = good.copy()
    pair[0] = 2.0 * np.eye(16)
    p, st = run_purify(be, pair, (3, 3))
    assert st[0] == -2 and st[1] == st_good[1]
    np.testing.assert_array_equal(p[1], p_good[1])
    # a diagonal F: exact zeros off the diagonal, ones on the occupied levels (both product paths)
    for n, k in ((20, 4), (200, 40)):
        lam = mc.fock_spectrum(n, k, 0.3, 9)
        order = np.random.default_rng(n).permutation(n)
        p, st = run_purify(be, np.diag(lam[order])[None], (k,))
        assert 0 < st[0] <= mc.PUR_MAX_ITER
        assert np.all(p[0][~np.eye(n, dtype=bool)] == 0)
        judge("nbx_purify", np.diag(p[0]), (order < k).astype(np.float64), mc.purify_bound(n, lam, 0.3), f"diagonal N={n}")


# ------------------------------------------------------------------------------------------ Newton-Schulz
@pytest.mark.parametrize("kappa", mc.KAPPAS)
@pytest.mark.parametrize("n", mc.POWER_SIZES)
def test_newton_schulz_cases(be, n, kappa):
    s = mc.power_matrix(n, kappa)[0]
    s_d = be.asarray(s)
    for p in mc.POWERS:
        ref, bound = mc.power_reference(n, kappa, p)
        got_d = be.sym_pow_newton_schulz(s_d, p, s)
        assert got_d is not None, (n, kappa, p)
        got = be.to_host(got_d)
        judge("nbx_sym_pow_ns", got, ref, bound, f"N={n} kappa={kappa:g} p={p}")
        assert np.max(np.abs(got - got.T)) <= 1e-15 * float(np.max(np.abs(ref)))
        # without the host copy the bound of the spectrum comes from the device array: the same number, the same bits
        again = be.sym_pow_newton_schulz(s_d, p)
        assert again is not None
        np.testing.assert_array_equal(be.to_host(again), got)
        np.testing.assert_array_equal(be.to_host(s_d), s)  # the input is untouched
        # the residual examined at every step, and every seventh (35 steps: a multiple of seven, so that the steps
        # the stopping rule adds after its last look fit -- the default 28 is a multiple of the default 4)
        for check_every, max_iter in ((1, mc.NS_MAX_ITER), (7, 35)):
            other = be.sym_pow_newton_schulz(s_d, p, s, max_iter=max_iter, check_every=check_every)
            assert other is not None, (n, kappa, p, check_every)
            judge("nbx_sym_pow_ns", be.to_host(other), ref, bound, f"N={n} kappa={kappa:g} p={p} check_every={check_every}")


def ns_direct(be, s, p, c, max_iter=mc.NS_MAX_ITER, check_every=mc.NS_CHECK_EVERY, work_bytes=None, sentinel=-7.25):
    """nbx_sym_pow_ns through the C entry with d_out filled by the test -> (rc, *h_iters, d_out on the host)."""
    torch = be.torch
    n = s.shape[-1]
    nbytes = int(be.lib.nbx_sym_pow_ns_worksize(n))
    work = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=be.device)
    out = torch.full((n, n), sentinel, dtype=torch.float64, device=be.device)
    s_d = be.asarray(s)
    iters = ctypes.c_int(-7)
    rc = be.lib.nbx_sym_pow_ns(be.ctx, n, be._p(s_d), float(p), float(c), be._p(out), be._p(work),
                               nbytes if work_bytes is None else work_bytes, int(max_iter), int(check_every), ctypes.byref(iters))
    be.synchronize()
    return rc, iters.value, be.to_host(out)


def test_newton_schulz_exact_structure(be):
    off = ~np.eye(37, dtype=bool)
    lam = mc.power_matrix(37, 1e4)[1].lam0[np.random.default_rng(3).permutation(37)]
    for p in mc.POWERS:
        got = be.sym_pow_newton_schulz(be.asarray(np.diag(lam)), p, np.diag(lam))
        assert got is not None
        got = be.to_host(got)
        assert np.all(got[off] == 0)
        judge("nbx_sym_pow_ns", np.diag(got), lam.astype(LD) ** LD(p), mc.power_bound(37, 1e4, p, lam**p), f"diagonal p={p}")
    for n in (16, 37):
        for p, want in ((0.5, 2.0), (-0.5, 0.5), (-1.0, 0.25)):
            got = be.sym_pow_newton_schulz(be.asarray(4.0 * np.eye(n)), p, 4.0 * np.eye(n))
            assert got is not None
            got = be.to_host(got)
            assert np.all(got[~np.eye(n, dtype=bool)] == 0)
            assert np.max(np.abs(np.diag(got) - want)) <= 4 * mc.EPS, (n, p, np.diag(got) - want)


@pytest.mark.parametrize("which", ["ill_conditioned", "indefinite"])
def test_newton_schulz_refuses_and_the_eigen_route_takes_over(be, which):
    s = getattr(mc, "refused_" + which)()
    n = s.shape[0]
    c = float(np.abs(s).sum(axis=1).max())
    for p in mc.POWERS:
        assert be.sym_pow_newton_schulz(be.asarray(s), p, s) is None
        assert be.sym_pow_newton_schulz(be.asarray(s), p) is None
        # "d_out is only written on success": a workspace of NaN, the sentinel in d_out survives, *h_iters says -1
        rc, iters, out = ns_direct(be, s, p, c)
        assert (rc, iters) == (_nbx.NBX_OK, -1)
        assert np.all(out == -7.25)
        if which == "indefinite" and p != -1.0:
            continue  # (a root of a negative level: the eigen route has nothing to say either)
        np.testing.assert_array_equal(be.to_host(be.sym_pow_fast(be.asarray(s), p, s)), be.to_host(be.sym_pow(be.asarray(s), p)))
    # an accepted call through the same entry does write, and says how many steps it took
    good = mc.power_matrix(n, 1e4)[0]
    rc, iters, out = ns_direct(be, good, -0.5, float(np.abs(good).sum(axis=1).max()))
    assert rc == _nbx.NBX_OK and 0 < iters <= mc.NS_MAX_ITER
    judge("nbx_sym_pow_ns", out, *mc.power_reference(n, 1e4, -0.5), "C entry, NaN workspace")
    # a NaN in S: refused
    bad = good.copy()
    bad[3, 5] = bad[5, 3] = float("nan")
    assert be.sym_pow_newton_schulz(be.asarray(bad), -0.5, bad) is None
    rc, iters, out = ns_direct(be, bad, -0.5, 1.0)
    assert (rc, iters) == (_nbx.NBX_OK, -1) and np.all(out == -7.25)


# ------------------------------------------------------------------------------------------ the eigen route
@pytest.mark.parametrize("kappa", mc.KAPPAS)
@pytest.mark.parametrize("n", mc.EIGEN_SIZES)
def test_sym_pow_eigen_route(be, n, kappa):
    s = mc.power_matrix(n, kappa)[0]
    for p in mc.POWERS:
        ref, bound = mc.power_reference(n, kappa, p)
        got = be.to_host(be.sym_pow(be.asarray(s), p))
        judge("nbx_sym_pow", got, ref, bound, f"N={n} kappa={kappa:g} p={p}")


# ------------------------------------------------------------------------------------------ C ABI refusals
def test_c_abi_refusals_leave_the_outputs_alone(be):
    torch, lib = be.torch, be.lib
    n = 8
    f = be.asarray(np.stack([mc.purify_matrix(n, 3, 0.3, i)[0] for i in range(65)]))
    p = torch.full((65, n, n), -7.25, dtype=torch.float64, device=be.device)
    status = torch.full((65,), 77, dtype=torch.int32, device=be.device)
    need = int(lib.nbx_purify_worksize(n, 64))
    work = torch.full((need // 8 + n * n + 64,), -7.25, dtype=torch.float64, device=be.device)  # (room for 65 as well)
    assert lib.nbx_purify_worksize(n, 65) == 0 and lib.nbx_purify_worksize(0, 1) == 0

    def purify(batch, nocc_a, nocc_b, work_bytes, max_iter=0):
        return lib.nbx_purify(be.ctx, n, batch, be._p(f), nocc_a, nocc_b, be._p(p), be._p(work), work_bytes, max_iter, be._p(status))

    def untouched():
        be.synchronize()
        assert bool(torch.all(p == -7.25)) and bool(torch.all(status == 77)) and bool(torch.all(work == -7.25))

    assert purify(65, 3, 3, work.numel() * 8) == _nbx.NBX_E_INVALID       # batch > 64
    assert purify(2, n + 1, 3, need) == _nbx.NBX_E_INVALID                 # n_occ > N, either slot
    assert purify(2, 3, n + 1, need) == _nbx.NBX_E_INVALID
    assert purify(2, -1, 3, need) == _nbx.NBX_E_INVALID
    assert purify(3, 3, 2, need) == _nbx.NBX_E_INVALID                     # batch 3, unequal occupations
    assert purify(0, 3, 3, need) == _nbx.NBX_E_INVALID
    short = int(lib.nbx_purify_worksize(n, 2))
    assert purify(2, 3, 3, short - 1) == _nbx.NBX_E_NOMEM                  # a short workspace
    assert str(short).encode() in lib.nbx_last_error()
    untouched()
    with pytest.raises(ValueError):
        be.purify(f[:3], (3, 3, 2))
    # the same arguments, accepted: the call does run
    assert purify(2, 3, 3, short) == _nbx.NBX_OK
    be.synchronize()
    assert bool(torch.all(status[:2] > 0)) and bool(torch.all(status[2:] == 77)) and bool(torch.all(p[2:] == -7.25))

    s = mc.power_matrix(16, 1e1)[0]
    c = float(np.abs(s).sum(axis=1).max())
    need = int(lib.nbx_sym_pow_ns_worksize(16))
    for kw, code in ((dict(p=0.3), _nbx.NBX_E_INVALID), (dict(p=1.0), _nbx.NBX_E_INVALID), (dict(c=0.0), _nbx.NBX_E_INVALID),
                     (dict(c=-c), _nbx.NBX_E_INVALID), (dict(max_iter=0), _nbx.NBX_E_INVALID),
                     (dict(max_iter=-3), _nbx.NBX_E_INVALID), (dict(check_every=0), _nbx.NBX_E_INVALID),
                     (dict(work_bytes=need - 1), _nbx.NBX_E_NOMEM)):
        args = dict(p=-0.5, c=c)
        args.update(kw)
        rc, iters, out = ns_direct(be, s, **args)
        assert rc == code, (kw, rc, lib.nbx_last_error())
        assert iters == -7 and np.all(out == -7.25), kw
    assert str(need).encode() in lib.nbx_last_error()
    assert be.sym_pow_newton_schulz(be.asarray(s), 0.3, s) is None
    # the context still works
    rc, iters, out = ns_direct(be, s, -0.5, c)
    assert rc == _nbx.NBX_OK and iters > 0
    judge("nbx_sym_pow_ns", out, *mc.power_reference(16, 1e1, -0.5), "after the refusals")
