"""The extended-precision SVD reference (oracle/svd.py) and the SVD contract of tests/svd_cases.py, on CPU.

* The reference agrees with mpmath's SVD at 40 digits to 1e-17 relative (longdouble arithmetic).
* The contract's relative-accuracy clause is not vacuous: LAPACK's singular values fail it on a
  column-graded matrix whose columns are not in decreasing order, the reference meets it.
* The kernel each GPU case is meant to exercise, from svd.hip's dispatch rule restated.
"""

from functools import lru_cache

import numpy as np
import pytest

import svd_cases as sc
from oracle import svd as osvd

mpmath = pytest.importorskip("mpmath")

LD = np.longdouble


@lru_cache(maxsize=None)
def _ref(kind, m, n, seed):
    return osvd.svd_right(sc.make(kind, m, n, seed))


@lru_cache(maxsize=None)
def _mp(kind, m, n, seed):
    a = sc.make(kind, m, n, seed)
    with mpmath.workdps(40):
        _, s, v = mpmath.svd_r(mpmath.matrix(a.tolist()), full_matrices=True)
        s_ld = np.array([LD(mpmath.nstr(x, 30)) for x in s])
        v_ld = np.array([[LD(mpmath.nstr(v[i, j], 30)) for j in range(n)] for i in range(n)])
    order = np.argsort(-s_ld, kind="stable")
    return s_ld[order], v_ld[order]


MP_CASES = [
    ("gauss", 1, 1), ("gauss", 6, 1), ("gauss", 1, 6), ("gauss", 6, 6), ("gauss", 24, 24), ("gauss", 9, 7),
    ("gauss", 7, 9), ("gauss", 21, 13), ("gauss", 5, 16), ("graded", 16, 16), ("graded", 20, 15),
    ("spectrum", 18, 18), ("spectrum", 24, 21), ("repeats", 12, 12), ("repeats", 15, 21),
]


@pytest.mark.parametrize("case", MP_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_reference_matches_mpmath(case):
    kind, m, n = case
    s, vt = _ref(kind, m, n, 7)
    s_mp, v_mp = _mp(kind, m, n, 7)
    assert s.dtype == LD and s.shape == (min(m, n),) and vt.shape == (n, n)
    # 1e-17 relative wherever Jacobi's own bound eps_ld min(kappa, ||A||_F / sigma) allows it: every value
    # of the well-conditioned and graded cases; the small values of a spectrum spread over 1e-6 get that bound
    a = sc.make(kind, m, n, 7)
    fro = float(np.linalg.norm(a))
    bound = np.maximum(1e-17, osvd.EPS_LD * np.minimum(sc.column_kappa(a), fro / s_mp.astype(np.float64)))
    rel = np.abs(s - s_mp) / np.where(s_mp > 0, s_mp, 1)
    assert np.all(rel <= bound), float(np.max(rel / bound))
    if kind in ("gauss", "graded"):
        assert float(rel.max()) <= 1e-17
    assert float(np.max(np.abs(vt @ vt.T - np.eye(n, dtype=LD)))) <= 1e-17 * n
    # vectors of well separated values agree up to sign, to 16 eps_ld min(||A||_F, kappa sigma) / gap
    kappa = sc.column_kappa(a)
    for j in range(min(m, n)):
        others = np.delete(s_mp, j)
        sj = float(s_mp[j])
        gap = float(np.min(np.abs(others - s_mp[j]))) if others.size else sj
        if gap > 1e-3 * sj:
            d = vt[j] - np.sign(vt[j] @ v_mp[j]) * v_mp[j]
            assert float(np.sqrt(d @ d)) <= 16 * osvd.EPS_LD * min(fro, kappa * sj) / gap, (j, gap / sj)
    if m < n:  # the completed rows span the null space of A
        res = np.asarray(a, dtype=LD) @ vt[m:].T
        assert float(np.max(np.abs(res))) <= 1e-17 * float(s_mp[0])


def test_reference_keeps_exact_zeros_and_repeats():
    a = sc.make("repeats", 24, 18)
    s, _ = _ref("repeats", 24, 18, 7)
    x = np.linalg.svd(a, compute_uv=False)
    # blockdiag(X, X, Z): the six values of X each appear twice, to 1e-17 or eps_ld ||A||_F / sigma relative
    tol = np.maximum(1e-17, 16 * osvd.EPS_LD * np.linalg.norm(a) / s.astype(np.float64))
    rel = np.abs(s[:, None] - s[None, :]) / s[:, None]
    pairs = (rel < tol[:, None]).sum(axis=1) - 1
    assert int(np.count_nonzero(pairs == 1)) == 12 and int(np.count_nonzero(pairs > 1)) == 0, (pairs, x)
    s0, vt0 = osvd.svd_right(np.zeros((5, 7)))
    assert np.all(s0 == 0) and np.array_equal(np.abs(vt0 @ vt0.T), np.eye(7))


def test_relative_clause_is_not_vacuous():
    """On a column-graded matrix with permuted columns the contract asks relative accuracy of sigma
    down to 1e-12; LAPACK (bidiagonalisation) loses it, the reference does not."""
    a = sc.make("graded", 60, 60)
    assert sc.column_kappa(a) <= 10.5
    s_ref, vt_ref = _ref("graded", 60, 60, 7)
    lap = np.linalg.svd(a, compute_uv=False)
    rel, _, floor = sc.sigma_errors(a, lap, s_ref)
    assert s_ref[-1] > 10 * floor  # every value is under the relative clause
    assert rel.max() > 10.0, rel.max()
    with pytest.raises(AssertionError):
        sc.check_contract(a, lap, np.linalg.svd(a)[2], (s_ref, vt_ref), "lapack")
    # the reference rounded to float64 meets it
    sc.check_contract(a, s_ref.astype(np.float64), vt_ref.astype(np.float64), (s_ref, vt_ref), "reference")


@pytest.mark.parametrize("case", [c for c in sc.CASES if c[1] * c[2] <= 40 * 40], ids=sc.case_id)
def test_contract_holds_for_the_rounded_reference(case):
    a = sc.make(*case)
    s, vt = _ref(*case, 7)
    sc.check_contract(a, s.astype(np.float64), vt.astype(np.float64), (s, vt), sc.case_id(case))


# ------------------------------------------------------------------ which kernel each GPU case runs
EDGES = {
    (138, 138): "lds", (139, 139): "fallback", (140, 140): "fallback",
    (100, 192): "lds", (101, 192): "fallback",
    (97, 196): "lds", (10, 197): "fallback",
    (9600, 2): "lds", (9601, 2): "fallback", (9601, 1): "fallback",
    (5, 8): "lds", (50, 300): "fallback",
    (115, 115): "lds", (169, 169): "fallback", (60, 33): "lds", (150, 140): "fallback",
}


@pytest.mark.parametrize("shape,kernel", list(EDGES.items()), ids=[f"{m}x{n}" for m, n in EDGES])
def test_dispatch_edges(shape, kernel):
    m, n = shape
    assert sc.kernel_for(m, n) == kernel
    assert (m, n) in {(c[1], c[2]) for c in sc.CASES}


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_gpu_case_table(case):
    """One line per GPU case: its id names the kernel it runs (``pytest -v`` lists them)."""
    kind, m, n = case
    assert kind in sc.KINDS and m > 0 and n > 0
    assert sc.case_id(case).endswith(sc.kernel_for(m, n))


def test_gpu_cases_cover_both_kernels_and_every_class():
    kernels = {(c[0], sc.kernel_for(c[1], c[2])) for c in sc.CASES}
    for kind in sc.KINDS:
        assert (kind, "fallback") in kernels, kind
        assert (kind, "lds") in kernels, kind
    for k in ("lds", "fallback"):
        odd = [c for c in sc.CASES if c[2] % 2 == 1 and sc.kernel_for(c[1], c[2]) == k]
        wide = [c for c in sc.CASES if c[1] < c[2] and sc.kernel_for(c[1], c[2]) == k]
        assert odd and wide, k
