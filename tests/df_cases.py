"""Shared by tests/test_host_df_cases.py (CPU) and tests/test_gpu_jk_df.py (MI355X): the factorised J/K -- nbx_jk_df
(nbed_amd/csrc/jk_df.hip) and HipBackend.jk_factor -- on inputs float64 holds EXACTLY, at shapes that reach every GEMM
kernel the benchmark's N = 2000 build runs on, and on real-valued inputs with a derived rounding bound.

What is computed.  B_L (naux symmetric N x N matrices), C^x (N x N, the first nocc[x] columns occupied), per L

    Yt^x_L = C_occ^x^T B_L                (nocc[x] x N)
    K[x]   = sum_L Yt^x_L^T Yt^x_L
    rho_L  = sum_x <Yt^x_L, C_occ^x^T>    (= <B_L, sum_x D_x>; doubled when one spin stands for both, ndm = 1)
    J      = sum_L rho_L B_L

and jk_factor forms the same J and K from the densities D_x = C_occ^x C_occ^x^T: J = sum_L B_L <B_L, sum_x D_x> (a
single density is NOT doubled there: factor_from_df() halves J of the ndm = 1 references) and K_x = sum_L B_L D_x B_L.

Exact inputs.  B_L has entries in {+-1, +-3} -- nothing is zero, so a skipped element changes an integer -- and C^x
entries in {+-1, +-2}, a different seed per spin (the matrices are not orthonormal; the formulas do not need it).  Every
term of every intermediate and output element is an integer and headroom() -- the same formulas on the absolute
values, an upper bound of every partial sum any order of summation can form, of jk_factor's too since |D_x| <=
|C_occ| |C_occ|^T element by element -- stays below 2^52 (the host test asserts it for every table entry; 2^36 at the
largest).  Every partial sum is then a float64: no rounding happens anywhere, in any order, fused or not, split over
lanes, waves, workgroups and slabs in any way, and numpy's float64 evaluation of the formulas IS the answer.  The
comparisons are array equality.

Graded variant.  Integer exponents e_p in [-12, 12]; B_L[p,q] is scaled by 2^(e_p + e_q) and C[q,i] by 2^(-e_q).  Every
term of Yt[i,q] then shares the factor 2^(e_q), every term of K[p,q] and J[p,q] the factor 2^(e_p + e_q), every term of
D[q,r] the factor 2^-(e_q + e_r), and rho is the same integer: the terms of ONE element share one exponent, their
integer parts are those of the plain variant, and everything above still holds while the inputs span 2^48.  A path that
orders, screens or truncates by magnitude fails it; so does one that adds terms of different elements.

Real inputs.  B = synth.df_factor(N, 0, naux), orthonormal C from the QR of a seeded normal matrix, the reference in
numpy.longdouble.  Per-element a-priori bounds, valid for any summation order, fused or not, with u = 2^-53,
g(n) = n u / (1 - n u), Ab = |B|, Ac = |C_occ|, Ya^x_L = Ac^x^T Ab_L:

    jk_df     K[x][p,q] : g(2 N + naux nocc_max + 2)      sum_L sum_i Ya^x_L[i,p] Ya^x_L[i,q]
    jk_df     J[p,q]    : g(N + N sum(nocc) + naux + 4)   sum_L Ab_L[p,q] R_L,
                          R_L = w sum_x sum_(i,q') Ya^x_L[i,q'] Ac^x[q',i],  w = 2 for ndm = 1
    jk_factor K[x][p,s] : g(2 N + naux N + 2)             sum_L (Ab_L |D_x| Ab_L)[p,s]
    jk_factor J[p,q]    : g(N N + ndm + naux + 4)         sum_L Ab_L[p,q] <Ab_L, sum_x |D_x|>

Each counts the roundings on the longest path from an input to the output element -- for K of jk_df: N additions
and a product for an element of Yt, naux nocc_max more for the sum over (L, i), two to spare; for J: an element of Yt
(N), the sum over (x, i, q') of rho, the doubling, the sum over L -- and a term of the sum that is multiplied by n
factors (1 + d), |d| <= u, is off by at most g(n) times its magnitude (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1).  They are derived, not measured.

The case table names, per slab of 64 auxiliary functions, the NBX_GEMM_KERNEL_* the Yt product of each spin and the K
product are meant to run on; tests/test_host_df_cases.py asks nbx_gemm_route -- the function nbx_gemm's launcher
calls -- for every one of them, and requires that the table holds an entry for each (product, kernel, beta) the
benchmark's shape, N = 2000 with n_occ = (512, 512), uses.

Section "not exact" (a kernel that is inexact for a correct, documented reason is held to a derived bound instead):
empty -- no kernel needed it.
"""

from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

import gemm_cases as gc
from gemm_cases import SMALL, T32, T64, T128, TN_DMA  # noqa: F401  (NBX_GEMM_KERNEL_* of include/nbx.h)

LS = 64  # DF_LS of nbed_amd/csrc/jk_df.hip: auxiliary functions per slab
EXP_RANGE = 12
U = 2.0 ** -53
LD = np.longdouble

# (N, naux, nocc, why, routes); routes: per slab, the kernel of the Yt product of each spin (None: the spin is empty,
# no product is formed) and then of the K product
Case = namedtuple("Case", "n naux nocc why routes")

CASES = [
    Case(1, 1, (1,), "the smallest size: one element, the tail of df_j_kernel alone", ((SMALL, SMALL),)),
    Case(2, 1, (1, 1), "the smallest even size: one vector pair", ((SMALL, SMALL, SMALL),)),
    Case(19, 5, (5, 4), "odd N (water / 6-31G* Cartesian)", ((SMALL, SMALL, SMALL),)),
    Case(24, 7, (6,), "one density (ndm = 1): rho doubled", ((SMALL, SMALL),)),
    Case(33, 65, (33, 1), "odd N; nocc = N; the transpose tile 32 | 33; a second slab of one",
         ((T32, SMALL, SMALL), (SMALL, SMALL, SMALL))),
    Case(97, 129, (32, 33), "odd N: vec = 0 operand staging in the tiled kernels; slabs of 64, 64 and 1",
         ((T32, T64, SMALL), (T32, T64, SMALL), (SMALL, SMALL, SMALL))),
    Case(148, 70, (70, 66), "the benchmark's small size; a last slab of six", ((T64, T64, T32), (SMALL, SMALL, SMALL))),
    Case(150, 130, (75, 0), "an empty spin; slabs of 64, 64 and 2",
         ((T64, None, T32), (T64, None, T32), (SMALL, None, SMALL))),
    Case(400, 64, (130,), "ndm = 1; Yt on the LDS-DMA kernel with the shared A (batch stride 0); exactly one slab",
         ((TN_DMA, T32),)),
    Case(400, 65, (130, 66), "alpha Yt on the LDS-DMA kernel and beta on 64 x 64 tiles in one slab; a last slab of one",
         ((TN_DMA, T64, T32), (SMALL, SMALL, T32))),
    Case(904, 129, (32, 31), "K on the LDS-DMA kernel with beta = 0, then beta = 1, at k = 64 * 32 = 2048 (the router's "
                             "threshold); the last slab (k = 32) accumulates onto its result from another kernel",
         ((T32, T32, TN_DMA), (T32, T32, TN_DMA), (SMALL, SMALL, T64))),
]
# the real-valued comparison: the longdouble reference costs too much beyond this; the larger shapes are covered exactly
REAL_MAX_N = 150
REAL_CASES = [c for c in CASES if c.n <= REAL_MAX_N]
# what the benchmark runs (bench.py: df_jk_leg, n2000_cycle)
BENCH_SHAPE = (2000, (512, 512))


def case_id(c: Case) -> str:
    return f"N{c.n}-L{c.naux}-occ{'x'.join(str(v) for v in c.nocc)}"


def by_shape(n: int, naux: int, nocc) -> Case:
    return next(c for c in CASES if (c.n, c.naux, c.nocc) == (n, naux, tuple(nocc)))


# ------------------------------------------------------------------------------------------ routing
Product = namedtuple("Product", "what spin shape beta")  # shape: gemm_cases.Case(m, n, k, batch)


def slab_products(n: int, naux: int, nocc):
    """The 'T','N' products nbx_jk_df hands nbx_gemm, slab by slab: Yt per non-empty spin (m = nocc[x], k = N, a batch
    of ls with A shared), then K (m = n = N, k = ls * nocc_max, a batch of ndm; beta = 1 from the second slab on)."""
    nmax = max(nocc)
    out = []
    if nmax == 0:
        return out
    for l0 in range(0, naux, LS):
        ls = min(LS, naux - l0)
        prods = [Product("yt", x, gc.Case(nocc[x], n, n, ls), 0.0) for x in range(len(nocc)) if nocc[x] > 0]
        prods.append(Product("k", None, gc.Case(n, n, ls * nmax, len(nocc)), 1.0 if l0 > 0 else 0.0))
        out.append(prods)
    return out


def library_routes(lib, n: int, naux: int, nocc):
    """What nbx_gemm_route answers for slab_products, in the layout of Case.routes.  The alignment flags are what
    nbx_gemm derives inside nbx_jk_df from allocations of their own: an even row length N (slab and spin strides are
    multiples of N)."""
    vec = 1 if n % 2 == 0 else 0
    out = []
    for prods in slab_products(n, naux, nocc):
        yt = {p.spin: gc.route(lib, "TN", p.shape, vec, vec) for p in prods if p.what == "yt"}
        k = next(gc.route(lib, "TN", p.shape, vec, vec) for p in prods if p.what == "k")
        out.append(tuple(yt.get(x) for x in range(len(nocc))) + (k,))
    return tuple(out)


def used_kernels(n: int, naux: int, nocc, routes):
    """{(product, kernel, beta)} of a shape whose routes are given in the layout of Case.routes."""
    out = set()
    for prods, slab in zip(slab_products(n, naux, nocc), routes):
        for p in prods:
            out.add((p.what, slab[p.spin] if p.what == "yt" else slab[-1], p.beta))
    return out


# ------------------------------------------------------------------------------------------ exact operands
Operands = namedtuple("Operands", "b c e")


def _sym_int8(rng, naux: int, n: int):
    a = (2 * rng.integers(0, 4, size=(naux, n, n), dtype=np.int8) - 3).astype(np.int8)  # {-3, -1, 1, 3}
    return np.tril(a) + np.tril(a, -1).transpose(0, 2, 1)


@lru_cache(maxsize=2)
def exact_operands(case: Case, seed: int = 0) -> Operands:
    """B (naux, N, N) symmetric with entries in {+-1, +-3}, C (ndm, N, N) with entries in {+-1, +-2} (a seed per spin)
    and the exponents e (N,) of the graded variant (read-only)."""
    n, naux, nocc = case.n, case.naux, case.nocc
    b = _sym_int8(np.random.default_rng([seed, n, naux, 20251021]), naux, n).astype(np.float64)
    c = np.stack([np.random.default_rng([seed, n, x, 7]).choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(n, n))
                  for x in range(len(nocc))])
    e = np.random.default_rng([seed, n, 3]).integers(-EXP_RANGE, EXP_RANGE + 1, size=n).astype(np.float64)
    for x in (b, c, e):
        x.setflags(write=False)
    return Operands(b, c, e)


def grade(e):
    """2^(e_p + e_q) as an (N, N) matrix."""
    return np.exp2(e[:, None] + e[None, :])


def graded(ops: Operands) -> Operands:
    """The graded variant of `ops` (module docstring): same integers, inputs spanning 2^(4 EXP_RANGE)."""
    return Operands(ops.b * grade(ops.e), ops.c * np.exp2(-ops.e)[None, :, None], ops.e)


def operands(case: Case, variant: str) -> Operands:
    assert variant in ("plain", "graded"), variant
    ops = exact_operands(case)
    return ops if variant == "plain" else graded(ops)


def occupied(c, nocc):
    """[C_occ^x (N, nocc[x])], contiguous."""
    return [np.ascontiguousarray(c[x][:, :nocc[x]]) for x in range(len(nocc))]


def densities(c, nocc):
    """D_x = C_occ^x C_occ^x^T (ndm, N, N): what jk_factor is handed (exact on the exact operands)."""
    return np.stack([co @ co.T for co in occupied(c, nocc)])


# ------------------------------------------------------------------------------------------ references
def jk_df_reference(b, c, nocc, dtype=np.float64):
    """(1 + ndm, N, N) = J, K_a[, K_b] of the module docstring's formulas, evaluated in `dtype`."""
    n, ndm = b.shape[-1], len(nocc)
    cos = [co.astype(dtype) for co in occupied(c, nocc)]
    w = 2.0 if ndm == 1 else 1.0
    out = np.zeros((1 + ndm, n, n), dtype=dtype)
    for bl in b:
        bl = bl.astype(dtype)
        rho = dtype(0.0)
        for x, co in enumerate(cos):
            yt = co.T @ bl
            out[1 + x] += yt.T @ yt
            rho = rho + (yt * co.T).sum()
        out[0] += (w * rho) * bl
    return out


def jk_factor_reference(b, dm, dtype=np.float64):
    """(1 + ndm, N, N) of HipBackend.jk_factor: J = sum_L B_L <B_L, sum_x D_x>, K_x = sum_L B_L D_x B_L; dm (N, N) or
    (ndm, N, N).  A density that is zero throughout gives K_x = 0 without the products."""
    n = b.shape[-1]
    dm = dm.reshape(-1, n, n).astype(dtype)
    dtot = dm.sum(axis=0)
    out = np.zeros((1 + dm.shape[0], n, n), dtype=dtype)
    live = [x for x in range(dm.shape[0]) if dm[x].any()]
    for bl in b:
        bl = bl.astype(dtype)
        out[0] += (bl * dtot).sum() * bl
        for x in live:
            out[1 + x] += bl @ dm[x] @ bl
    return out


def factor_from_df(ref, ndm: int):
    """jk_factor's result from jk_df's on the same orbitals: the same arrays, except that a single density is not
    doubled in J (a halving, exact)."""
    if ndm == 2:
        return ref
    out = ref.copy()
    out[0] *= 0.5
    return out


@lru_cache(maxsize=4)
def exact_reference(case: Case, variant: str):
    """jk_df_reference of operands(case, variant) (read-only)."""
    ops = operands(case, variant)
    ref = jk_df_reference(ops.b, ops.c, case.nocc)
    ref.setflags(write=False)
    return ref


def headroom(b, c, nocc) -> float:
    """The largest sum of |terms| any intermediate or output element has -- Yt, rho, K and J of the formulas evaluated
    on the absolute values (jk_factor's partial sums are bounded by the same: |D_x| <= Ac Ac^T).  Every partial sum a
    kernel can form is below it.  For the graded variant, call it on the plain operands: the integer parts are the same."""
    ab = np.abs(b)
    acs = [np.abs(co) for co in occupied(c, nocc)]
    w = 2.0 if len(nocc) == 1 else 1.0
    n = b.shape[-1]
    top = 0.0
    j = np.zeros((n, n))
    ks = [np.zeros((n, n)) for _ in acs]
    for al in ab:
        r = 0.0
        for x, ac in enumerate(acs):
            ya = ac.T @ al
            top = max(top, float(ya.max()) if ya.size else 0.0)
            ks[x] += ya.T @ ya
            r += float((ya * ac.T).sum())
        j += (w * r) * al
        top = max(top, w * r)
    return max([top, float(j.max())] + [float(k.max()) for k in ks])


# ------------------------------------------------------------------------------------------ the slab algorithm
MUTATIONS = ("drop_short_slab", "beta0_second_slab", "stale_rho", "stale_rows", "swap_spins", "no_factor2", "transposed_b",
             "skip_odd_tail")


def slab_algorithm(b, c, nocc, mutation: str = ""):
    """numpy restatement of nbx_jk_df as the kernels walk it: Yt rows of nocc_max per l with zero rows past a spin's own
    count, rho per slab, K and J accumulated from the second slab on, J over the flattened n2 = N^2 elements in pairs.
    `mutation`: one of MUTATIONS -- a defect of the kind the exact comparison is there to catch ("transposed_b" is the
    control: B_L is symmetric, so using it transposed changes nothing)."""
    assert mutation == "" or mutation in MUTATIONS, mutation
    naux, n = b.shape[0], b.shape[-1]
    ndm, nmax = len(nocc), max(nocc)
    n2 = n * n
    jk = np.zeros((1 + ndm, n, n))
    if naux == 0 or nmax == 0:
        return jk
    ct = [co.T.copy() for co in occupied(c, nocc)]
    yt = np.zeros((ndm, LS, nmax, n))
    rho = np.zeros(LS)
    for l0 in range(0, naux, LS):
        ls = min(LS, naux - l0)
        if mutation == "drop_short_slab" and l0 > 0 and ls < LS:
            continue
        for x in range(ndm):
            if nocc[x] == 0:
                continue
            for l in range(ls):
                bl = b[l0 + l].T if mutation == "transposed_b" else b[l0 + l]
                yt[x, l, :nocc[x]] = ct[x] @ bl
        if mutation == "stale_rows" and ndm == 2:
            yt[1, :ls, nocc[1]:nocc[0]] = yt[0, :ls, nocc[1]:nocc[0]]
        if not (mutation == "stale_rho" and l0 > 0):
            for l in range(ls):
                t = sum(float((yt[x, l, :nocc[x]] * ct[x]).sum()) for x in range(ndm))
                rho[l] = 2.0 * t if ndm == 1 and mutation != "no_factor2" else t
        beta = 0.0 if l0 == 0 or (mutation == "beta0_second_slab" and l0 == LS) else 1.0
        for x in range(ndm):
            y = yt[x, :ls].reshape(ls * nmax, n)
            jk[1 + x] = beta * jk[1 + x] + y.T @ y
        jflat = jk[0].reshape(-1)
        upto = n2 - 1 if mutation == "skip_odd_tail" and n2 % 2 else n2
        part = rho[:ls] @ b[l0:l0 + ls].reshape(ls, n2)
        jflat[:upto] = (jflat[:upto] if l0 > 0 else 0.0) + part[:upto]
    if mutation == "swap_spins" and ndm == 2:
        jk[[1, 2]] = jk[[2, 1]]
    return jk


# ------------------------------------------------------------------------------------------ real-valued operands
def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


@lru_cache(maxsize=2)
def real_operands(case: Case):
    """(B, C): synth.df_factor(N, 0, naux) and orthonormal orbitals per spin from the QR of a seeded normal matrix."""
    from nbed_amd import synth

    b = synth.df_factor(case.n, 0, case.naux)
    c = np.stack([np.linalg.qr(np.random.default_rng([case.n, x, 95]).standard_normal((case.n, case.n)))[0]
                  for x in range(len(case.nocc))])
    b.setflags(write=False)
    c.setflags(write=False)
    return b, c


def jk_df_bound(b, c, nocc):
    """(1 + ndm, N, N): the per-element bounds of nbx_jk_df (module docstring)."""
    n, naux, ndm = b.shape[-1], b.shape[0], len(nocc)
    ab = np.abs(b)
    acs = [np.abs(co) for co in occupied(c, nocc)]
    w = 2.0 if ndm == 1 else 1.0
    out = np.zeros((1 + ndm, n, n))
    for al in ab:
        r = 0.0
        for x, ac in enumerate(acs):
            ya = ac.T @ al
            out[1 + x] += ya.T @ ya
            r += float((ya * ac.T).sum())
        out[0] += (w * r) * al
    out[0] *= gamma(n + n * sum(nocc) + naux + 4)
    out[1:] *= gamma(2 * n + naux * max(nocc) + 2)
    return out


def jk_factor_bound(b, dm):
    """(1 + ndm, N, N): the per-element bounds of HipBackend.jk_factor (module docstring)."""
    n, naux = b.shape[-1], b.shape[0]
    ad = np.abs(dm.reshape(-1, n, n))
    ndm = ad.shape[0]
    ab = np.abs(b)
    out = np.zeros((1 + ndm, n, n))
    adtot = ad.sum(axis=0)
    for al in ab:
        out[0] += float((al * adtot).sum()) * al
        for x in range(ndm):
            out[1 + x] += al @ ad[x] @ al
    out[0] *= gamma(n * n + ndm + naux + 4)
    out[1:] *= gamma(2 * n + naux * n + 2)
    return out


Real = namedtuple("Real", "b c dm df_ref df_bound factor_ref factor_bound")


@lru_cache(maxsize=1)
def real_case(case: Case) -> Real:
    """Operands, the float64 densities jk_factor is handed, the longdouble references of both entry points and their
    bounds (read-only).  ndm = 1: dm is the single (N, N) density."""
    b, c = real_operands(case)
    dm = densities(c, case.nocc)
    if len(case.nocc) == 1:
        dm = dm[0]
    out = Real(b, c, dm, jk_df_reference(b, c, case.nocc, LD), jk_df_bound(b, c, case.nocc),
               jk_factor_reference(b, dm, LD), jk_factor_bound(b, dm))
    for x in out:
        x.setflags(write=False)
    return out


def worst_ratio(got, ref, bound) -> float:
    """max |got - ref| / bound over the elements (the difference taken in the reference's precision); an element whose
    bound is zero -- K of an empty spin -- has to be exactly the reference."""
    err = np.abs(np.asarray(got).astype(ref.dtype) - ref).astype(np.float64)
    assert not np.isnan(err).any()
    zero = bound == 0
    assert not err[zero].any(), "an element with a zero bound differs from the reference"
    return float(np.max(err[~zero] / bound[~zero])) if (~zero).any() else 0.0


# ------------------------------------------------------------------------------------------ the comparison
def assert_exact(got, ref, what: str = ""):
    """Every element, every bit (NaN anywhere fails); the message names the first offending rows."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(got == ref)
    if bad.any():
        where = np.argwhere(bad)
        lead = sorted({tuple(int(v) for v in w[:-1]) for w in where[:2000]})[:3]
        rows = "; ".join(f"{ix}: got {got[ix][:6]} want {ref[ix][:6]}" for ix in lead)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(where[0])}; rows {rows}")


def differs(got, ref) -> bool:
    return bool((~(np.asarray(got) == np.asarray(ref))).any())
