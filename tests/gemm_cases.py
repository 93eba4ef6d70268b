"""Shared by tests/test_host_gemm_cases.py (CPU) and tests/test_gpu_gemm.py (MI355X): a shape for every kernel
behind nbx_gemm in every operand layout it serves, operands whose product is exact in float64, and real-valued
operands with the rounding bound a float64 product has to meet.

nbx_gemm (nbed_amd/csrc/gemm.hip) is five kernels -- gemm_small_kernel, gemm_f64_kernel with 32 x 32, 64 x 64 and
128 x 128 tiles, and the LDS-DMA kernel gemm_m4_tn_kernel ('T','N' only) -- each instantiated per op(A)/op(B) layout.
Which one a product runs on is decided by thresholds that get retuned; nbx_gemm_route reports the decision, and
TABLE below names the kernel every shape is MEANT to reach, so that a retuning which empties a test fails
tests/test_host_gemm_cases.py instead of passing unnoticed.

Exact operands.  Entries are integers drawn uniformly from [-2^p, 2^p], alpha and beta are powers of two, and p is
the largest integer with  k 2^(2p) |alpha| + |beta| 2^p < 2^52  for every (alpha, beta) in ALPHA_BETA.  Every product
is then an integer multiple of min(1, |alpha|) >= 1/2 and every partial sum of alpha op(A) op(B) + beta C0, in any
order, stays below 2^52 in magnitude: each is a float64, so any summation order, with or without FMA, gives the same
bits, and numpy's float64 product IS the answer.  The operands carry p + 1 >= 20 significant bits, their products 40
and more: an accumulator narrower than float64 cannot hold them.

Real-valued operands.  Entries +-10^u, u uniform in [-6, 6], signs mixed so that results cancel.  The reference is
xc_reference.matmul (longdouble, or error-free products where that is no wider).  The bound is

    |got - ref| <= (k + 4) eps (|alpha| (|op(A)| |op(B)|) + |beta C0|),   eps = 2^-52,

per entry: a length-k dot product accumulated in any order, fused or not, has every term a_i b_i multiplied by at
most k factors (1 + d), |d| <= u = eps / 2 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1);
the multiplication by alpha and the fma with beta C0 add one such factor each, to the term beta C0 only the last:
gamma_(k+2) = (k + 2) u / (1 - (k + 2) u) < (k + 4) eps for every k here.  It is derived, not measured.
"""

from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

NONE, SMALL, T32, T64, T128, TN_DMA = range(6)  # NBX_GEMM_KERNEL_* of include/nbx.h
KERNEL_NAMES = {NONE: "NONE", SMALL: "SMALL", T32: "T32", T64: "T64", T128: "T128", TN_DMA: "TN_DMA"}
LAYOUTS = ("NN", "NT", "TN", "TT")  # trans_a + trans_b
EPS = float(np.finfo(np.float64).eps)
ALPHA_BETA = ((1.0, 0.0), (0.5, -2.0))  # what the exact-operand tests run with

Case = namedtuple("Case", "m n k batch")

# kernel -> shapes (m, n, k, batch) meant to reach it, in every layout of LAYOUTS_OF[kernel]
TABLE = {
    SMALL: [Case(1, 1, 1, 1), Case(17, 31, 5, 1), Case(148, 148, 148, 1),
            Case(16, 16, 4096, 1),   # k at the small kernel's limit
            Case(352, 368, 3, 1)],   # 506 tiles of 16 x 16, just under its 512
    T32: [Case(353, 368, 3, 1),      # one row past the small kernel's tile limit
          Case(16, 16, 4097, 1),     # k one past its k limit
          Case(5, 9000, 7, 1), Case(9000, 5, 7, 1), Case(399, 401, 37, 1),
          Case(4, 4, 4, 70000)],     # two batch chunks (a grid's z extent ends at 65535)
    T64: [Case(700, 777, 19, 1), Case(130, 200, 21, 12), Case(33, 33, 5, 128), Case(64, 8256, 6, 1)],
    T128: [Case(129, 131, 9, 128), Case(65, 65, 5, 512),
           Case(130, 134, 22, 128)],  # 'T','N' with k % 4 != 0 must stay off the DMA kernel
    TN_DMA: [Case(130, 134, 4, 128),     # one 4-row step
             Case(130, 134, 20, 128),    # two and a half k-tiles, the last a single step; row and column edge in every tile
             Case(66, 16400, 2048, 1),   # the `tiles128 >= 128 && k >= 2048` door
             Case(128, 70000, 20, 1)],
}
LAYOUTS_OF = {SMALL: LAYOUTS, T32: LAYOUTS, T64: LAYOUTS, T128: LAYOUTS, TN_DMA: ("TN",)}
# where the DMA shapes go in the layouts (and with the operand alignment) the DMA kernel does not take
DMA_FALLBACK = {Case(130, 134, 4, 128): T128, Case(130, 134, 20, 128): T128, Case(66, 16400, 2048, 1): T64,
                Case(128, 70000, 20, 1): T128}


def intended(kernel: int, case: Case, layout: str) -> int:
    """The kernel `case`, listed under `kernel`, is meant to run on in `layout` (aligned, even-ld operands)."""
    if kernel == TN_DMA and layout != "TN":
        return DMA_FALLBACK[case]
    return kernel


def all_entries():
    """(intended kernel, case, layout) for every table entry in every layout, case-major (operands are cached per case)."""
    return [(intended(kern, case, lay), case, lay) for kern, cases in TABLE.items() for case in cases for lay in LAYOUTS]


def entry_id(entry) -> str:
    kern, case, lay = entry
    return f"{KERNEL_NAMES[kern]}-{case.m}x{case.n}x{case.k}x{case.batch}-{lay}"


def route(lib, layout: str, case: Case, vec_a: int = 1, vec_b: int = 1) -> int:
    return lib.nbx_gemm_route(layout[0].encode(), layout[1].encode(), case.m, case.n, case.k, case.batch, vec_a, vec_b)


# ------------------------------------------------------------------------------------------ storage
def stored(x, trans: bool):
    """Logical op(X) (..., rows, cols) -> what nbx_gemm is handed: the row-major array itself ('N' for A, 'N' for B)
    or its transpose.  Works on numpy arrays and torch tensors alike."""
    if not trans:
        return x
    t = x.swapaxes(-1, -2)
    return np.ascontiguousarray(t) if isinstance(t, np.ndarray) else t.contiguous()


# ------------------------------------------------------------------------------------------ exact operands
def exact_bits(k: int) -> int:
    """Largest p with k 2^(2p) |alpha| + |beta| 2^p < 2^52 for every (alpha, beta) of ALPHA_BETA."""
    p = 0
    while all(k * 4 ** (p + 1) * abs(al) + abs(be) * 2 ** (p + 1) < 2 ** 52 for al, be in ALPHA_BETA):
        p += 1
    return p


@lru_cache(maxsize=2)
def exact_operands(case: Case, seed: int = 0):
    """Integer-valued float64 op(A) (batch, m, k), op(B) (batch, k, n), C0 (batch, m, n) (read-only; see the module's
    docstring).  The bound that makes every summation order exact is asserted on the arrays themselves."""
    m, n, k, batch = case
    p = exact_bits(k)
    rng = np.random.default_rng([seed, m, n, k, batch])
    lim = 2 ** p
    a, b, c0 = (rng.integers(-lim, lim + 1, size=shape).astype(np.float64)
                for shape in ((batch, m, k), (batch, k, n), (batch, m, n)))
    amax, bmax, cmax = (float(np.abs(x).max()) if x.size else 0.0 for x in (a, b, c0))
    for al, be in ALPHA_BETA:
        assert np.log2(abs(al)) % 1 == 0 and (be == 0 or np.log2(abs(be)) % 1 == 0)
        assert k * amax * bmax * abs(al) + abs(be) * cmax < 2.0 ** 52, (case, p)
    assert p >= 19, (case, p)  # (20 significant bits per operand at every k of the table)
    for x in (a, b, c0):
        x.setflags(write=False)
    return a, b, c0


@lru_cache(maxsize=2)
def exact_product(case: Case, seed: int = 0):
    """op(A) op(B) of exact_operands: float64 (BLAS), exact whatever order it sums in."""
    a, b, _ = exact_operands(case, seed)
    prod = np.matmul(a, b)
    prod.setflags(write=False)
    return prod


def exact_reference(case: Case, alpha: float, beta: float, seed: int = 0):
    """alpha op(A) op(B) + beta C0, exact (beta = 0: C0 is not read)."""
    prod = exact_product(case, seed)
    if beta == 0.0:
        return alpha * prod
    return alpha * prod + beta * exact_operands(case, seed)[2]


# ------------------------------------------------------------------------------------------ real-valued operands
REAL_ALPHA_BETA = (-0.75, 1.5)


def real_entries(rng, shape):
    """+-10^u, u uniform in [-6, 6]."""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-6.0, 6.0, size=shape)


@lru_cache(maxsize=8)
def real_operands(case: Case, seed: int = 0):
    """op(A), op(B), C0 with entries +-10^u, u uniform in [-6, 6]; then the extended-precision reference of
    alpha op(A) op(B) + beta C0 for (alpha, beta) = REAL_ALPHA_BETA and the per-entry rounding bound (module docstring).
    Returns (a, b, c0, ref, bound)."""
    import xc_reference as xr

    m, n, k, batch = case
    rng = np.random.default_rng([seed, m, n, k, batch, 1])
    a, b, c0 = real_entries(rng, (batch, m, k)), real_entries(rng, (batch, k, n)), real_entries(rng, (batch, m, n))
    alpha, beta = REAL_ALPHA_BETA
    prod = np.stack([np.asarray(xr.matmul(a[z], b[z]), dtype=xr.LD) for z in range(batch)])
    ref = alpha * prod + beta * c0.astype(xr.LD)
    bound = (k + 4) * EPS * (abs(alpha) * np.matmul(np.abs(a), np.abs(b)) + np.abs(beta * c0))
    for x in (a, b, c0, ref, bound):
        x.setflags(write=False)
    return a, b, c0, ref, bound


def worst_ratio(got, ref, bound) -> float:
    """max |got - ref| / bound over the entries (the difference taken in the reference's precision)."""
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    assert np.all(bound > 0)
    return float(np.max(err / bound))
