"""CPU checks of tests/gemm_cases.py: every table entry reaches the kernel it is meant to reach by the library's own
routing function (nbx_gemm_route: the function nbx_gemm's launcher calls, host arithmetic only), every kernel is in
the table under every layout it serves, and the references the GPU tests compare with are what they claim to be."""

from fractions import Fraction

import numpy as np
import pytest

import gemm_cases as gc
from gemm_cases import Case
from nbed_amd import _nbx


@pytest.fixture(scope="module")
def lib():
    return _nbx.load_library()


def test_kernel_ids_mirror_the_header():
    header = (_nbx.LIB_PATH.parent.parent / "include" / "nbx.h").read_text()
    for kern, name in gc.KERNEL_NAMES.items():
        assert f"#define NBX_GEMM_KERNEL_{name} {kern} " in header, name
    assert (_nbx.GEMM_KERNEL_NONE, _nbx.GEMM_KERNEL_SMALL, _nbx.GEMM_KERNEL_T32, _nbx.GEMM_KERNEL_T64, _nbx.GEMM_KERNEL_T128,
            _nbx.GEMM_KERNEL_TN_DMA) == (gc.NONE, gc.SMALL, gc.T32, gc.T64, gc.T128, gc.TN_DMA)


@pytest.mark.parametrize("entry", gc.all_entries(), ids=gc.entry_id)
def test_table_entry_reaches_its_kernel(lib, entry):
    kern, case, layout = entry
    assert gc.KERNEL_NAMES[gc.route(lib, layout, case)] == gc.KERNEL_NAMES[kern]
    assert gc.route(lib, layout.lower(), case) == kern  # lower-case flags as nbx_gemm takes them


@pytest.mark.parametrize("case", gc.TABLE[gc.TN_DMA], ids=str)
def test_dma_shapes_leave_the_dma_kernel_when_it_does_not_apply(lib, case):
    """Other layouts, and 'T','N' with an operand the load unit cannot fetch 16 bytes at a time (vec = 0)."""
    fallback = gc.DMA_FALLBACK[case]
    assert fallback in (gc.T64, gc.T128)
    assert gc.route(lib, "TN", case) == gc.TN_DMA
    for layout in ("NN", "NT", "TT"):
        assert gc.route(lib, layout, case) == fallback, layout
    for vec_a, vec_b in ((0, 1), (1, 0), (0, 0)):
        assert gc.route(lib, "TN", case, vec_a, vec_b) == fallback, (vec_a, vec_b)


def test_every_kernel_is_in_the_table_under_every_layout_it_serves(lib):
    reached = {(gc.route(lib, layout, case), layout) for _, case, layout in gc.all_entries()}
    want = {(kern, layout) for kern, layouts in gc.LAYOUTS_OF.items() for layout in layouts}
    assert reached == want
    assert set(gc.TABLE) == {gc.SMALL, gc.T32, gc.T64, gc.T128, gc.TN_DMA}
    # only the DMA kernel looks at the alignment flags
    for kern, case, layout in gc.all_entries():
        if kern != gc.TN_DMA:
            assert gc.route(lib, layout, case, 0, 0) == kern, (case, layout)


def test_route_edges(lib):
    """Nothing to launch; the thresholds the table's neighbours sit on; a batch past one grid answers for its first chunk."""
    for case in (Case(0, 5, 5, 1), Case(5, 0, 5, 1), Case(5, 5, 5, 0)):
        assert gc.route(lib, "NN", case) == gc.NONE
    assert gc.route(lib, "NN", Case(5, 5, 0, 1)) == gc.SMALL  # k = 0: C <- beta C by the small kernel
    assert gc.route(lib, "TN", Case(700, 777, 0, 1)) == gc.T64
    # 512 tiles of 16 x 16 is still the small kernel's, 513 is not
    assert gc.route(lib, "NN", Case(16, 16, 8, 512)) == gc.SMALL
    assert gc.route(lib, "NN", Case(16, 16, 8, 513)) == gc.T32
    # one chunk of 65535 and the rest: the answer is the first chunk's (128 x 128 x 65535 tiles, not x 70000)
    assert gc.route(lib, "NN", Case(4, 4, 4, 65535)) == gc.route(lib, "NN", Case(4, 4, 4, 70000)) == gc.T32
    # the DMA kernel's own conditions: even extents, k % 4 == 0, more than 64 rows and columns
    for case in (Case(131, 134, 20, 128), Case(130, 135, 20, 128), Case(130, 134, 21, 128), Case(130, 134, 2, 128)):
        assert gc.route(lib, "TN", case) == gc.T128, case
    assert gc.route(lib, "TN", Case(64, 134, 20, 512)) == gc.T64  # (64 rows: neither the DMA kernel nor 128 x 128 tiles)


def test_exact_reference_is_exact():
    """The float64 product of the integer operands equals their product as Python integers, and so does the
    alpha / beta form (halves are exact too)."""
    for case in (Case(17, 31, 5, 1), Case(33, 33, 5, 128)):
        a, b, c0 = gc.exact_operands(case)
        assert all(np.array_equal(x, np.rint(x)) for x in (a, b, c0))
        assert max(np.abs(a).max(), np.abs(b).max()) > 2 ** (gc.exact_bits(case.k) - 1)  # (the range is used)
        ai, bi, ci = (np.vectorize(int, otypes=[object])(x) for x in (a, b, c0))
        prod = np.matmul(ai, bi)  # object dtype: Python integers, no rounding anywhere
        got = gc.exact_reference(case, 1.0, 0.0)
        assert got.dtype == np.float64 and np.array_equal(np.vectorize(int, otypes=[object])(got), prod)
        assert all(float(v) == v for v in prod.ravel())
        half = gc.exact_reference(case, 0.5, -2.0)
        want2 = prod - 4 * ci  # twice the answer, an integer
        assert np.array_equal(np.vectorize(int, otypes=[object])(2.0 * half), want2)
        assert np.abs(half).max() < 2.0 ** 52


def test_exact_bits_is_the_largest_that_keeps_the_bound():
    for k in (1, 3, 5, 148, 2048, 4096, 4097):
        p = gc.exact_bits(k)
        assert all(k * 4 ** p * abs(al) + abs(be) * 2 ** p < 2 ** 52 for al, be in gc.ALPHA_BETA)
        assert any(k * 4 ** (p + 1) * abs(al) + abs(be) * 2 ** (p + 1) >= 2 ** 52 for al, be in gc.ALPHA_BETA)
        assert p >= 19


def test_real_reference_and_float64_product_stay_inside_the_bound():
    """Fraction arithmetic is the truth: the extended-precision reference is far inside the bound, and a plain
    float64 product (numpy) is inside it -- the bound is one a correct float64 GEMM meets."""
    case = Case(17, 31, 5, 1)
    a, b, c0, ref, bound = gc.real_operands(case)
    alpha, beta = gc.REAL_ALPHA_BETA
    assert (a < 0).any() and (a > 0).any() and np.abs(a).max() / np.abs(a).min() > 1e6
    fa, fb, fc = ([[Fraction(float(v)) for v in row] for row in x[0]] for x in (a, b, c0))
    truth = [[Fraction(alpha) * sum(fa[i][q] * fb[q][j] for q in range(case.k)) + Fraction(beta) * fc[i][j]
              for j in range(case.n)] for i in range(case.m)]
    plain = alpha * (a[0] @ b[0]) + beta * c0[0]
    worst_ref = worst_plain = 0.0
    for i in range(case.m):
        for j in range(case.n):
            bd = Fraction(float(bound[0, i, j]))
            # (a longdouble is a sum of two float64 exactly enough: hi + lo below)
            hi = float(ref[0, i, j])
            lo = float(ref[0, i, j] - type(ref[0, i, j])(hi))
            worst_ref = max(worst_ref, float(abs(Fraction(hi) + Fraction(lo) - truth[i][j]) / bd))
            worst_plain = max(worst_plain, float(abs(Fraction(float(plain[i, j])) - truth[i][j]) / bd))
    print(f"reference / bound {worst_ref:.2e}, float64 numpy / bound {worst_plain:.2e}")
    assert worst_ref < 0.1  # (a reference rounded to float64 is within 1 / (2 (k + 4)) of it; longdouble far closer)
    assert worst_plain <= 1.0
    assert gc.worst_ratio(plain[None], ref, bound) <= 1.0
    # cancellation is there: some results are far smaller than the products that made them
    assert np.min(np.abs(plain) / (bound[0] / ((case.k + 4) * gc.EPS))) < 0.2
