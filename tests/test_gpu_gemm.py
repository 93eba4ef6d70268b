"""nbx_gemm on the MI355X, every kernel and operand layout (tests/gemm_cases.py has the case table, the operands and
the reasoning): bit-exact against integer-valued operands whose product float64 holds exactly, through be.gemm_raw
so that leading dimensions, batch strides and base alignment are the test's; NaN sentinels round every operand and
result; and real-valued operands against an extended-precision reference within the derived rounding bound.
Before a product is compared, nbx_gemm_route has to name the kernel the case is there for."""

from collections import Counter

import numpy as np
import pytest

import gemm_cases as gc
from gemm_cases import Case

# (the shared operands are read-only numpy arrays; torch warns when it wraps one, and nothing here writes through it)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

SENTINEL_BITS = 0x7FF8DEAD0000BEEF  # a NaN no kernel produces: whatever is not operand or result holds it


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


class Placed:
    """A (batch, rows, cols) device array laid out with leading dimension `ld` and batch stride `stride`, `offset`
    doubles into a buffer of sentinels (stride = 0: one matrix, read by every batch entry)."""

    def __init__(self, be, x3, ld=None, stride=None, offset=0, tail=5):
        t = self.torch = be.torch
        batch, rows, cols = x3.shape
        self.ld = cols if ld is None else ld
        self.stride = rows * self.ld if stride is None else stride
        assert self.ld >= cols and (self.stride == 0 and batch == 1 or self.stride >= rows * self.ld)
        span = offset + (batch - 1) * self.stride + (rows - 1) * self.ld + cols
        self.buf = t.full((span + tail,), SENTINEL_BITS, dtype=t.int64, device=be.device).view(t.float64)
        assert self.buf.data_ptr() % 16 == 0
        self.dims = ((batch, rows, cols), (self.stride, self.ld, 1), offset)
        self.view = t.as_strided(self.buf, *self.dims)
        self.view.copy_(x3)
        self.ptr = self.buf[offset:]
        # what nbx_gemm derives from the address: 16-byte loads of this operand are possible
        self.vec = int(self.ptr.data_ptr() % 16 == 0 and self.ld % 2 == 0 and self.stride % 2 == 0)

    def host(self):
        return self.view.cpu().numpy()

    def sentinels_untouched(self) -> bool:
        outside = self.buf.new_ones(self.buf.shape, dtype=self.torch.bool)
        outside.as_strided(*self.dims).fill_(False)
        return bool((self.buf.view(self.torch.int64)[outside] == SENTINEL_BITS).all())


def gemm(be, layout, case, alpha, a, b, beta, c):
    be.gemm_raw(layout[0], layout[1], case.m, case.n, case.k, alpha, a.ptr, a.ld, a.stride, b.ptr, b.ld, b.stride, beta,
                c.ptr, c.ld, c.stride, case.batch)


def nan_like(be, case):
    return be.torch.full((case.batch, case.m, case.n), float("nan"), dtype=be.torch.float64, device=be.device)


_DEV = {}


def on_device(be, kind, case):
    """The logical operands of a case on the device, one case at a time (the largest is 270 MB)."""
    if _DEV.get("key") != (kind, case):
        _DEV.clear()
        src = gc.exact_operands(case) if kind == "exact" else gc.real_operands(case)[:3]
        _DEV.update(key=(kind, case), val=tuple(be.asarray(x) for x in src))
    return _DEV["val"]


def even(x):
    return x + (x & 1)


def place_ab(be, layout, a3, b3, **kw):
    return Placed(be, gc.stored(a3, layout[0] == "T"), **kw), Placed(be, gc.stored(b3, layout[1] == "T"), **kw)


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))


# ---------------------------------------------------------------- every table entry x layout, exact
CENSUS = Counter()
ENTRIES = gc.all_entries()


@pytest.mark.parametrize("entry", ENTRIES, ids=gc.entry_id)
def test_gemm_exact(be, entry):
    """alpha = 1, beta = 0 into a C full of NaN (beta == 0 must not read C), then alpha = 1/2, beta = -2: equal to the
    exact answer in every bit, on the kernel the table says."""
    kern, case, layout = entry
    a3, b3, c03 = on_device(be, "exact", case)
    a, b = place_ab(be, layout, a3, b3)
    assert gc.KERNEL_NAMES[gc.route(be.lib, layout, case, a.vec, b.vec)] == gc.KERNEL_NAMES[kern]
    c = Placed(be, nan_like(be, case))
    gemm(be, layout, case, 1.0, a, b, 0.0, c)
    np.testing.assert_array_equal(c.host(), gc.exact_reference(case, 1.0, 0.0))
    c = Placed(be, c03)
    gemm(be, layout, case, 0.5, a, b, -2.0, c)
    np.testing.assert_array_equal(c.host(), gc.exact_reference(case, 0.5, -2.0))
    assert c.sentinels_untouched() and a.sentinels_untouched() and b.sentinels_untouched()
    CENSUS[(kern, layout)] += 1


def test_gemm_exact_route_census():
    """Which kernel x layout the exact-operand test went through (printed), and that it was all of them."""
    for kern in (gc.SMALL, gc.T32, gc.T64, gc.T128, gc.TN_DMA):
        print(f"{gc.KERNEL_NAMES[kern]:7s}", "  ".join(f"{lay}: {CENSUS[(kern, lay)]:2d}" for lay in gc.LAYOUTS))
    if sum(CENSUS.values()) == len(ENTRIES):  # (a partial selection of the test above has a partial census)
        for kern, layouts in gc.LAYOUTS_OF.items():
            for lay in gc.LAYOUTS:
                assert (CENSUS[(kern, lay)] > 0) == (lay in layouts), (gc.KERNEL_NAMES[kern], lay)


# ---------------------------------------------------------------- leading dimensions
EDGE_CASE = {gc.SMALL: Case(17, 31, 5, 1), gc.T32: Case(399, 401, 37, 1), gc.T64: Case(130, 200, 21, 12),
             gc.T128: Case(129, 131, 9, 128), gc.TN_DMA: Case(130, 134, 20, 128)}
EDGE_ENTRIES = [(kern, case, lay) for kern, case in EDGE_CASE.items() for lay in gc.LAYOUTS_OF[kern]]


def test_edge_cases_are_table_entries():
    for kern, case in EDGE_CASE.items():
        assert case in gc.TABLE[kern]
        # a partial last tile in rows, columns and k of that kernel
        tile, ktile = {gc.SMALL: (16, 16), gc.T32: (32, 16), gc.T64: (64, 16), gc.T128: (128, 16), gc.TN_DMA: (128, 8)}[kern]
        assert case.m % tile and case.n % tile and case.k % ktile


@pytest.mark.parametrize("entry", EDGE_ENTRIES, ids=gc.entry_id)
@pytest.mark.parametrize("pads", [(3, 3, 3), (4, 4, 4), (4, 4, 3)], ids=lambda p: "ld+%d+%d+%d" % p)
def test_gemm_leading_dimensions(be, entry, pads):
    """A, B and C inside larger buffers (ld = row + 3 or + 4, sentinels between the rows and round the matrices): the
    result is exact and no sentinel of C's buffer has changed.  'T','N' with even lda, ldb stays on the DMA kernel,
    whose epilogue stores 16 bytes at a time when ldc is even and element by element when it is odd."""
    kern, case, layout = entry
    a3, b3, c03 = on_device(be, "exact", case)
    sa, sb = gc.stored(a3, layout[0] == "T"), gc.stored(b3, layout[1] == "T")
    a = Placed(be, sa, ld=sa.shape[2] + pads[0])
    b = Placed(be, sb, ld=sb.shape[2] + pads[1])
    got_route = gc.route(be.lib, layout, case, a.vec, b.vec)
    if kern == gc.TN_DMA:
        assert got_route == (gc.TN_DMA if pads[0] % 2 == 0 and pads[1] % 2 == 0 else gc.DMA_FALLBACK[case])
    else:
        assert got_route == kern
    for alpha, beta in gc.ALPHA_BETA:
        c = Placed(be, nan_like(be, case) if beta == 0.0 else c03, ld=case.n + pads[2])
        gemm(be, layout, case, alpha, a, b, beta, c)
        np.testing.assert_array_equal(c.host(), gc.exact_reference(case, alpha, beta))
        assert c.sentinels_untouched()
    assert a.sentinels_untouched() and b.sentinels_untouched()


# ---------------------------------------------------------------- scalar staging (vec = 0)
@pytest.mark.parametrize("entry", [e for e in EDGE_ENTRIES if e[0] in (gc.T32, gc.T64, gc.T128)], ids=gc.entry_id)
def test_gemm_scalar_staging(be, entry):
    """The operands' base advanced by one double, and odd leading dimensions: gemm_f64_kernel stages such an operand
    element by element (vec_a / vec_b = 0) instead of in pairs.  Same bits as the aligned run, exact operands (= the
    reference) and real-valued ones."""
    kern, case, layout = entry
    for kind in ("exact", "real"):
        a3, b3, _ = on_device(be, kind, case)
        sa, sb = gc.stored(a3, layout[0] == "T"), gc.stored(b3, layout[1] == "T")
        lda, ldb = even(sa.shape[2]), even(sb.shape[2])
        results = []
        for off_a, ld_a, off_b, ld_b in ((0, lda, 0, ldb), (1, lda, 0, ldb), (0, lda, 1, ldb), (0, lda + 1, 0, ldb),
                                         (0, lda, 0, ldb + 1), (1, lda + 1, 1, ldb + 1)):
            a = Placed(be, sa, ld=ld_a, stride=even(sa.shape[1] * ld_a), offset=off_a)
            b = Placed(be, sb, ld=ld_b, stride=even(sb.shape[1] * ld_b), offset=off_b)
            assert (a.vec, b.vec) == (int(off_a == 0 and ld_a == lda), int(off_b == 0 and ld_b == ldb))
            assert gc.route(be.lib, layout, case, a.vec, b.vec) == kern
            c = Placed(be, nan_like(be, case))
            gemm(be, layout, case, 1.0, a, b, 0.0, c)
            results.append(c.host())
        if kind == "exact":
            np.testing.assert_array_equal(results[0], gc.exact_reference(case, 1.0, 0.0))
        for r in results[1:]:
            assert same_bits(r, results[0])


@pytest.mark.parametrize("case", gc.TABLE[gc.TN_DMA], ids=str)
def test_gemm_dma_shapes_with_misaligned_a(be, case):
    """The DMA kernel fetches 16 bytes per lane: an A one double off its alignment has to go to another kernel
    (nbx_gemm_route says which) and come out exact."""
    a3, b3, _ = on_device(be, "exact", case)
    a = Placed(be, gc.stored(a3, True), offset=1)
    b = Placed(be, b3)
    assert (a.vec, b.vec) == (0, 1)
    assert gc.route(be.lib, "TN", case, a.vec, b.vec) == gc.DMA_FALLBACK[case]
    c = Placed(be, nan_like(be, case))
    gemm(be, "TN", case, 1.0, a, b, 0.0, c)
    np.testing.assert_array_equal(c.host(), gc.exact_reference(case, 1.0, 0.0))


# ---------------------------------------------------------------- batch addressing
BATCH_CASE = {gc.SMALL: Case(17, 31, 5, 3), gc.T32: Case(4, 4, 4, 70000), gc.T64: Case(130, 200, 21, 12),
              gc.T128: Case(129, 131, 9, 128), gc.TN_DMA: Case(130, 134, 20, 128)}
BATCH_ENTRIES = [(kern, case, lay) for kern, case in BATCH_CASE.items() for lay in gc.LAYOUTS_OF[kern]]


@pytest.mark.parametrize("entry", BATCH_ENTRIES, ids=gc.entry_id)
def test_gemm_batch_addressing(be, entry):
    """stride_a = 0 (one A for every entry) with a B per entry, stride_b = 0 with an A per entry, odd strides, and a
    stride_c larger than a matrix with sentinels in the gaps; the 70000 entries of the chunked case include 65534,
    65535 and 65536, the last of the first grid and the first two of the second."""
    kern, case, layout = entry
    m, n, k, batch = case
    a3, b3, c03 = on_device(be, "exact", case)
    ah, bh, ch = gc.exact_operands(case)
    sa, sb = gc.stored(a3, layout[0] == "T"), gc.stored(b3, layout[1] == "T")

    def check(c, want):
        got = c.host()
        if batch > 65535:
            for z in (65534, 65535, 65536):
                np.testing.assert_array_equal(got[z], want[z], err_msg=f"batch entry {z}")
        np.testing.assert_array_equal(got, want)
        assert c.sentinels_untouched()

    # one A, a B per entry; the C blocks six doubles apart
    a, b = Placed(be, sa[:1], stride=0), Placed(be, sb, stride=even(sb.shape[1] * sb.shape[2]) + 2)
    assert gc.route(be.lib, layout, case, a.vec, b.vec) == kern
    c = Placed(be, c03, stride=m * n + 6)
    gemm(be, layout, case, 0.5, a, b, -2.0, c)
    check(c, 0.5 * np.matmul(ah[:1], bh) - 2.0 * ch)
    # an A per entry, one B; the C blocks an odd distance apart (every other one off 16-byte alignment)
    a, b = Placed(be, sa, stride=even(sa.shape[1] * sa.shape[2]) + 2), Placed(be, sb[:1], stride=0)
    assert gc.route(be.lib, layout, case, a.vec, b.vec) == kern
    c = Placed(be, nan_like(be, case), stride=m * n + 5 + (m * n) % 2)
    assert c.stride % 2 == 1
    gemm(be, layout, case, 1.0, a, b, 0.0, c)
    check(c, np.matmul(ah, bh[:1]))
    # odd strides of A and B: staged element by element, and never by the DMA kernel
    a = Placed(be, sa, stride=even(sa.shape[1] * sa.shape[2]) + 3)
    b = Placed(be, sb, stride=even(sb.shape[1] * sb.shape[2]) + 1)
    assert (a.vec, b.vec) == (0, 0)
    assert gc.route(be.lib, layout, case, 0, 0) == (gc.DMA_FALLBACK[case] if kern == gc.TN_DMA else kern)
    c = Placed(be, c03, stride=m * n + 7)
    gemm(be, layout, case, 0.5, a, b, -2.0, c)
    check(c, gc.exact_reference(case, 0.5, -2.0) if case in gc.TABLE[kern] else 0.5 * np.matmul(ah, bh) - 2.0 * ch)


# ---------------------------------------------------------------- NaN containment
@pytest.mark.parametrize("entry", EDGE_ENTRIES, ids=gc.entry_id)
def test_gemm_nan_stays_in_its_row_and_column(be, entry):
    """One NaN in op(A)[i, kk], i in the last (partial) row tile and kk in the last (partial) k-tile: row i of C is
    NaN and every other entry has the bits of the clean run; the same for a NaN in op(B)[kk, j] and column j.  An edge
    mask that multiplies what it should have replaced, or a tile that takes a neighbour's element, does not pass."""
    kern, case, layout = entry
    m, n, k, batch = case
    a3, b3, _ = on_device(be, "exact", case)
    want = gc.exact_reference(case, 1.0, 0.0)
    z, i, j, kk = batch - 1, m - 1, n - 1, k - 1
    for which in ("clean", "a", "b"):
        a3n, b3n, expect = a3, b3, want
        if which == "a":
            a3n = a3.clone()
            a3n[z, i, kk] = float("nan")
            expect = want.copy()
            expect[z, i, :] = np.nan
        elif which == "b":
            b3n = b3.clone()
            b3n[z, kk, j] = float("nan")
            expect = want.copy()
            expect[z, :, j] = np.nan
        a, b = place_ab(be, layout, a3n, b3n)
        assert gc.route(be.lib, layout, case, a.vec, b.vec) == kern
        c = Placed(be, nan_like(be, case))
        gemm(be, layout, case, 1.0, a, b, 0.0, c)
        np.testing.assert_array_equal(c.host(), expect, err_msg=which)  # (NaN where expected, and nowhere else)


# ---------------------------------------------------------------- stale LDS
@pytest.mark.parametrize("entry", [e for e in EDGE_ENTRIES if e[0] != gc.SMALL], ids=gc.entry_id)
def test_gemm_ignores_stale_lds(be, entry):
    """Every CU's LDS full of NaN before the product, k with a partial last k-tile: what a kernel multiplies out of
    LDS it has to have written itself."""
    kern, case, layout = entry
    a3, b3, c03 = on_device(be, "exact", case)
    a, b = place_ab(be, layout, a3, b3)
    assert gc.route(be.lib, layout, case, a.vec, b.vec) == kern
    for alpha, beta in gc.ALPHA_BETA:
        c = Placed(be, nan_like(be, case) if beta == 0.0 else c03)
        be.debug_fill_lds(float("nan"))
        gemm(be, layout, case, alpha, a, b, beta, c)
        np.testing.assert_array_equal(c.host(), gc.exact_reference(case, alpha, beta))


# ---------------------------------------------------------------- rounding
ROUND_CASE = dict(EDGE_CASE)
ROUND_CASE[gc.SMALL] = Case(148, 148, 148, 1)
WORST = {}


@pytest.mark.parametrize("entry", [(kern, case, lay) for kern, case in ROUND_CASE.items() for lay in gc.LAYOUTS_OF[kern]],
                         ids=gc.entry_id)
def test_gemm_rounding_bound(be, entry):
    """Real-valued operands over twelve orders of magnitude with cancelling signs: every entry within
    (k + 4) eps (|alpha| |op(A)| |op(B)| + |beta C0|) of the extended-precision reference (gemm_cases: derived)."""
    kern, case, layout = entry
    assert case in gc.TABLE[kern]
    _, _, _, ref, bound = gc.real_operands(case)
    a3, b3, c03 = on_device(be, "real", case)
    a, b = place_ab(be, layout, a3, b3)
    assert gc.route(be.lib, layout, case, a.vec, b.vec) == kern
    c = Placed(be, c03)
    alpha, beta = gc.REAL_ALPHA_BETA
    gemm(be, layout, case, alpha, a, b, beta, c)
    ratio = gc.worst_ratio(c.host(), ref, bound)
    WORST[kern] = max(WORST.get(kern, 0.0), ratio)
    print(f"{gc.entry_id(entry)}: worst |got - ref| / bound = {ratio:.3e} (kernel so far {WORST[kern]:.3e})")
    assert ratio <= 1.0


# ---------------------------------------------------------------- kernel independence
@pytest.mark.parametrize("layout", gc.LAYOUTS)
def test_gemm_small_and_tiled_kernels_agree_bitwise(be, layout):
    """gemm_small_kernel takes k in the order of gemm_f64_kernel (its comment in gemm.hip), so the two give the same
    bits for real-valued operands too: the 352 rows that (352, 368, k) on the small kernel shares with (353, 368, k)
    on the 32 x 32 kernel, and k = 4096 on the small kernel against k = 4097 with a zero last row of op(B) on the
    32 x 32 kernel -- one row, or one k, past the small kernel's limits."""
    rng = np.random.default_rng(77)
    alpha, beta = gc.REAL_ALPHA_BETA

    def product(case, a3, b3, c03):
        a, b = place_ab(be, layout, be.asarray(a3), be.asarray(b3))
        c = Placed(be, be.asarray(c03))
        gemm(be, layout, case, alpha, a, b, beta, c)
        return gc.route(be.lib, layout, case, a.vec, b.vec), c.host()

    k = 37
    a3, b3, c03 = gc.real_entries(rng, (1, 353, k)), gc.real_entries(rng, (1, k, 368)), gc.real_entries(rng, (1, 353, 368))
    r_small, c_small = product(Case(352, 368, k, 1), a3[:, :352], b3, c03[:, :352])
    r_tiled, c_tiled = product(Case(353, 368, k, 1), a3, b3, c03)
    assert (r_small, r_tiled) == (gc.SMALL, gc.T32)
    assert same_bits(c_small, c_tiled[:, :352])

    a3, b3, c03 = gc.real_entries(rng, (1, 16, 4097)), gc.real_entries(rng, (1, 4097, 16)), gc.real_entries(rng, (1, 16, 16))
    b3[:, 4096] = 0.0
    r_small, c_small = product(Case(16, 16, 4096, 1), a3[:, :, :4096], b3[:, :4096], c03)
    r_tiled, c_tiled = product(Case(16, 16, 4097, 1), a3, b3, c03)
    assert (r_small, r_tiled) == (gc.SMALL, gc.T32)
    assert same_bits(c_small, c_tiled)
