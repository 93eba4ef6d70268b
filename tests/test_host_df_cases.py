"""CPU checks of tests/df_cases.py: every table entry reaches the GEMM kernels it names by the library's own routing
function (nbx_gemm_route, host arithmetic only), the table covers every (product, kernel, beta) the benchmark's
N = 2000 build uses, the float64 references are what exact arithmetic gives, every defect the exact comparison is there
to catch changes a result (and the symmetric-B control does not), and the rounding bounds of the real-valued cases are
ones a correct float64 evaluation meets."""

from fractions import Fraction

import numpy as np
import pytest

import df_cases as dc
import gemm_cases as gc
from nbed_amd import _nbx

HOST_MAX_N = 400  # the mutations and the graded identity run up to here; N = 904 is routed, generated and bounded only


@pytest.fixture(scope="module")
def lib():
    return _nbx.load_library()


def _names(routes):
    return [[gc.KERNEL_NAMES.get(k) for k in slab] for slab in routes]


# ------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_table_entry_reaches_its_kernels(lib, case):
    """The slab walk of nbx_jk_df -- ls = min(64, naux - l0), k = ls * nocc_max, batches of ls and ndm -- asked of
    nbx_gemm_route with the alignment flags the library derives (N even)."""
    assert len(case.routes) == -(-case.naux // dc.LS)
    assert _names(dc.library_routes(lib, case.n, case.naux, case.nocc)) == _names(case.routes)


def test_table_covers_the_benchmarks_kernels(lib):
    """N = 2000, n_occ = (512, 512), slabs of 64: all three products run on the LDS-DMA kernel, K with beta = 0 and then
    beta = 1 -- and the table has an entry for each (product, kernel, beta) of it.  A retuned threshold that moves
    the table off the benchmark's kernel fails here."""
    n, nocc = dc.BENCH_SHAPE
    routes = dc.library_routes(lib, n, 2 * dc.LS, nocc)
    assert routes == ((gc.TN_DMA,) * 3,) * 2, _names(routes)
    assert dc.library_routes(lib, n, 4000, nocc) == ((gc.TN_DMA,) * 3,) * (-(-4000 // dc.LS))  # (bench.py's --df-naux default)
    want = dc.used_kernels(n, 2 * dc.LS, nocc, routes)
    assert want == {("yt", gc.TN_DMA, 0.0), ("k", gc.TN_DMA, 0.0), ("k", gc.TN_DMA, 1.0)}
    have = {}
    for case in dc.CASES:
        for key in dc.used_kernels(case.n, case.naux, case.nocc, dc.library_routes(lib, case.n, case.naux, case.nocc)):
            have.setdefault(key, []).append(dc.case_id(case))
    for key in sorted(want):
        print(key[0], gc.KERNEL_NAMES[key[1]], f"beta={key[2]:g}:", have.get(key))
        assert key in have, key
    # the accumulation of another kernel's slab onto the LDS-DMA kernel's K, and both Yt kernels side by side in a slab
    assert ("k", gc.T64, 1.0) in dc.used_kernels(904, 129, (32, 31), dc.by_shape(904, 129, (32, 31)).routes)
    assert dc.by_shape(400, 65, (130, 66)).routes[0][:2] == (gc.TN_DMA, gc.T64)


def test_table_has_the_edges_of_the_slab_structure():
    """Slab counts of exactly 64, 64 + 1 and 2 * 64 + 1; nocc at 32 / 33 (the tile of df_transpose_occ_kernel) and
    nocc = N; N = 1 and N = 2; odd sizes; one density; an empty spin."""
    shapes = {(c.n, c.naux, c.nocc) for c in dc.CASES}
    assert {c.naux for c in dc.CASES} >= {dc.LS, dc.LS + 1, 2 * dc.LS + 1}
    assert {v for c in dc.CASES for v in c.nocc} >= {0, 1, 32, 33}
    assert any(c.n in c.nocc for c in dc.CASES if c.n > 32)
    assert {1, 2} <= {c.n for c in dc.CASES}
    assert sum(c.n % 2 for c in dc.CASES) >= 4 and any(c.n % 2 and c.naux % 2 and c.naux > dc.LS for c in dc.CASES)
    assert any(len(c.nocc) == 1 for c in dc.CASES)
    assert {(148, 70, (70, 66)), (150, 130, (75, 0))} <= shapes  # (what tests/test_gpu_kernels.py runs to a tolerance)
    assert len(shapes) == len(dc.CASES)


# ------------------------------------------------------------------------------------------ references
def _as_objects(x, conv):
    return np.vectorize(conv, otypes=[object])(x)


def _object_reference(b, c, nocc):
    """The formulas of jk_df_reference on object arrays (Python integers or Fractions: no rounding anywhere)."""
    n, ndm = b.shape[-1], len(nocc)
    out = [np.zeros((n, n), dtype=object) for _ in range(1 + ndm)]
    for bl in b:
        rho = 0
        for x in range(ndm):
            co = c[x][:, :nocc[x]]
            yt = np.matmul(co.T, bl)
            out[1 + x] = out[1 + x] + np.matmul(yt.T, yt)
            rho = rho + (yt * co.T).sum()
        out[0] = out[0] + ((2 if ndm == 1 else 1) * rho) * bl
    return np.stack(out)


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.n <= 19], ids=dc.case_id)
def test_exact_references_equal_exact_arithmetic(case):
    """Plain: Python integers.  Graded: Fractions of the graded operands -- and both the jk_df and the jk_factor form."""
    ops = dc.exact_operands(case)
    assert all(np.array_equal(x, np.rint(x)) for x in (ops.b, ops.c))
    assert set(np.unique(np.abs(ops.b))) <= {1.0, 3.0} and set(np.unique(np.abs(ops.c))) <= {1.0, 2.0}
    truth = _object_reference(_as_objects(ops.b, int), _as_objects(ops.c, int), case.nocc)
    ref = dc.exact_reference(case, "plain")
    assert ref.dtype == np.float64 and np.array_equal(_as_objects(ref, int), truth)
    gops = dc.graded(ops)
    gtruth = _object_reference(_as_objects(gops.b, Fraction), _as_objects(gops.c, Fraction), case.nocc)
    gref = dc.exact_reference(case, "graded")
    assert np.array_equal(_as_objects(gref, Fraction), gtruth)
    for o, r in ((ops, ref), (gops, gref)):
        dm = dc.densities(o.c, case.nocc)
        dc.assert_exact(dc.jk_factor_reference(o.b, dm), dc.factor_from_df(r, len(case.nocc)), "jk_factor form")
        if len(case.nocc) == 1:
            dc.assert_exact(dc.jk_factor_reference(o.b, dm[0]), dc.factor_from_df(r, 1), "jk_factor form, 2-D density")


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.n <= HOST_MAX_N], ids=dc.case_id)
def test_graded_reference_is_the_plain_one_scaled_element_by_element(case):
    ops = dc.exact_operands(case)
    assert case.n < 3 or ops.e.max() - ops.e.min() >= 8  # (the inputs do span many binades)
    dc.assert_exact(dc.exact_reference(case, "graded"), dc.exact_reference(case, "plain") * dc.grade(ops.e), "graded")
    dm, gdm = dc.densities(ops.c, case.nocc), dc.densities(dc.graded(ops).c, case.nocc)
    dc.assert_exact(gdm, dm / dc.grade(ops.e), "graded densities")


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_headroom_is_below_2_to_52(case):
    ops = dc.exact_operands(case)
    assert ops.b.shape == (case.naux, case.n, case.n) and ops.c.shape == (len(case.nocc), case.n, case.n)
    assert np.array_equal(ops.b, ops.b.transpose(0, 2, 1))
    assert len(case.nocc) == 1 or case.n < 3 or not np.array_equal(ops.c[0], ops.c[1])
    h = dc.headroom(ops.b, ops.c, case.nocc)
    print(f"{dc.case_id(case)}: headroom 2^{np.log2(h):.1f}")
    assert h < 2.0 ** 52
    assert np.abs(dc.exact_reference(case, "plain")).max() <= h


# ------------------------------------------------------------------------------------------ mutations
def _named(pred):
    return [c for c in dc.CASES if c.n <= HOST_MAX_N and pred(c)]


MUTATION_CASES = {
    "drop_short_slab": _named(lambda c: c.naux > dc.LS and c.naux % dc.LS),
    "beta0_second_slab": _named(lambda c: c.naux > dc.LS),
    "stale_rho": _named(lambda c: c.naux > dc.LS),
    "stale_rows": _named(lambda c: len(c.nocc) == 2 and c.nocc[1] < c.nocc[0]),
    "swap_spins": _named(lambda c: len(c.nocc) == 2),
    "no_factor2": _named(lambda c: len(c.nocc) == 1),
    "skip_odd_tail": _named(lambda c: c.n % 2 == 1),
}


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.n <= HOST_MAX_N], ids=dc.case_id)
def test_slab_algorithm_and_its_mutations(case):
    """The numpy restatement of nbx_jk_df's slab walk equals the reference in every bit; every mutation changes the
    result on each case named for it, on the plain and on the graded operands; B_L used transposed -- it is
    symmetric -- changes nothing (the control: the comparison does not fail for whatever is done to the walk)."""
    for variant in ("plain", "graded"):
        ops, ref = dc.operands(case, variant), dc.exact_reference(case, variant)
        dc.assert_exact(dc.slab_algorithm(ops.b, ops.c, case.nocc), ref, f"slab walk, {variant}")
        dc.assert_exact(dc.slab_algorithm(ops.b, ops.c, case.nocc, "transposed_b"), ref, f"control, {variant}")
        for mutation, cases in MUTATION_CASES.items():
            if case in cases:
                assert dc.differs(dc.slab_algorithm(ops.b, ops.c, case.nocc, mutation), ref), (mutation, variant)


def test_every_mutation_has_cases():
    assert set(MUTATION_CASES) | {"transposed_b"} == set(dc.MUTATIONS)
    for mutation, cases in MUTATION_CASES.items():
        assert len(cases) >= 2, mutation
    assert {dc.case_id(c) for c in MUTATION_CASES["skip_odd_tail"]} >= {"N1-L1-occ1", "N19-L5-occ5x4", "N97-L129-occ32x33"}
    assert dc.by_shape(150, 130, (75, 0)) in MUTATION_CASES["stale_rows"]  # (an empty spin must not inherit alpha's rows)


# ------------------------------------------------------------------------------------------ bounds
def _ld_fraction(v):
    """A longdouble as a Fraction (hi + lo, both float64, exactly enough)."""
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - dc.LD(hi)))


def test_real_reference_stays_inside_the_bound_against_fractions():
    """Fraction arithmetic on the float64 operands is the truth: the longdouble references are far inside the bounds and
    a plain float64 evaluation is inside them."""
    case = dc.by_shape(19, 5, (5, 4))
    rc = dc.real_case(case)
    fb, fc, fd = _as_objects(rc.b, Fraction), _as_objects(rc.c, Fraction), _as_objects(rc.dm, Fraction)
    truth_df = _object_reference(fb, fc, case.nocc)
    truth_f = [sum((fb[l] * fd.sum(axis=0)).sum() * fb[l] for l in range(case.naux))]
    truth_f += [sum(np.matmul(np.matmul(fb[l], fd[x]), fb[l]) for l in range(case.naux)) for x in range(2)]
    plain_df = dc.slab_algorithm(rc.b, rc.c, case.nocc)
    plain_f = dc.jk_factor_reference(rc.b, rc.dm)
    for what, truth, ref, bound, plain in (("jk_df", truth_df, rc.df_ref, rc.df_bound, plain_df),
                                           ("jk_factor", np.stack(truth_f), rc.factor_ref, rc.factor_bound, plain_f)):
        worst_ref = worst_plain = 0.0
        for ix in np.ndindex(ref.shape):
            bd = Fraction(float(bound[ix]))
            worst_ref = max(worst_ref, float(abs(_ld_fraction(ref[ix]) - truth[ix]) / bd))
            worst_plain = max(worst_plain, float(abs(Fraction(float(plain[ix])) - truth[ix]) / bd))
        print(f"{what}: reference / bound {worst_ref:.2e}, float64 numpy / bound {worst_plain:.2e}")
        assert worst_ref < 0.01  # (u of a longdouble is 2^-64: 2^-11 of the float64 bound)
        assert worst_plain <= 1.0


@pytest.mark.parametrize("case", dc.REAL_CASES, ids=dc.case_id)
def test_float64_numpy_meets_the_real_input_bounds(case):
    """The bounds are ones a correct float64 evaluation meets: numpy's, in the slab order of the kernels and in the
    order of the reference, against the longdouble reference."""
    rc = dc.real_case(case)
    assert rc.df_ref.dtype == dc.LD and np.finfo(dc.LD).eps < 2e-19
    for x, nocc in enumerate(case.nocc):  # orthonormal occupied orbitals
        co = rc.c[x][:, :nocc]
        assert nocc == 0 or np.abs(co.T @ co - np.eye(nocc)).max() < 1e-13
    ratios = {
        "jk_df, slab order": dc.worst_ratio(dc.slab_algorithm(rc.b, rc.c, case.nocc), rc.df_ref, rc.df_bound),
        "jk_df, reference order": dc.worst_ratio(dc.jk_df_reference(rc.b, rc.c, case.nocc), rc.df_ref, rc.df_bound),
        "jk_factor": dc.worst_ratio(dc.jk_factor_reference(rc.b, rc.dm), rc.factor_ref, rc.factor_bound),
    }
    print(dc.case_id(case), {k: f"{v:.2e}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0
    # the two entry points compute the same J and K: their references agree to the rounding of the float64 densities
    ndm = len(case.nocc)
    same = dc.factor_from_df(np.array(rc.df_ref), ndm)
    scale = float(np.abs(same).max())
    assert float(np.abs(same - rc.factor_ref).max()) <= 1e-12 * max(scale, 1e-300)
