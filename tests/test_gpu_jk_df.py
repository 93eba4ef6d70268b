"""The factorised J/K -- nbx_jk_df (nbed_amd/csrc/jk_df.hip) and HipBackend.jk_factor -- on EVERY element, bit for bit,
on the GEMM kernels the benchmark's N = 2000 build runs on (MI355X).

tests/df_cases.py has the inputs: integer factors and orbitals whose J and K float64 holds exactly whatever the order
of summation, a graded variant spanning 2^48, and real-valued ones with a derived per-element rounding bound against
a longdouble reference.  Before a result is compared, nbx_gemm_route has to name the kernels the case is there for.
Beyond the table: slabs of the auxiliary index add exactly, jk_factor's chunk loop, a workspace reused after a larger
call, NaN-poisoned allocations, the refusals of the C entry points, and nbx_df_synth with a slab offset and past one
grid pass."""

import ctypes
import gc

import numpy as np
import pytest

import df_cases as dc
from nbed_amd import _nbx, synth

pytestmark = pytest.mark.gpu


def _backend():
    from nbed_amd.backend import HipBackend

    return HipBackend()


def free_device(be):
    import torch

    be.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def be():
    be = _backend()
    assert not be._poison  # (stale workspace contents are part of what is tested; the poisoned runs make their own)
    yield be
    free_device(be)


def dev(be, x):
    """Host array -> device (a copy first where the upload would alias it: the operand caches are read-only)."""
    return be.asarray(x if x.size >= (1 << 26) else np.array(x))


def density_of(ops_c, nocc):
    """What jk_factor is handed: (ndm, N, N), or the single (N, N) density when ndm = 1."""
    dm = dc.densities(ops_c, nocc)
    return dm[0] if len(nocc) == 1 else dm


def check_symmetric(jk, what):
    dc.assert_exact(jk, jk.transpose(0, 2, 1), what + ": J and K symmetric")


def assert_routes(be, case):
    got = dc.library_routes(be.lib, case.n, case.naux, case.nocc)
    assert got == case.routes, (dc.case_id(case), got)


# ------------------------------------------------------------------------------------------ exact, every element
@pytest.mark.parametrize("case,variant", [(c, v) for c in dc.CASES for v in ("plain", "graded")],
                         ids=lambda p: dc.case_id(p) if isinstance(p, dc.Case) else p)
def test_jk_df_and_jk_factor_are_exact(be, case, variant):
    """All N^2 elements of J and of every K, from the orbitals (nbx_jk_df) and from the densities (jk_factor; one density
    as a 2-D array, its J not doubled), equal to the float64 reference in every bit and exactly symmetric."""
    assert_routes(be, case)
    free_device(be)
    ops, ref = dc.operands(case, variant), dc.exact_reference(case, variant)
    tag = f"{dc.case_id(case)} {variant}"
    b_d, c_d = dev(be, ops.b), dev(be, ops.c)
    got = be.to_host(be.jk_df(b_d, c_d, case.nocc))
    dc.assert_exact(got, ref, tag + " jk_df")
    check_symmetric(got, tag + " jk_df")
    dm = density_of(ops.c, case.nocc)
    assert dm.ndim == (2 if len(case.nocc) == 1 else 3)
    got = be.to_host(be.jk_factor(b_d, dev(be, dm)))
    dc.assert_exact(got, dc.factor_from_df(ref, len(case.nocc)), tag + " jk_factor")
    check_symmetric(got, tag + " jk_factor")


@pytest.mark.parametrize("case,variant", [(dc.by_shape(97, 129, (32, 33)), "plain"), (dc.by_shape(97, 129, (32, 33)), "graded"),
                                          (dc.by_shape(148, 70, (70, 66)), "plain"), (dc.by_shape(150, 130, (75, 0)), "plain")],
                         ids=lambda p: dc.case_id(p) if isinstance(p, dc.Case) else p)
def test_slabs_of_the_auxiliary_index_add_exactly(be, case, variant):
    """jk_df(B[:cut]) + jk_df(B[cut:]) is the whole, bit for bit (the multi-rank split; at an odd N and an odd cut the
    second slab starts 8 bytes off a 16-byte boundary)."""
    ops, ref = dc.operands(case, variant), dc.exact_reference(case, variant)
    b_d, c_d = dev(be, ops.b), dev(be, ops.c)
    for cut in (1, 63, 64, 65):
        assert 0 < cut < case.naux
        parts = be.to_host(be.jk_df(b_d[:cut], c_d, case.nocc)) + be.to_host(be.jk_df(b_d[cut:], c_d, case.nocc))
        dc.assert_exact(parts, ref, f"{dc.case_id(case)} {variant} cut at {cut}")


@pytest.mark.parametrize("case", [dc.by_shape(24, 7, (6,)), dc.by_shape(148, 70, (70, 66))], ids=dc.case_id)
def test_factor_that_starts_eight_bytes_into_an_allocation(be, case):
    """An even N with B a view that is only 8-byte aligned: neither the GEMMs' nor df_j_kernel's 16-byte loads apply."""
    ops, ref = dc.operands(case, "plain"), dc.exact_reference(case, "plain")
    flat = be.empty((ops.b.size + 1,))
    flat[1:].copy_(dev(be, ops.b).reshape(-1))
    b_d = flat[1:].view(ops.b.shape)
    assert b_d.data_ptr() % 16 == 8 and b_d.is_contiguous()
    dc.assert_exact(be.to_host(be.jk_df(b_d, dev(be, ops.c), case.nocc)), ref, dc.case_id(case))


@pytest.mark.parametrize("case", [dc.by_shape(19, 5, (5, 4)), dc.by_shape(97, 129, (32, 33))], ids=dc.case_id)
def test_jk_factor_chunk_loop(be, case):
    """Chunks of three auxiliary functions (3 + 2 at naux = 5, 43 of three at 129): the beta = 1 branch of the K product,
    against the unchunked call and the reference."""
    n, ndm = case.n, len(case.nocc)
    assert case.naux > 3
    for variant in ("plain", "graded"):
        ops, ref = dc.operands(case, variant), dc.exact_reference(case, variant)
        b_d, dm_d = dev(be, ops.b), dev(be, density_of(ops.c, case.nocc))
        whole = be.to_host(be.jk_factor(b_d, dm_d))
        be.JK_FACTOR_CHUNK_DOUBLES = 3 * n * n
        try:
            chunked = be.to_host(be.jk_factor(b_d, dm_d))
        finally:
            del be.JK_FACTOR_CHUNK_DOUBLES
        assert be.JK_FACTOR_CHUNK_DOUBLES == type(be).JK_FACTOR_CHUNK_DOUBLES == 1 << 25
        dc.assert_exact(chunked, whole, f"{dc.case_id(case)} {variant}: chunked against unchunked")
        dc.assert_exact(chunked, dc.factor_from_df(ref, ndm), f"{dc.case_id(case)} {variant}: chunked")


# ------------------------------------------------------------------------------------------ real-valued inputs
WORST = {}


@pytest.mark.parametrize("case", dc.REAL_CASES, ids=dc.case_id)
def test_real_inputs_within_the_derived_bounds(be, case):
    """synth.df_factor and orthonormal orbitals: every element of J and K of both entry points within the a-priori
    bound of tests/df_cases.py of the longdouble reference."""
    rc = dc.real_case(case)
    b_d = dev(be, rc.b)
    got = be.to_host(be.jk_df(b_d, dev(be, rc.c), case.nocc))
    ratio_df = dc.worst_ratio(got, rc.df_ref, rc.df_bound)
    got = be.to_host(be.jk_factor(b_d, dev(be, rc.dm)))
    ratio_f = dc.worst_ratio(got, rc.factor_ref, rc.factor_bound)
    WORST[dc.case_id(case)] = (ratio_df, ratio_f)
    print(f"{dc.case_id(case)}: worst |got - ref| / bound: jk_df {ratio_df:.3e}, jk_factor {ratio_f:.3e}")
    assert ratio_df <= 1.0 and ratio_f <= 1.0


# ------------------------------------------------------------------------------------------ workspace, poison
def test_workspace_reuse_and_determinism(be):
    """A = (148, 70, (70, 66)), then B = (150, 130, (75, 0)) -- a larger nocc_max: the cached workspace grows -- then A
    again on what B left in it: both runs of A give the same bits, and those of a fresh backend; on the exact inputs
    they are the reference as well."""
    a, b = dc.by_shape(148, 70, (70, 66)), dc.by_shape(150, 130, (75, 0))
    for kind in ("real", "exact"):
        if kind == "real":
            (ab, ac), (bb, bc) = dc.real_operands(a), dc.real_operands(b)
        else:
            (ab, ac, _), (bb, bc, _) = dc.operands(a, "plain"), dc.operands(b, "plain")
        free_device(be)
        ab_d, ac_d = dev(be, ab), dev(be, ac)
        first = be.to_host(be.jk_df(ab_d, ac_d, a.nocc))
        small = be._work["jk_df"].numel()
        other = be.to_host(be.jk_df(dev(be, bb), dev(be, bc), b.nocc))
        assert be._work["jk_df"].numel() > small
        again = be.to_host(be.jk_df(ab_d, ac_d, a.nocc))
        dc.assert_exact(again, first, f"{kind}: A after B")
        fresh = _backend()
        dc.assert_exact(fresh.to_host(fresh.jk_df(dev(fresh, ab), dev(fresh, ac), a.nocc)), first, f"{kind}: fresh backend")
        del fresh
        if kind == "exact":
            dc.assert_exact(first, dc.exact_reference(a, "plain"), "A")
            dc.assert_exact(other, dc.exact_reference(b, "plain"), "B")


def test_poisoned_allocations(monkeypatch):
    """A backend created under NBED_POISON_EMPTY=1: outputs hold NaN and workspaces NaN bit patterns before every call,
    so whatever a kernel reads without having written it -- Yt rows past a spin's count, the tail of a short slab, the
    rows of an empty spin -- shows."""
    monkeypatch.setenv("NBED_POISON_EMPTY", "1")
    pbe = _backend()
    assert pbe._poison
    for shape in ((33, 65, (33, 1)), (97, 129, (32, 33)), (150, 130, (75, 0))):
        case = dc.by_shape(*shape)
        ops, ref = dc.operands(case, "plain"), dc.exact_reference(case, "plain")
        b_d = dev(pbe, ops.b)
        got = pbe.to_host(pbe.jk_df(b_d, dev(pbe, ops.c), case.nocc))
        assert not np.isnan(got).any()
        dc.assert_exact(got, ref, dc.case_id(case) + " poisoned jk_df")
        got = pbe.to_host(pbe.jk_factor(b_d, dev(pbe, density_of(ops.c, case.nocc))))
        assert not np.isnan(got).any()
        dc.assert_exact(got, dc.factor_from_df(ref, len(case.nocc)), dc.case_id(case) + " poisoned jk_factor")
    free_device(pbe)


# ------------------------------------------------------------------------------------------ the C entry points
def _provoke_other_error(be):
    """Leaves another entry point's message in nbx_last_error, so that the next refusal has to set its own."""
    assert be.lib.nbx_df_synth(be.ctx, 0, 0, 1, 1, 1.0, None) == _nbx.NBX_E_INVALID
    assert b"nbx_df_synth" in be.lib.nbx_last_error()


def test_c_abi_refusals_and_empty_inputs(be):
    torch = be.torch
    lib = be.lib
    case = dc.by_shape(24, 7, (6,))
    n, naux = case.n, case.naux
    ops = dc.operands(case, "plain")
    b_d = dev(be, ops.b)
    c_d = dev(be, np.stack([ops.c[0], ops.c[0][::-1]]))
    jk = torch.empty((3, n, n), dtype=torch.float64, device=be.device)
    nbytes = int(lib.nbx_jk_df_worksize(n, 2, 6))
    assert nbytes > 0 and nbytes % 256 == 0
    work = torch.empty(nbytes, dtype=torch.uint8, device=be.device)

    def call(nao=n, naux=naux, ndm=2, nocc=(6, 5), work_bytes=nbytes, null_nocc=False):
        jk.fill_(-3.0)
        counts = (ctypes.c_int64 * 2)(*nocc)
        rc = lib.nbx_jk_df(be.ctx, nao, naux, be._p(b_d), ndm, be._p(c_d), None if null_nocc else counts, be._p(jk), be._p(work),
                           work_bytes)
        be.synchronize()
        return rc, be.to_host(jk)

    for what, kwargs, code, word in (("ndm = 3", dict(ndm=3), _nbx.NBX_E_INVALID, b"invalid argument"),
                                     ("nocc > N", dict(nocc=(n + 1, 5)), _nbx.NBX_E_INVALID, b"invalid argument"),
                                     ("nocc > N, second spin", dict(nocc=(6, n + 1)), _nbx.NBX_E_INVALID, b"invalid argument"),
                                     ("naux < 0", dict(naux=-1), _nbx.NBX_E_INVALID, b"invalid argument"),
                                     ("null nocc", dict(null_nocc=True), _nbx.NBX_E_INVALID, b"invalid argument"),
                                     ("workspace one byte short", dict(work_bytes=nbytes - 1), _nbx.NBX_E_NOMEM, b"workspace")):
        _provoke_other_error(be)
        rc, out = call(**kwargs)
        assert rc == code, (what, rc)
        assert np.all(out == -3.0), what
        msg = lib.nbx_last_error()
        assert msg.startswith(b"nbx_jk_df") and word in msg, (what, msg)

    # the same arguments unrefused, then nothing to contract: zeros, not what the output held
    rc, out = call()
    assert rc == _nbx.NBX_OK
    c_h = be.to_host(c_d)
    dc.assert_exact(out, dc.jk_df_reference(ops.b, c_h, (6, 5)), "two spins through the C entry point")
    for what, kwargs in (("naux = 0", dict(naux=0)), ("all nocc = 0", dict(nocc=(0, 0)))):
        rc, out = call(**kwargs)
        assert rc == _nbx.NBX_OK, (what, rc)
        assert np.all(out == 0.0), what

    assert lib.nbx_jk_df_worksize(0, 2, 0) == 0 and lib.nbx_jk_df_worksize(-5, 1, 0) == 0
    assert lib.nbx_jk_df_worksize(n, 0, 1) == 0 and lib.nbx_jk_df_worksize(n, 3, 1) == 0
    assert lib.nbx_jk_df_worksize(n, 2, n + 1) == 0 and lib.nbx_jk_df_worksize(n, 2, n) > 0
    assert lib.nbx_jk_df_worksize(n, 2, 0) == lib.nbx_jk_df_worksize(n, 2, 1) > 0


# ------------------------------------------------------------------------------------------ nbx_df_synth
@pytest.mark.parametrize("n,l0,l1", [(19, 3, 8), (150, 64, 70), (1025, 2, 4)])
def test_df_synth_slab_offset_and_grid_stride(be, n, l0, l1):
    """A slab [l0, l1) generated on its own is that slab of the host generator's factor, bit for bit, every slice
    symmetric; at N = 1025 a slice has more elements than one pass of the 4096 x 256 grid."""
    if n == 1025:
        assert n * n > 4096 * 256
    want = synth.df_factor(n, 0, l1)[l0:]
    got = be.to_host(be.df_synth(n, l0, l1))
    dc.assert_exact(got, want, f"df_synth({n}, {l0}, {l1})")
    dc.assert_exact(got, got.transpose(0, 2, 1), "symmetric slices")
    dc.assert_exact(got, synth.df_factor(n, l0, l1), "the host generator's own slab")


def test_df_synth_refusals(be):
    torch = be.torch
    lib = be.lib
    buf = torch.full((4 * 4,), -3.0, dtype=torch.float64, device=be.device)
    for what, (nao, l0, l1) in (("l1 < l0", (4, 2, 1)), ("more than 65535 slices", (4, 0, 65536)),
                                ("nao >= 92681", (92681, 0, 1)), ("nao = 0", (0, 0, 1)), ("l0 < 0", (4, -1, 0))):
        # (another entry point's message first, so that the refusal has to set its own)
        assert lib.nbx_jk_df(be.ctx, 4, 0, None, 2, None, None, None, None, 0) == _nbx.NBX_E_INVALID
        assert lib.nbx_last_error().startswith(b"nbx_jk_df")
        rc = lib.nbx_df_synth(be.ctx, nao, l0, l1, synth.SEED, 1.0, be._p(buf))
        be.synchronize()
        assert rc == _nbx.NBX_E_INVALID, (what, rc)
        assert lib.nbx_last_error().startswith(b"nbx_df_synth"), what
        assert bool((buf == -3.0).all()), what
    assert lib.nbx_df_synth(be.ctx, 4, 1, 1, synth.SEED, 1.0, be._p(buf)) == _nbx.NBX_OK  # an empty slab: nothing written
    be.synchronize()
    assert bool((buf == -3.0).all())
    assert lib.nbx_df_synth(be.ctx, 4, 1, 2, synth.SEED, synth.df_scale(4), be._p(buf)) == _nbx.NBX_OK
    be.synchronize()
    dc.assert_exact(be.to_host(buf).reshape(1, 4, 4), synth.df_factor(4, 1, 2), "one slice through the C entry point")


def test_zz_worst_ratios():
    """The worst error / bound of the real-valued cases (run with -s to see them)."""
    for name, (ratio_df, ratio_f) in WORST.items():
        print(f"{name}: jk_df {ratio_df:.3e}  jk_factor {ratio_f:.3e}")
    assert all(max(v) <= 1.0 for v in WORST.values())
