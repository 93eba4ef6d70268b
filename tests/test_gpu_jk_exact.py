"""J/K and the AO->MO transform on EVERY element, bit for bit, at every kernel instance (MI355X).

The two-electron tensor is given in factorised form with small integer factors (tests/jk_cases.py): the J/K
contraction, the Fock epilogue and the four quarter transforms then hold exactly in float64 whatever the order of
summation, and the references cost O(L N^3) on the host -- all N^2 elements of J, K and F at N = 400 as easily as at
N = 24, every n^4 element of a transform.  Every comparison is array equality.  Before a result is compared,
nbx_jk_packed_route has to name the kernel and the instance the case is there for.  Outputs and workspaces hold NaN
before every call (the backend's poison knob)."""

import numpy as np
import pytest

import _jk_exact_worker as worker
import jk_cases as jc
from _jk_exact_worker import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    be = worker.fresh_backend()
    yield be
    worker.free_device(be)


# ------------------------------------------------------------------------------------------ packed J/K
@pytest.mark.parametrize("case", jc.PACKED_CASES, ids=jc.packed_id)
def test_packed_instance_is_exact(be, case):
    """Two densities, one density, the Fock epilogue without and with the Dtot' table of the scalars kernel, and row
    slabs packed on their own (three of equal triangular work; from N = 320 the slabs the dense tensor is built in):
    all N^2 elements of J, K[0], K[1], F and vhf, J and K exactly symmetric, every slab its own reference."""
    worker.run_packed_case(be, case)


PACKED_BY_N = {c.n: c for c in jc.PACKED_CASES}


@pytest.mark.parametrize("family", list(jc.FAMILY_CASES), ids=str)
def test_packed_family_graded_operands_and_stale_lds(be, family):
    """One instance per kernel family on the graded variant (inputs spanning 2^96, every output element still exact: a
    kernel that screens, truncates or orders by magnitude fails), and on the plain one with every CU's LDS holding NaN
    before each launch."""
    case = PACKED_BY_N[jc.FAMILY_CASES[family]]
    worker.run_packed_case(be, case, ops=jc.graded(jc.operands(case.n)))
    worker.run_packed_case(be, case, lds_nan=True)


def test_switch_selected_fallbacks_are_exact(be):
    """The kernels the shipped library keeps behind NBX_JK_M8=0 (csrc/jk_m4.hip for 97 .. 148), NBX_JK_M8=0 NBX_JK_M4=0
    and NBX_JK_MX=0 (csrc/jk_s4.hip up to 256, its NB = 4 / 17-loads instance included): the switches are read once
    per process, so a child process per setting (tests/_jk_exact_worker.py), one after the other, each with its own time
    limit; an abnormal exit ends the test before the next child starts.  The route is asserted inside the child."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    worker.free_device(be)
    root = Path(__file__).resolve().parent.parent
    for setting, cases in jc.SWITCH_CASES.items():
        env = dict(os.environ, PYTHONPATH=str(root))
        for name in ("NBX_JK_M8", "NBX_JK_M4", "NBX_JK_MX"):
            env.pop(name, None)
        env.update(item.split("=") for item in setting.split())
        r = subprocess.run([sys.executable, str(root / "tests" / "_jk_exact_worker.py"), setting], env=env,
                           capture_output=True, text=True, timeout=420)
        assert r.returncode == 0 and f"JKX OK {setting}" in r.stdout, f"{setting}:\n" + r.stdout[-3000:] + r.stderr[-3000:]
        assert r.stdout.count(": exact (") == len(cases), r.stdout[-3000:]


# ------------------------------------------------------------------------------------------ dense J/K
def _dense_check(be, case, ops, lds_nan=False):
    n = case.n
    b_dev, dm = dev(be, ops.b), dev(be, ops.dm)
    dm1 = dm[1].clone()
    ref = jc.jk_reference(ops.b, ops.dm)
    ref1 = jc.jk_reference(ops.b, ops.dm[1])
    tag = f"jk.hip N={n}"

    def run(eri, d, p0, p1):
        if lds_nan:
            be.debug_fill_lds(float("nan"))
        return be.to_host(be.jk(eri, d, p0, p1))

    if case.rows is None:
        eri = jc.device_rows(be.torch, b_dev, 0, n)
        whole, whole1 = run(eri, dm, 0, n), run(eri, dm1, 0, n)
        jc.assert_exact(whole, ref, tag + " two densities")
        jc.assert_exact(whole1, ref1, tag + " one density")
        worker.check_symmetric(whole, tag)
        del eri
        slabs = [s for s in ((0, 1), (n // 3, n // 3 + 2), (n - 1, n)) if 0 <= s[0] < s[1] <= n]
    else:
        whole, whole1 = ref, ref1
        slabs = [case.rows]
    for p0, p1 in slabs:  # (a slab is an allocation of its own: its rows start 16-byte aligned at any N)
        eri = jc.device_rows(be.torch, b_dev, p0, p1)
        jc.assert_exact(run(eri, dm, p0, p1), whole[:, p0:p1], f"{tag} rows [{p0}, {p1}) two densities")
        jc.assert_exact(run(eri, dm1, p0, p1), whole1[:, p0:p1], f"{tag} rows [{p0}, {p1}) one density")
        del eri


@pytest.mark.parametrize("case", jc.DENSE_CASES, ids=lambda c: f"N{c.n}-CS{c.cs}-{'vec2' if c.vec2 else 'scalar'}")
def test_dense_kernel_is_exact(be, case):
    """nbx_jk_dense (csrc/jk.hip), every (NDM, CS, VEC2) instance: the whole tensor where it fits, and row slabs that are
    bit-equal to the rows of the whole (sizes past 256: a row slab against the reference)."""
    assert jc.dense_class(case.n) == (case.cs, case.vec2)
    worker.free_device(be)
    _dense_check(be, case, jc.operands(case.n))


def _sym_slab_reference(ops, dm, p0, p1, qb):
    if qb:
        return jc.slab_reference(ops.b, dm, p0, p1, "lower")
    rows = jc.slab_reference(ops.b, dm, p0, p1, "rows")  # (odd N: nbx_jk_dense's rows scattered into full-size matrices)
    full = np.zeros((rows.shape[0], ops.b.shape[-1], ops.b.shape[-1]))
    full[:, p0:p1] = rows
    return full


def _sym_check(be, case, ops, lds_nan=False):
    n = case.n
    b_dev, dm = dev(be, ops.b), dev(be, ops.dm)
    dm1 = dm[1].clone()
    tag = f"jk_sym.hip N={n}"

    def run(eri, d, p0, p1):
        if lds_nan:
            be.debug_fill_lds(float("nan"))
        return be.to_host(be.jk_sym(eri, d, p0, p1))

    if case.rows is None:
        eri = jc.device_rows(be.torch, b_dev, 0, n)
        for d, dh, what in ((dm, ops.dm, " two densities"), (dm1, ops.dm[1], " one density")):
            got = run(eri, d, 0, n)
            jc.assert_exact(got, jc.jk_reference(ops.b, dh), tag + what)
            worker.check_symmetric(got, tag + what)
        del eri
        slabs = jc.equal_work_cuts(n)
    else:
        slabs = [case.rows]
    acc = 0.0
    for p0, p1 in slabs:
        eri = jc.device_rows(be.torch, b_dev, p0, p1)
        part = run(eri, dm, p0, p1)
        jc.assert_exact(part, _sym_slab_reference(ops, ops.dm, p0, p1, case.qb), f"{tag} slab [{p0}, {p1}) two densities")
        jc.assert_exact(run(eri, dm1, p0, p1), _sym_slab_reference(ops, ops.dm[1], p0, p1, case.qb),
                        f"{tag} slab [{p0}, {p1}) one density")
        acc = acc + part
        del eri
    if case.rows is None:
        jc.assert_exact(acc, jc.jk_reference(ops.b, ops.dm), tag + " sum of the slabs")


@pytest.mark.parametrize("case", jc.SYM_CASES, ids=lambda c: f"N{c.n}-QB{c.qb}")
def test_dense_sym_kernel_is_exact(be, case):
    """nbx_jk_dense_sym (csrc/jk_sym.hip): QB = 2 and 4 on either side of N = 192, the largest N / 2 it has threads for,
    and an odd size (the fallback through nbx_jk_dense) -- the whole tensor and additive row slabs."""
    assert jc.sym_qb(case.n) == case.qb
    worker.free_device(be)
    _sym_check(be, case, jc.operands(case.n))


@pytest.mark.parametrize("n", [24, 194, 37])
def test_dense_sym_fock_is_exact(be, n):
    """nbx_jk_dense_sym_fock (the Fock epilogue in the symmetric kernel's reduction; odd N: the two-call fallback) through
    the path that reaches it: nbx_mu_cycle_fock on a state that holds the dense tensor."""
    worker.free_device(be)
    ops = jc.operands(n)
    b_dev, dm, hv = dev(be, ops.b), dev(be, ops.dm), dev(be, ops.hv)
    eri = jc.device_rows(be.torch, b_dev, 0, n)
    eye = dev(be, np.stack([np.eye(n), np.eye(n)]))
    state = be.mu_cycle_state(n, (n // 2, n // 2), None, hv, eye, eye, eri=eri)
    out = state.sets[0]
    be.mu_cycle_fock(state, dm, out).get()
    fock_ref, vhf_ref = jc.fock_reference(ops.b, ops.dm, ops.hv)
    jc.assert_exact(be.to_host(out["fock"]), fock_ref, f"dense-sym fock N={n}")
    jc.assert_exact(be.to_host(out["vhf"]), vhf_ref, f"dense-sym vhf N={n}")
    jc.assert_exact(be.to_host(state.jk), jc.jk_reference(ops.b, ops.dm), f"dense-sym J/K of the cycle N={n}")


@pytest.mark.parametrize("kind", ["dense", "dense-sym"])
def test_dense_family_graded_operands_and_stale_lds(be, kind):
    worker.free_device(be)
    if kind == "dense":
        for case in (jc.DENSE_CASES[1], jc.DENSE_CASES[3]):
            _dense_check(be, case, jc.graded(jc.operands(case.n)))
            _dense_check(be, case, jc.operands(case.n), lds_nan=True)
    else:
        for case in (jc.SYM_CASES[0], jc.SYM_CASES[2]):
            _sym_check(be, case, jc.graded(jc.operands(case.n)))
            _sym_check(be, case, jc.operands(case.n), lds_nan=True)


# ------------------------------------------------------------------------------------------ ao2mo
def _assert_transform(be, got, m_fac, n_fac, what, i0=0):
    """got (rows, n2, n3, n4) == sum_L M_L[i0 + i, j] N_L[k, l] on every element: the outer products are formed on the
    device a chunk of i at a time; the offending rows come to the host for the message."""
    torch = be.torch
    rows = got.shape[0]
    step = max(1, (1 << 27) // max(1, got[0].numel()))
    for a in range(0, rows, step):
        z = min(a + step, rows)
        ref = torch.zeros_like(got[a:z])
        for ml, nl in zip(m_fac, n_fac):
            ref.addcmul_(ml[i0 + a:i0 + z, :, None, None], nl[None, None, :, :])
        if not torch.equal(got[a:z], ref):
            bad = (got[a:z] != ref).flatten(1).any(dim=1).nonzero().flatten()[:2] + a
            for i in bad.tolist():
                jc.assert_exact(be.to_host(got[i]), be.to_host(ref[i - a]), f"{what}, outer index {i0 + i}")
            raise AssertionError(what)  # (NaN in both places)


@pytest.mark.parametrize("case", jc.AO2MO_CASES, ids=lambda c: f"N{c.n}-{c.n1}x{c.n2}x{c.n3}x{c.n4}")
def test_ao2mo_entry_points_are_exact(be, case):
    """nbx_ao2mo, nbx_ao2mo_pair (whole and an outer-index slab), nbx_ao2mo_pair_sym dense and rs-packed with one and two
    outputs, nbx_eri_pack_rs: all n^4 elements against sum_L M_L (x) N_L with the (L, n, n) factors from the host; the
    pair-symmetric outputs exactly symmetric in (i, j)."""
    worker.free_device(be)
    n = case.n
    torch = be.torch
    ops = jc.operands(n)
    cs = jc.ao2mo_coefficients(case)
    c1, c2, c3, c4, c5, c6 = (dev(be, c) for c in cs)
    b_dev = dev(be, ops.b)
    eri = jc.device_rows(torch, b_dev, 0, n)
    m12 = dev(be, jc.ao2mo_factors(ops.b, cs[0], cs[1]))
    m11 = dev(be, jc.ao2mo_factors(ops.b, cs[0], cs[0]))
    n34 = dev(be, jc.ao2mo_factors(ops.b, cs[2], cs[3]))
    n56 = dev(be, jc.ao2mo_factors(ops.b, cs[4], cs[5]))
    tag = f"N={n}"
    i0, i1 = case.n1 // 3, min(case.n1, case.n1 // 3 + 5)

    _assert_transform(be, be.ao2mo(eri, c1, c2, c3, c4), m12, n34, tag + " ao2mo")
    _assert_transform(be, be.ao2mo(eri, c1, c2, c3, c4, i0=i0, i1=i1), m12, n34, tag + " ao2mo outer slab", i0)
    o1, o2 = be.ao2mo_pair(eri, c1, c2, c3, c4, c5, c6)
    _assert_transform(be, o1, m12, n34, tag + " ao2mo_pair first")
    _assert_transform(be, o2, m12, n56, tag + " ao2mo_pair second")
    o1, o2 = be.ao2mo_pair(eri, c1, c2, c3, c4, c5, c6, i0=i0, i1=i1)
    _assert_transform(be, o1, m12, n34, tag + " ao2mo_pair outer slab first", i0)
    _assert_transform(be, o2, m12, n56, tag + " ao2mo_pair outer slab second", i0)
    del o1, o2

    # nbx_eri_pack_rs against the host's packing: the (r, s <= r) index lists come from numpy
    r_idx, s_idx = np.tril_indices(n)
    eri_rs = be.eri_pack_rs(eri, n)
    ri, si = torch.as_tensor(r_idx, device=be.device), torch.as_tensor(s_idx, device=be.device)
    want = torch.zeros_like(eri_rs)
    for bl in b_dev:
        want.addcmul_(bl[:, :, None], bl[ri, si][None, None, :])
    assert torch.equal(eri_rs, want), tag + " eri_pack_rs"
    del want
    if n <= 40:
        jc.assert_exact(be.to_host(eri_rs), jc.pack_rs(jc.dense_tensor(ops.b)), tag + " eri_pack_rs against the host's packing")

    for src, packed, name in ((eri, False, "pair_sym"), (eri_rs, True, "pair_sym rs-packed")):
        one = be.ao2mo_pair_sym(src, c1, c3, c4, rs_packed=packed)
        _assert_transform(be, one, m11, n34, f"{tag} {name}, one output")
        assert torch.equal(one, one.transpose(0, 1)), f"{tag} {name}: (ij|kl) = (ji|kl)"
        del one
        o1, o2 = be.ao2mo_pair_sym(src, c1, c3, c4, c5, c6, rs_packed=packed)
        _assert_transform(be, o1, m11, n34, f"{tag} {name}, first of two")
        _assert_transform(be, o2, m11, n56, f"{tag} {name}, second of two")
        assert torch.equal(o1, o1.transpose(0, 1)) and torch.equal(o2, o2.transpose(0, 1)), f"{tag} {name}: (ij|kl) = (ji|kl)"
        del o1, o2
