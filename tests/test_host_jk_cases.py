"""CPU checks of tests/jk_cases.py: the factorised references are the einsum definitions and the C oracle, the operand
family is what its docstring claims (odd tensor, few coincidences under a wrong index order, sums far below 2^52), every
kernel instance the dispatch code can select is in the tables and reached by the library's own routing query
(nbx_jk_packed_route: the functions the launcher asks, host arithmetic only), and the comparison the GPU tests use fails
for every mutation of a numpy restatement of the tile walk."""

import numpy as np
import pytest

import jk_cases as jc
from nbed_amd import _nbx
from oracle import cref, hamiltonian
from oracle.pyscf_like import get_jk


@pytest.fixture(scope="module")
def lib():
    return _nbx.load_library()


def test_kernel_ids_mirror_the_header():
    header = (_nbx.LIB_PATH.parent.parent / "include" / "nbx.h").read_text()
    for kern, name in jc.KERNEL_NAMES.items():
        assert f"#define NBX_JK_KERNEL_{name} {kern} " in header, name
    assert (_nbx.JK_KERNEL_NONE, _nbx.JK_KERNEL_S4, _nbx.JK_KERNEL_M4, _nbx.JK_KERNEL_M8, _nbx.JK_KERNEL_MX,
            _nbx.JK_KERNEL_MX_HI) == (jc.NONE, jc.S4, jc.M4, jc.M8, jc.MX, jc.MX_HI)


# ------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("n", [5, 16, 24])
def test_factorised_jk_is_the_einsum_definition(n):
    for ops in (jc.operands(n), jc.graded(jc.operands(n))):
        eri = jc.dense_tensor(ops.b)
        j, k = get_jk(eri, ops.dm)
        ref = jc.jk_reference(ops.b, ops.dm)
        np.testing.assert_array_equal(ref[0], j[0] + j[1])
        np.testing.assert_array_equal(ref[1:], k)
        one = jc.jk_reference(ops.b, ops.dm[1])
        np.testing.assert_array_equal(one, np.stack([j[1], k[1]]))
        fock, vhf = jc.fock_reference(ops.b, ops.dm, ops.hv)
        np.testing.assert_array_equal(vhf, (j[0] + j[1])[None] - k)
        np.testing.assert_array_equal(fock, ops.hv + vhf)
    plain, g = jc.operands(n), jc.graded(jc.operands(n))
    # the graded variant: the same integers under one power of two per element
    np.testing.assert_array_equal(jc.jk_reference(g.b, g.dm), jc.jk_reference(plain.b, plain.dm) * jc.grade(plain.e))
    assert g.b.max() / np.abs(g.b[0]).min() >= 2.0 ** 40 or n < 16


@pytest.mark.parametrize("n", [6, 24])
def test_slab_references_are_the_masked_einsum_and_add_up(n):
    ops = jc.operands(n)
    eri = jc.dense_tensor(ops.b)
    idx = np.arange(n)
    a, b, c, d = np.meshgrid(idx, idx, idx, idx, indexing="ij")
    whole = jc.jk_reference(ops.b, ops.dm)
    cuts = jc.equal_work_cuts(n)
    assert cuts[0][0] == 0 and cuts[-1][1] == n and all(x[1] == y[0] for x, y in zip(cuts[:-1], cuts[1:]))
    for conv, top in (("sym", np.maximum(a, b)), ("fold8", np.maximum(np.maximum(a, b), np.maximum(c, d)))):
        for p0, p1 in cuts:
            j, k = get_jk(eri * ((top >= p0) & (top < p1)), ops.dm)
            np.testing.assert_array_equal(jc.slab_reference(ops.b, ops.dm, p0, p1, conv), np.stack([j.sum(0), *k]))
    for conv in ("sym", "lower", "fold8"):
        np.testing.assert_array_equal(sum(jc.slab_reference(ops.b, ops.dm, p0, p1, conv) for p0, p1 in cuts), whole)
    for p0, p1 in cuts:
        low = jc.slab_reference(ops.b, ops.dm, p0, p1, "lower")
        sym = jc.slab_reference(ops.b, ops.dm, p0, p1, "sym")
        np.testing.assert_array_equal(np.tril(low), np.tril(sym))
        np.testing.assert_array_equal(low, low.transpose(0, 2, 1))
        np.testing.assert_array_equal(jc.slab_reference(ops.b, ops.dm, p0, p1, "rows"), whole[:, p0:p1])


def test_factorised_jk_is_the_c_oracle_at_a_mid_size():
    n = 52
    ops = jc.operands(n)
    eri = np.ascontiguousarray(jc.dense_tensor(ops.b))
    np.testing.assert_array_equal(cref.jk(eri, np.ascontiguousarray(ops.dm)), jc.jk_reference(ops.b, ops.dm))
    p0, p1 = 17, 23
    rows = cref.jk(np.ascontiguousarray(eri[p0:p1]), np.ascontiguousarray(ops.dm), p0, p1)
    np.testing.assert_array_equal(rows, jc.slab_reference(ops.b, ops.dm, p0, p1, "rows"))


@pytest.mark.parametrize("case", [c for c in jc.AO2MO_CASES if c.n <= 37], ids=lambda c: f"{c.n}-{c.n1}")
def test_factorised_ao2mo_is_the_einsum_definition(case):
    ops = jc.operands(case.n)
    c1, c2, c3, c4, c5, c6 = jc.ao2mo_coefficients(case)
    eri = jc.dense_tensor(ops.b)
    np.testing.assert_array_equal(jc.ao2mo_reference(ops.b, c1, c2, c3, c4), hamiltonian.ao2mo_full(eri, c1, c2, c3, c4))
    np.testing.assert_array_equal(jc.ao2mo_reference(ops.b, c1, c2, c5, c6), hamiltonian.ao2mo_full(eri, c1, c2, c5, c6))
    np.testing.assert_array_equal(jc.ao2mo_reference(ops.b, c1, c2, c3, c4), cref.ao2mo(np.ascontiguousarray(eri), c1, c2, c3, c4))
    packed = jc.pack_rs(eri)
    assert packed.shape == (case.n, case.n, case.n * (case.n + 1) // 2)
    assert packed[3, 2, 4 * 5 // 2 + 1] == eri[3, 2, 4, 1]


# ------------------------------------------------------------------------------------------ the operand family
def test_every_tensor_entry_is_odd_and_wrong_index_orders_rarely_coincide():
    from itertools import permutations

    n = 24
    ops = jc.operands(n)
    eri = jc.dense_tensor(ops.b)
    assert np.array_equal(np.abs(eri) % 2, np.ones_like(eri)) and np.abs(eri).min() >= 1
    group = {(0, 1, 2, 3), (1, 0, 2, 3), (0, 1, 3, 2), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 0, 1), (2, 3, 1, 0), (3, 2, 1, 0)}
    worst = 0.0
    for perm in permutations(range(4)):
        same = float(np.mean(eri == eri.transpose(perm)))
        if perm in group:
            assert same == 1.0, perm
        else:
            worst = max(worst, same)
    print(f"largest share of entries equal under an index order outside the 8-fold group: {worst:.3f}")
    assert worst <= 0.25
    for x in (ops.b, ops.dm, ops.hv):
        np.testing.assert_array_equal(x, x.transpose(0, 2, 1))
    assert set(np.unique(ops.b[0])) == {-3.0, -1.0, 1.0, 3.0} and set(np.unique(ops.b[1])) == {-2.0, 0.0, 2.0}
    assert set(np.unique(ops.dm[0])) == {-3.0, -1.0, 1.0, 3.0} and set(np.unique(ops.dm[1])) == {-5.0, -3.0, -1.0, 1.0, 3.0, 5.0}
    # swapping the spins changes K everywhere it matters
    k = jc.jk_reference(ops.b, ops.dm)[1:]
    assert np.mean(k[0] != k[1]) > 0.9
    assert ops.e.min() == -jc.EXP_RANGE and ops.e.max() == jc.EXP_RANGE


def all_sizes():
    return sorted({c.n for c in jc.PACKED_CASES} | {c.n for cs in jc.SWITCH_CASES.values() for c in cs}
                  | {c.n for c in jc.DENSE_CASES} | {c.n for c in jc.SYM_CASES} | set(jc.FAMILY_CASES.values()))


def test_every_case_stays_below_two_to_the_52():
    worst = 0.0
    for n in all_sizes():
        ops = jc.operands(n)
        jmax, kmax = jc.headroom(ops.b, ops.dm)
        # (+ hv in the Fock epilogue; the graded variant has the same integers: headroom of the integer parts)
        worst = max(worst, jmax + kmax + np.abs(ops.hv).max())
        g = jc.graded(ops)
        gj, gk = jc.headroom(g.b, g.dm)
        scale = jc.grade(ops.e).max()
        assert gj <= jmax * scale and gk <= kmax * scale
    print(f"largest sum of |terms| over all J/K cases: {worst:.3g}")
    assert worst < 2.0 ** 52
    for case in jc.AO2MO_CASES:
        big = jc.ao2mo_headroom(jc.operands(case.n).b, jc.ao2mo_coefficients(case))
        print(f"ao2mo {tuple(case[:5])}: sum of |terms| {big:.3g}")
        assert big < 2.0 ** 52


# ------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("case", jc.PACKED_CASES, ids=jc.packed_id)
def test_packed_case_reaches_its_kernel(lib, case):
    assert jc.route(lib, case.n) == (case.kernel, case.run_as), case.why
    assert lib.nbx_jk_packed_supported(case.n) == (1 if case.run_as == case.n else 2)
    assert lib.nbx_jk_packed_fold(case.n) == (8 if case.kernel == jc.M8 else 4)


def test_every_packed_instance_the_dispatch_can_select_is_in_the_table(lib):
    """Every (kernel, instance size) nbx_jk_packed_route answers for any N, and every (NB, LPT) instance of jk_s4.hip
    below jk_m8.hip's range (NB^2 LPT = nbx_jk_dts_bytes / 1024), has an unpadded entry; padded entries exist for each
    kernel; the ranges the header documents hold."""
    reachable = {jc.route(lib, n) for n in range(0, 460)} - {(jc.NONE, 0)}
    own = {(c.kernel, c.run_as) for c in jc.PACKED_CASES if c.run_as == c.n}
    s4_sizes = {r for k, r in reachable if k == jc.S4}
    s4_classes = {lib.nbx_jk_dts_bytes(n) // 1024 for n in s4_sizes}
    assert {k for k, _ in reachable} == {jc.S4, jc.M8, jc.MX, jc.MX_HI}
    assert {kr for kr in reachable if kr[0] != jc.S4} == {kr for kr in own if kr[0] != jc.S4}
    assert {r for k, r in own if k == jc.S4} <= s4_sizes
    assert {lib.nbx_jk_dts_bytes(n) // 1024 for n in jc.S4_CLASSES} == s4_classes == {8, 24, 40, 32, 96}
    assert all(lib.nbx_jk_dts_bytes(n) // 1024 == cls for n, cls in jc.S4_CLASSES.items())
    assert set(jc.S4_CLASSES) == {c.n for c in jc.S4_CASES if c.run_as == c.n}
    # the first and the last size of every class are entries (the class boundaries are where a retuning moves sizes)
    for cls in s4_classes:
        members = sorted(n for n in s4_sizes if lib.nbx_jk_dts_bytes(n) // 1024 == cls)
        assert members[0] in jc.S4_CLASSES, (cls, members)
    for kern in (jc.S4, jc.M8, jc.MX, jc.MX_HI):
        assert any(c.kernel == kern and c.run_as != c.n for c in jc.PACKED_CASES), kern
    assert {c.n % 4 for c in jc.M8_CASES if c.run_as != c.n} == {1, 2, 3}
    assert sorted(r for k, r in reachable if k == jc.M8) == jc.M8_INSTANCES and len(jc.M8_INSTANCES) == 13
    assert sorted(r for k, r in reachable if k in (jc.MX, jc.MX_HI)) == jc.MX_LO_INSTANCES + jc.MX_HI_INSTANCES
    assert len(jc.MX_LO_INSTANCES + jc.MX_HI_INSTANCES) == 23
    # the ranges: s4 below, m8 for 97 .. 148, mx for 149 .. 256, mx-hi above
    kern_of = {n: jc.route(lib, n)[0] for n in range(1, 402)}
    assert all(kern_of[n] == jc.NONE for n in range(1, 16)) and all(kern_of[n] == jc.S4 for n in range(16, 97))
    assert all(kern_of[n] == jc.M8 for n in range(97, 149)) and all(kern_of[n] == jc.MX for n in range(149, 257))
    assert {kern_of[n] for n in range(257, 401)} == {jc.MX_HI, jc.NONE} and kern_of[400] == jc.MX_HI and kern_of[401] == jc.NONE
    assert jc.route(lib, 393) == (jc.MX_HI, 400) and jc.route(lib, 391) == (jc.NONE, 0)
    # the family cases run unpadded on the kernel they are named for
    assert {name: jc.route(lib, n) for name, n in jc.FAMILY_CASES.items()} == {
        "s4": (jc.S4, 92), "m8": (jc.M8, 116), "mx-whole": (jc.MX, 168), "mx-hi-whole": (jc.MX_HI, 272),
        "mx-hi-band": (jc.MX_HI, 304)}
    # the Dtot' table of the scalars kernel exists exactly for the unpadded jk_s4.hip and jk_m8.hip sizes
    for c in jc.PACKED_CASES:
        assert (lib.nbx_jk_dts_bytes(c.n) > 0) == (c.kernel in (jc.S4, jc.M8) and c.run_as == c.n), c


@pytest.mark.parametrize("setting", list(jc.SWITCH_CASES), ids=lambda s: s.replace(" ", ","))
def test_switch_cases_reach_their_fallback_kernels(setting):
    """The switches are read once per process: a child process (host arithmetic only, no GPU) asks the routing query
    for every case tests/_jk_exact_worker.py runs under this setting."""
    import os
    import subprocess
    import sys

    code = ("import sys; sys.path.insert(0, sys.argv[1]); import jk_cases as jc; from nbed_amd import _nbx; "
            "lib = _nbx.load_library(); "
            "bad = [(c, jc.route(lib, c.n)) for c in jc.SWITCH_CASES[sys.argv[2]] if jc.route(lib, c.n) != (c.kernel, c.run_as)]; "
            "print('ROUTES', bad); sys.exit(1 if bad else 0)")
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(tests))
    for name in ("NBX_JK_M8", "NBX_JK_M4", "NBX_JK_MX"):
        env.pop(name, None)
    env.update(item.split("=") for item in setting.split())
    r = subprocess.run([sys.executable, "-c", code, tests, setting], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ROUTES []" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    kernels = {c.kernel for c in jc.SWITCH_CASES[setting]}
    assert kernels == {"NBX_JK_M8=0": {jc.M4}, "NBX_JK_M8=0 NBX_JK_M4=0": {jc.S4, jc.MX}, "NBX_JK_MX=0": {jc.S4}}[setting]
    assert any(c.run_as != c.n for c in jc.SWITCH_CASES[setting])


def test_dense_tables_hold_the_smallest_size_of_every_instance():
    classes = {jc.dense_class(n) for n in range(1, 2049) if n % 2 == 0 or n <= 1024}
    assert classes == {(cs, v) for cs in (1, 2, 4) for v in (True, False)}
    assert {(c.cs, c.vec2) for c in jc.DENSE_CASES} == classes
    for cs, vec2 in classes:
        smallest = min(n for n in range(1, 2049) if jc.dense_class(n) == (cs, vec2))
        assert smallest in {c.n for c in jc.DENSE_CASES}, (cs, vec2, smallest)
    for c in jc.DENSE_CASES:
        assert jc.dense_class(c.n) == (c.cs, c.vec2), c
        assert c.rows is not None or 8 * c.n ** 4 <= 2 ** 30, c
        assert c.rows is None or (0 <= c.rows[0] < c.rows[1] <= c.n and 8 * (c.rows[1] - c.rows[0]) * c.n ** 3 <= 2 ** 35), c
    assert any(c.n % 2 for c in jc.DENSE_CASES)
    assert {c.qb for c in jc.SYM_CASES} == {0, 2, 4}
    for c in jc.SYM_CASES:
        assert jc.sym_qb(c.n) == c.qb, c
    assert jc.sym_qb(192) == 2 and jc.sym_qb(194) == 4 and {192, 194} <= {c.n for c in jc.SYM_CASES}
    assert max(c.n for c in jc.SYM_CASES) == 512 and jc.sym_qb(514) == 0


def test_the_dense_class_restatement_matches_the_source():
    """dense_class / sym_qb restate jk_plan and js_qb: the lines they restate are still in the sources."""
    src = _nbx.LIB_PATH.parent / "csrc"
    jk = (src / "jk.hip").read_text()
    assert "constexpr int JK_THREADS = 256;" in jk and "pl.vec2 = (N % 2 == 0);" in jk
    assert "pl.cs = CX <= JK_THREADS ? 1 : (CX <= 2 * JK_THREADS ? 2 : 4);" in jk
    sym = (src / "jk_sym.hip").read_text()
    assert "int js_qb(int64_t N) { return N <= 192 ? 2 : 4; }" in sym and "constexpr int JS_THREADS = 256;" in sym
    assert "return nao >= 2 && nao % 2 == 0 && nao / 2 <= JS_THREADS;" in sym


def test_slab_plans_keep_dense_slabs_within_the_limit():
    for c in jc.PACKED_CASES:
        if c.n >= jc.SLAB_ONLY_FROM:
            slabs = jc.dense_slabs(c.n)
            assert slabs[0][0] == 0 and slabs[-1][1] == c.n and all(x[1] == y[0] for x, y in zip(slabs[:-1], slabs[1:]))
            assert all(8 * (p1 - p0) * c.n ** 3 <= jc.DENSE_SLAB_BYTES for p0, p1 in slabs), c
        else:
            assert 8 * c.n ** 4 * 1.3 < 100 * 2 ** 30, c  # dense + packed, whole


# ------------------------------------------------------------------------------------------ mutations
def tile_walk(b, dm, skip=None, twice=None, halve=True, swap_spins=False):
    """numpy restatement of the 8-fold packed walk (csrc/jk_m8.hip): the tiles (p, q <= p) in sequence, of each the
    elements (rs) <= (pq), (rs) = (pq) halved; J_pq from the tile, J_rs from the mirrored copy, K = Kp + Kp^T.  The
    mutations: `skip` / `twice` = a tile (p, q) visited zero times / twice, halve=False, swap_spins."""
    n = b.shape[-1]
    dtot = dm.sum(axis=0)
    dtp = dtot + dtot.T - np.diag(np.diag(dtot))  # D_ab + D_ba, D_aa
    pair = lambda a, c: a * (a + 1) // 2 + c
    j = np.zeros((n, n))
    kp = np.zeros((dm.shape[0], n, n))
    for p in range(n):
        for q in range(p + 1):
            visits = 0 if (p, q) == skip else 2 if (p, q) == twice else 1
            for _ in range(visits):
                tile = np.einsum("l,lrs->rs", b[:, p, q], b)
                for r in range(p + 1):
                    for s in range(r + 1):
                        if pair(r, s) > pair(p, q):
                            break
                        e = tile[r, s] * (0.5 if halve and pair(r, s) == pair(p, q) else 1.0)
                        j[p, q] += e * dtp[r, s]
                        j[r, s] += e * dtp[p, q]
                        e *= (0.5 if p == q else 1.0) * (0.5 if r == s else 1.0)
                        for x in range(dm.shape[0]):
                            kp[x, p, r] += e * dm[x, q, s]
                            kp[x, p, s] += e * dm[x, q, r]
                            kp[x, q, r] += e * dm[x, p, s]
                            kp[x, q, s] += e * dm[x, p, r]
    j = np.tril(j) + np.tril(j, -1).T
    k = kp + kp.transpose(0, 2, 1)
    if swap_spins:
        k = k[::-1]
    return np.stack([j, *k])


def test_the_exact_comparison_fails_for_every_mutation_of_the_tile_walk():
    n = 9
    ops = jc.operands(n)
    ref = jc.jk_reference(ops.b, ops.dm)
    jc.assert_exact(tile_walk(ops.b, ops.dm), ref, "unmutated walk")
    g = jc.graded(ops)
    jc.assert_exact(tile_walk(g.b, g.dm), jc.jk_reference(g.b, g.dm), "unmutated walk, graded")
    for name, kw in (("skip one tile", {"skip": (5, 2)}), ("skip a diagonal tile", {"skip": (4, 4)}),
                     ("count one tile twice", {"twice": (7, 0)}), ("do not halve (rs) = (pq)", {"halve": False}),
                     ("swap K's spins", {"swap_spins": True})):
        with pytest.raises(AssertionError, match="elements differ"):
            jc.assert_exact(tile_walk(ops.b, ops.dm, **kw), ref, name)
        with pytest.raises(AssertionError, match="elements differ"):
            jc.assert_exact(tile_walk(g.b, g.dm, **kw), jc.jk_reference(g.b, g.dm), name + ", graded")
    # the smallest slips: one element off by one unit in the last place, a NaN, a shape
    off = ref.copy()
    off[2, 3, 4] = np.nextafter(off[2, 3, 4], np.inf)
    with pytest.raises(AssertionError, match="1 of"):
        jc.assert_exact(off, ref)
    off[2, 3, 4] = np.nan
    with pytest.raises(AssertionError):
        jc.assert_exact(off, ref)
    with pytest.raises(AssertionError):
        jc.assert_exact(ref[:, :-1], ref)
