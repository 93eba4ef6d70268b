"""The small kernels the SCF cycle queues (nbed_amd/csrc/elementwise.hip, chained by csrc/scf_cycle.hip) on the MI355X,
against tests/scf_kernel_cases.py: exact operands compared for equality, real-valued operands compared against the
derived rounding bound (the worst error / bound per kernel is printed), at every kernel instance and at the sizes where
a tile, a trip of loads, a grid cap or a launch path changes.  Data is far from any fixed point: dm and dm_old are
unrelated matrices."""

import ctypes

import numpy as np
import pytest

import scf_kernel_cases as sk
from nbed_amd import _nbx

# (the shared operands are read-only numpy arrays; they are only ever copied to the device)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
LD = sk.LD
WORST = {}


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


def judge(kernel, got, ref, bound, what=""):
    """Real-valued operands: |got - ref| <= bound everywhere; the worst ratio per kernel is kept and printed."""
    ratio = sk.worst_ratio(got, ref, bound)
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: worst |got - ref| / bound = {ratio:.3e} (kernel so far {WORST[kernel]:.3e})")
    assert ratio <= 1.0, (kernel, what, ratio)


def same(got, ref):
    """Exact operands: the longdouble reference is a float64 number and the result is that number."""
    ref64 = np.asarray(ref, dtype=np.float64)
    assert np.all(np.asarray(ref, dtype=LD) == ref64.astype(LD))
    np.testing.assert_array_equal(got, ref64)


def compare(kind, kernel, got, ref, bound, what=""):
    if kind == "exact":
        same(got, ref)
    else:
        judge(kernel, got, ref, bound, what)


def refused(be, rc, code=_nbx.NBX_E_INVALID):
    assert rc == code, (rc, be.lib.nbx_last_error())


class pinned_slot_untouched:
    """The slot of pinned host memory the next asynchronous scalars call stores into: after a refused call its four
    results are what they were and its "all stored" word, which the wrapper cleared, is still 0."""

    def __init__(self, be):
        self.be = be

    def __enter__(self):
        self.slot = self.be._pin_ring[self.be._pin_next]
        self.slot[:4] = -7.0
        return self

    def __exit__(self, *exc):
        self.be.synchronize()
        np.testing.assert_array_equal(self.slot[:5].numpy(), [-7.0] * 4 + [0.0])
        return False


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------ Fock assembly
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 37])  # n^2 = 1, 225, 256, 289 (one block, its edge, two), 1369
def test_fock_uhf(be, N, kind):
    h3, vemb, jk = sk.fock_operands(kind, N)
    for h in (h3, h3[0]):
        for v in (None, vemb):
            fock, vhf = be.fock_uhf(be.asarray(h), None if v is None else be.asarray(v), be.asarray(jk))
            f_ref, v_ref, bf, bv = sk.fock_reference(h, v, jk)
            compare(kind, "fock_uhf", be.to_host(fock), f_ref, bf, f"N={N} fock")
            compare(kind, "fock_uhf", be.to_host(vhf), v_ref, bv, f"N={N} vhf")
    fock, vhf = be.fock_uhf(be.asarray(h3), be.asarray(vemb), be.asarray(jk), want_vhf=False)
    assert vhf is None
    np.testing.assert_array_equal(be.to_host(fock), be.to_host(be.fock_uhf(be.asarray(h3), be.asarray(vemb), be.asarray(jk))[0]))


# ------------------------------------------------------------------------------------------ Huzinaga operator
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("N", sk.HUZ_SIZES)
def test_huzinaga_fused_and_sym(be, N, batch, kind):
    f3, ds3 = sk.huz_operands(kind, N, batch)
    f, ds = (f3[0], ds3[0]) if batch == 1 else (f3, ds3)  # batch 1 is the 2-D form
    f_d, ds_d = be.asarray(f), be.asarray(ds)
    fds_d = be.gemm(f_d, ds_d)
    fds = be.to_host(fds_d)
    for kappa in (1.0, 0.5):
        hz_ref, fo_ref, bh, bf = sk.huz_fused_reference(f, ds, kappa)
        hz_d, fo_d = be.huzinaga_fused(f_d, ds_d, kappa, want_fock=True)
        hz, fo = be.to_host(hz_d), be.to_host(fo_d)
        compare(kind, "huzinaga_fused", hz, hz_ref, bh, f"N={N} batch={batch} kappa={kappa} hz")
        compare(kind, "huzinaga_fused", fo, fo_ref, bf, f"N={N} batch={batch} kappa={kappa} fock")
        np.testing.assert_array_equal(hz, np.swapaxes(hz, -1, -2))  # symmetric to the bit
        np.testing.assert_array_equal(be.to_host(f_d), f)  # the input is untouched
        hz_only, none = be.huzinaga_fused(f_d, ds_d, kappa, want_fock=False)
        assert none is None
        np.testing.assert_array_equal(be.to_host(hz_only), hz)
        # the two-kernel path: product, then the symmetrisation (judged against the device's own product)
        for with_fock in (False, True):
            io = be.asarray(f) if with_fock else None
            hz2 = be.to_host(be.huzinaga_sym(fds_d, kappa, io))
            h_ref, o_ref, b1, b2 = sk.huz_sym_reference(fds, kappa, f if with_fock else None)
            compare(kind, "huzinaga_sym", hz2, h_ref, b1, f"N={N} batch={batch} kappa={kappa} hz")
            np.testing.assert_array_equal(hz2, np.swapaxes(hz2, -1, -2))
            if with_fock:
                compare(kind, "huzinaga_sym", be.to_host(io), o_ref, b2, f"N={N} batch={batch} kappa={kappa} fock")
            if kind == "exact":  # the fused result IS GEMM + huzinaga_sym
                np.testing.assert_array_equal(hz2, hz)
                if with_fock:
                    np.testing.assert_array_equal(be.to_host(io), fo)


# ------------------------------------------------------------------------------------------ trace
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("N", sk.TRACE_SIZES)
def test_trace_prod(be, N, kind):
    a, b = sk.trace_operands(kind, N)
    ref, bound = sk.trace_reference(a, b)
    a_d, b_d = be.asarray(a), be.asarray(b)
    got2 = be.trace_prod(a_d, b_d)
    got1 = be.trace_prod(a_d[1], b_d[1])
    compare(kind, "trace_prod", got2, ref, bound, f"N={N} batch 2")
    compare(kind, "trace_prod", np.array([got1]), ref[1:], bound[1:], f"N={N} 2-D")
    assert got1 == got2[1]


def test_trace_prod_refuses_what_its_scratch_cannot_hold(be):
    N = sk.TRACE_REFUSED
    a = be.zeros((N, N))
    out = (ctypes.c_double * 1)(-7.0)
    refused(be, be.lib.nbx_trace_prod(be.ctx, N, 1, ptr(a), ptr(a), out))
    assert out[0] == -7.0


# ------------------------------------------------------------------------------------------ the cycle's scalars
def scalars_variants(ops):
    """(hcore, vemb) forms: 2-D and 3-D hcore, vemb None and given."""
    h3, vemb = ops[0], ops[1]
    return [(h3, vemb), (h3[0], vemb), (h3, None), (h3[0], None)]


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("N", sk.SYNC_SIZES)
def test_huz_cycle_scalars_sync(be, N, kind):
    ops = sk.scalars_operands(kind, N)
    _, _, vhf, hz, dm, dm_old = ops
    dv = [be.asarray(x) for x in (vhf, hz, dm, dm_old)]
    for h, vemb in scalars_variants(ops)[: 4 if N <= 100 else 1]:
        got = be.huz_cycle_scalars(be.asarray(h), None if vemb is None else be.asarray(vemb), *dv)
        worst = sk.check_scalars(got, sk.scalars_reference(h, vemb, vhf, hz, dm, dm_old), exact=kind == "exact")
        if kind == "real":
            WORST["huz_scalars<32> sync"] = max(WORST.get("huz_scalars<32> sync", 0.0), worst)
            print(f"huz_cycle_scalars N={N}: worst error / bound {worst:.3e}")


def test_huz_cycle_scalars_refuse_a_size_past_the_scratch(be):
    N = sk.REFUSED_SIZE
    z = be.zeros((2, N, N))
    out = (ctypes.c_double * 4)(*([-7.0] * 4))
    refused(be, be.lib.nbx_huz_cycle_scalars(be.ctx, N, ptr(z), 3, None, ptr(z), ptr(z), ptr(z), ptr(z), out))
    assert list(out) == [-7.0] * 4
    assert be.lib.nbx_cycle_scalars_route(N, -1, -1) == sk.SC_REFUSED
    with pinned_slot_untouched(be):
        with pytest.raises(_nbx.NbxError) as err:
            be.huz_cycle_scalars_async(z, None, z, z, z, z)
    assert err.value.code == _nbx.NBX_E_INVALID


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("N", sk.ASYNC_T16 + sk.ASYNC_T32)
def test_huz_cycle_scalars_async(be, N, kind):
    want = sk.SC_T16 if N in sk.ASYNC_T16 else sk.SC_T32
    assert be.lib.nbx_cycle_scalars_route(N, -1, -1) == want
    ops = sk.scalars_operands(kind, N)
    _, _, vhf, hz, dm, dm_old = ops
    dv = [be.asarray(x) for x in (vhf, hz, dm, dm_old)]
    name = f"huz_scalars<{16 if want == sk.SC_T16 else 32}> async"
    torch = be.torch
    extras = [None, torch.tensor([3, -5], dtype=torch.int32, device=be.device),
              torch.arange(-31, 33, dtype=torch.int32, device=be.device) * 1000003]
    for k, (h, vemb) in enumerate(scalars_variants(ops)):  # (the third, (h3, None), carries the 64-word tail)
        extra = extras[k % 3]
        args = (be.asarray(h), None if vemb is None else be.asarray(vemb), *dv)
        pend = be.huz_cycle_scalars_async(*args, extra=extra)
        got = pend.get()
        worst = sk.check_scalars(got, sk.scalars_reference(h, vemb, vhf, hz, dm, dm_old), exact=kind == "exact")
        if kind == "real":
            WORST[name] = max(WORST.get(name, 0.0), worst)
            print(f"{name} N={N}: worst error / bound {worst:.3e}")
        if extra is None:
            assert pend.get_extra() is None
        else:
            np.testing.assert_array_equal(pend.get_extra(), extra.cpu().numpy().astype(np.int64))
        again = be.huz_cycle_scalars_async(*args, extra=extra)
        np.testing.assert_array_equal(again.get(), got)  # the same call twice: the same bits
    with pytest.raises(ValueError):
        be.huz_cycle_scalars_async(*args, extra=torch.zeros(65, dtype=torch.int32, device=be.device))


@pytest.mark.parametrize("N", sk.DTS_SIZES[:2])
def test_huz_cycle_scalars_leave_the_next_builds_dtot_table(be, N):
    """With `dts` the scalars kernel leaves Dtot' of D for the next packed J/K build: the numpy restatement
    (sum_x (D_ab + D_ba) below the diagonal, sum_x D_aa on it; exact operands) at the offsets of the restated layout
    (scf_kernel_cases.dts_layout), zeros elsewhere; and the Fock matrices of a build from this table equal those of
    a build that prepares its own, bit for bit (as test_jk_packed_fock_and_prepared_dtot_table)."""
    assert be.jk_packed_supported(N)
    ops = sk.scalars_operands("exact", N)
    h3, vemb, vhf, hz, dm0, dm_old = ops
    dm = dm0 + np.swapaxes(dm0, -1, -2)  # (the build contracts a symmetric density)
    dts = be.jk_dts_new(N)
    args = [be.asarray(x) for x in (h3, vemb, vhf, hz, dm, dm_old)]
    plain = be.huz_cycle_scalars_async(*args).get()
    got = be.huz_cycle_scalars_async(*args, dts=dts).get()
    np.testing.assert_array_equal(got, plain)
    table = be.to_host(dts)
    idx, size = sk.dts_layout(N)
    assert table.size == size
    want = np.zeros(size)  # (the slots no pair owns stay zero)
    low = np.tril_indices(N)
    want[idx[low]] = sk.dts_restatement(dm)[low]
    np.testing.assert_array_equal(table, want)
    # a second density overwrites every entry the first wrote
    args[4] = be.asarray(2.0 * dm)
    be.huz_cycle_scalars_async(*args, dts=dts).get()
    np.testing.assert_array_equal(be.to_host(dts), 2.0 * table)
    # ... and the packed build reads it where the kernel put it
    packed = be.eri_pack(be.synth_eri(N), N)
    hv = be.asarray(h3)
    fock0, vhf0 = be.jk_packed_fock(packed, args[4], hv)
    fock1, vhf1 = be.jk_packed_fock(packed, args[4], hv, dts=dts)
    assert be.torch.equal(fock0, fock1) and be.torch.equal(vhf0, vhf1)


def test_no_dtot_table_for_a_zero_padded_size(be):
    """An odd size the packed build accepts by zero padding (117) prepares its table itself: there is none to hand
    to the scalars kernel, and a call that passes one is refused with nothing stored."""
    N = sk.DTS_SIZES[2]
    assert N % 2 == 1 and be.jk_packed_supported(N) and be.lib.nbx_jk_dts_bytes(N) == 0
    with pytest.raises(ValueError):
        be.jk_dts_new(N)
    z = be.zeros((2, N, N))
    with pinned_slot_untouched(be):
        with pytest.raises(_nbx.NbxError) as err:
            be.huz_cycle_scalars_async(z, None, z, z, z, z, dts=be.zeros(1 << 16))
    assert err.value.code == _nbx.NBX_E_INVALID
    ops = sk.scalars_operands("exact", N)
    got = be.huz_cycle_scalars_async(*[be.asarray(x) for x in ops]).get()
    sk.check_scalars(got, sk.scalars_reference(*ops), exact=True)


# ------------------------------------------------------------------------------------------ the post-Fock chain
def run_huz_cycle(be, h, jk_d, dm_in_d, c_in, out, mode, iters, diis_mode):
    def inject(jk):
        jk.copy_(jk_d)

    pend = be.huz_cycle(h, dm_in_d, c_in, out, mode, iters, diis_mode, 0, 1, False, reduce=inject)
    return pend.get(), pend.get_extra()


def chain_state(be, N, nocc):
    hv, jk, ds, dm_in, s, x = sk.chain_operands(N)
    dts = be.jk_dts_new(N) if N in sk.DTS_SIZES[:2] else None
    s_b = be.asarray(np.stack([s, s]))
    h = be.huz_cycle_state(N, nocc, None, be.asarray(hv), be.asarray(ds), s_b, be.asarray(x), dts, eri=None, p0=0, p1=0)
    h.dts = dts
    return h, be.asarray(jk), be.asarray(dm_in)


def check_chain_elementwise(be, h, out, N, diis_mode):
    """Fock assembly, Huzinaga operator and DIIS hand-over of a cycle: exact from the injected J/K."""
    hv, jk, ds, _, _, _ = sk.chain_operands(N)
    f_ref, v_ref, _, _ = sk.fock_reference(hv, None, jk)
    same(be.to_host(h.fock), f_ref)
    same(be.to_host(h.vhf), v_ref)
    fock = f_ref.astype(np.float64)
    hz_ref, f2_ref, _, _ = sk.huz_fused_reference(fock, ds, 1.0)
    same(be.to_host(out["hz"]), hz_ref)
    same(be.to_host(h.fock2), f2_ref)
    if diis_mode == 1:
        np.testing.assert_array_equal(be.to_host(h.diis_xprev), be.to_host(h.fock2).reshape(-1))


def check_chain_scalars(be, h, out, dm_in_d, scal, name):
    """The four scalars against longdouble on the device's own tensors, and bit for bit against the stand-alone
    scalars kernel on them; the Dtot' table against the one that kernel leaves."""
    hv_d = h.keep[2]
    hv, vhf, hz, dm, dm_in = (be.to_host(t) for t in (hv_d, h.vhf, out["hz"], out["dm"], dm_in_d))
    worst = sk.check_scalars(scal, sk.scalars_reference(hv, None, vhf, hz, dm, dm_in), exact=False)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"{name} N={h.n} nocc={h.nelec}: worst error / bound {worst:.3e}")
    table = None if h.dts is None else h.dts.clone()
    alone = be.huz_cycle_scalars_async(hv_d, None, h.vhf, out["hz"], out["dm"], dm_in_d, dts=h.dts)
    np.testing.assert_array_equal(scal, alone.get())
    if table is not None:
        assert be.torch.equal(table, h.dts) and float(table.abs().max()) > 0


@pytest.mark.parametrize("N,nocc", sk.CHAIN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_post_fock_chain_cold(be, N, nocc):
    """nbx_huz_cycle_post on a chosen J/K (an empty integral slab, the J/K copied in through the reduce seam), cold
    guarded eigensolve: everything element-wise around the eigensolver, judged against the device's own orbitals."""
    fused = (N, nocc) in sk.CHAIN_FUSED
    assert be.lib.nbx_cycle_scalars_route(N, *nocc) == (sk.SC_T16_DENS if fused else sk.SC_T16)
    h, jk_d, dm_in_d = chain_state(be, N, nocc)
    out = h.sets[0]
    scal, status = run_huz_cycle(be, h, jk_d, dm_in_d, None, out, 0, 6, 1)
    # (the guarded solver's status words live in its workspace, not in out["status"], which mode 0 does not write)
    off = int(be.lib.nbx_eigh_status_offset(N, 2))
    words = h.eig_work[off:off + 8].clone().view(be.torch.int32).cpu().numpy()
    np.testing.assert_array_equal(status, words.astype(np.int64))
    check_chain_elementwise(be, h, out, N, 1)
    dm_d = out["dm"]
    assert be.torch.equal(dm_d, be.density_occ(out["c"], nocc))  # the fused density IS the product's, bit for bit
    c, dm = be.to_host(out["c"]), be.to_host(dm_d)
    assert np.all(np.isfinite(c))
    d_ref, d_bound = sk.density_reference(c, nocc)
    for x in range(2):
        if nocc[x] == 0:
            assert not dm[x].any()  # an empty spin: exact zeros
        else:
            judge("density" + (" fused" if fused else " gemm"), dm[x], d_ref[x], d_bound[x], f"N={N} nocc={nocc[x]}")
    np.testing.assert_array_equal(dm, np.swapaxes(dm, -1, -2))
    check_chain_scalars(be, h, out, dm_in_d, scal, "huz_scalars<16, DENS>" if fused else "huz_scalars<16> after gemm")
    # the same call again: the same bits
    out2 = h.sets[1]
    scal2, status2 = run_huz_cycle(be, h, jk_d, dm_in_d, None, out2, 0, 6, 1)
    np.testing.assert_array_equal(scal2, scal)
    np.testing.assert_array_equal(status2, status)
    assert all(be.torch.equal(out[k], out2[k]) for k in ("dm", "c", "w", "hz"))


@pytest.mark.parametrize("N,nocc", [(16, (3, 2)), (148, (40, 39))], ids=lambda v: str(v).replace(" ", ""))
def test_post_fock_chain_tracked(be, N, nocc):
    """Mode 1: the orbitals refined from the cold cycle's on the pencil (F, S); the status words are the tracked
    solver's own."""
    h, jk_d, dm_in_d = chain_state(be, N, nocc)
    cold = h.sets[0]
    run_huz_cycle(be, h, jk_d, dm_in_d, None, cold, 0, 6, 0)
    out = h.sets[1]
    scal, status = run_huz_cycle(be, h, jk_d, dm_in_d, cold["c"], out, 1, 6, 0)
    np.testing.assert_array_equal(status, out["status"].cpu().numpy().astype(np.int64))
    check_chain_elementwise(be, h, out, N, 0)
    assert be.torch.equal(out["dm"], be.density_occ(out["c"], nocc))
    dm = be.to_host(out["dm"])
    d_ref, d_bound = sk.density_reference(be.to_host(out["c"]), nocc)
    judge("density fused", dm, d_ref, d_bound, f"tracked N={N}")
    np.testing.assert_array_equal(dm, np.swapaxes(dm, -1, -2))
    check_chain_scalars(be, h, out, dm_in_d, scal, "huz_scalars<16, DENS>")


def test_post_fock_chain_purified(be):
    """Mode 2: the density by purification -- no orbitals and no levels are written; the scalars are the stand-alone
    kernel's on that density."""
    N, nocc = 17, (8, 8)
    h, jk_d, dm_in_d = chain_state(be, N, nocc)
    out = h.sets[0]
    out["c"].fill_(-7.0)
    out["w"].fill_(-7.0)
    scal, status = run_huz_cycle(be, h, jk_d, dm_in_d, None, out, 2, 60, 1)
    np.testing.assert_array_equal(status, out["status"].cpu().numpy().astype(np.int64))
    assert float(out["c"].min()) == float(out["c"].max()) == -7.0 and float(out["w"].min()) == float(out["w"].max()) == -7.0
    check_chain_elementwise(be, h, out, N, 1)
    assert np.all(np.isfinite(be.to_host(out["dm"])))
    check_chain_scalars(be, h, out, dm_in_d, scal, "huz_scalars<16> after purification")
    scal2, _ = run_huz_cycle(be, h, jk_d, dm_in_d, None, h.sets[1], 2, 60, 1)
    np.testing.assert_array_equal(scal2, scal)


# ------------------------------------------------------------------------------------------ DIIS
def diis_device_ring(be, space, n):
    return {"xs": be.zeros((space, n)), "es": be.zeros((space, n)), "h": be.asarray(sk.pulay_matrix(space)),
            "coef": be.diis_coef_buffer(space), "out": be.zeros(n)}


@pytest.mark.parametrize("n", sk.DIIS_NS)
@pytest.mark.parametrize("space", sk.DIIS_SPACES)
def test_diis_update_err(be, space, n):
    """nbx_diis_update_err over space + 3 updates (the ring wraps; spaces >= 8 go from the fused kernel to the general
    one on the same H): stored vectors and Pulay matrix exact, the extrapolation against the device's own coefficients,
    the coefficients against the longdouble Pulay solve."""
    ring, host = diis_device_ring(be, space, n), sk.DiisHost(space, n)
    seen = set()
    for t, (slot, nd) in enumerate(sk.diis_schedule(space)):
        x, e = sk.diis_vectors(space, n, t)
        seen.add(be.lib.nbx_diis_route(n, nd))
        be.diis_update_err(space, slot, nd, be.asarray(x), be.asarray(e), ring["out"], ring["xs"], ring["es"], ring["h"],
                           ring["coef"])
        hs = host.push(slot, nd, x, e)
        np.testing.assert_array_equal(be.to_host(ring["xs"][slot]), x)
        np.testing.assert_array_equal(be.to_host(ring["es"][slot]), e)
        h_dev = be.to_host(ring["h"])
        np.testing.assert_array_equal(h_dev, host.h, err_msg=f"update {t}")  # exact, hence symmetric
        if sk.diis_singular_by_construction(n, nd):
            continue
        coef = be.to_host(ring["coef"])[:nd]
        assert np.all(np.isfinite(coef))
        ref, bound = host.extrapolate(coef, nd)
        fused = be.lib.nbx_diis_route(n, nd) == sk.DIIS_FUSED
        judge("diis fused" if fused else "diis general", be.to_host(ring["out"]), ref, bound, f"space={space} n={n} update {t}")
        c_ref = sk.pulay_solve(hs)[1:]
        cb = sk.diis_coef_bound(hs, c_ref)
        err = float(np.max(np.abs(coef.astype(LD) - c_ref)))
        key = "diis coefficients " + ("fused" if fused else "general")
        WORST[key] = max(WORST.get(key, 0.0), err / cb)
        assert err <= cb, (t, err, cb)
        sum_err = abs(float(np.sum(coef.astype(LD)) - 1))
        WORST[key + " (sum - 1)"] = max(WORST.get(key + " (sum - 1)", 0.0), sum_err / cb)
        assert sum_err <= cb, (t, coef, sum_err, cb)
    if t == len(sk.diis_schedule(space)) - 1:
        print(f"diis space={space} n={n}: coefficients worst error / bound so far "
              f"{ {k: f'{v:.2e}' for k, v in WORST.items() if k.startswith('diis coef')} }")
    assert seen == ({sk.DIIS_FUSED, sk.DIIS_GENERAL} if space >= 8 else {sk.DIIS_FUSED})


@pytest.mark.parametrize("space,n", [(1, 257), (2, 1), (6, 257), (9, 32769), (16, 32768)])
def test_diis_update_forms_its_own_error_vector(be, space, n):
    """nbx_diis_update: e = x - xprev with xprev the vector the previous update returned -- one IEEE subtraction per
    element, so es[slot] equals numpy's float64 difference to the bit; H is then a sum of real products (bound)."""
    ring = diis_device_ring(be, space, n)
    es = np.zeros((space, n))
    for t, (slot, nd) in enumerate(sk.diis_schedule(space)):
        x, _ = sk.diis_vectors(space, n, t)
        prev = be.to_host(ring["out"])
        be.diis_update(space, slot, nd, be.asarray(x), ring["out"], ring["xs"], ring["es"], ring["h"], ring["coef"])
        es[slot] = x - prev
        np.testing.assert_array_equal(be.to_host(ring["es"][slot]), es[slot])
        np.testing.assert_array_equal(be.to_host(ring["xs"][slot]), x)
        row_ref, row_bound = sk.dots_reference(es[slot], es[:nd])
        h_dev = be.to_host(ring["h"])
        judge("diis push (real)", h_dev[slot + 1, 1:nd + 1], row_ref, row_bound, f"space={space} n={n} update {t}")
        np.testing.assert_array_equal(h_dev, h_dev.T)
        coef = be.to_host(ring["coef"])[:nd]
        xs = be.to_host(ring["xs"])[:nd]
        ref, bound = sk.lincomb_reference(coef, xs)
        fused = be.lib.nbx_diis_route(n, nd) == sk.DIIS_FUSED
        judge("diis fused" if fused else "diis general", be.to_host(ring["out"]), ref, bound, f"update {t}")


def test_diis_refusals_leave_everything_untouched(be):
    n = 256
    for space, slot, nd in ((17, 0, 1), (6, 2, 2), (6, 6, 6), (6, 0, 7), (6, 0, 0)):  # space = 17; slot >= nd; slot >= space; nd > space
        ring = diis_device_ring(be, min(space, 16), n)
        before = {k: v.clone() for k, v in ring.items()}
        x = be.asarray(sk.diis_vectors(6, n, 0)[0])
        rc = be.lib.nbx_diis_update_err(be.ctx, n, space, slot, nd, ptr(x), ptr(x), ptr(ring["out"]), ptr(ring["xs"]),
                                        ptr(ring["es"]), ptr(ring["h"]), ptr(ring["coef"]))
        refused(be, rc)
        assert all(be.torch.equal(ring[k], before[k]) for k in ring), (space, slot, nd)


# ------------------------------------------------------------------------------------------ the mu-shift chain
@pytest.mark.parametrize("N,nocc", sk.MU_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_mu_shift_chain(be, N, nocc):
    """nbx_mu_cycle_solve + nbx_mu_cycle_fock_post around a chosen J/K, ten cycles on a CDIIS ring of eight: the error
    vector formed inside the push kernel, the Fock assembly, the scalars of the form without a Huzinaga operator
    (hz == NULL) with the gradient sums carried behind the status words, and the layout of the pinned slot."""
    torch = be.torch
    h1e, jk, s, x = sk.mu_operands(N)
    s_b = be.asarray(np.stack([s, s]))
    h = be.mu_cycle_state(N, nocc, None, be.asarray(h1e), s_b, be.asarray(x), eri=None, p0=0, p1=0)
    jk_d = be.asarray(jk)
    f_ref, v_ref, _, _ = sk.fock_reference(h1e, None, jk)
    ring = diis_device_ring(be, sk.MU_SPACE, 2 * N * N)  # the same updates through nbx_diis_update_err

    def inject(buf):
        buf.copy_(jk_d)

    for t in range(sk.MU_CYCLES + 1):
        diis_on = t < sk.MU_CYCLES  # (the last cycle runs without DIIS)
        want_grad = t % 2 == 0
        slot, nd = t % sk.MU_SPACE, min(t + 1, sk.MU_SPACE)
        d_in, f_in = sk.mu_cycle_inputs(N, t)
        d_in_d, f_in_d = be.asarray(d_in), be.asarray(f_in)
        out = h.sets[t % 3]
        es_before, h_before = h.diis_es.clone(), h.diis_h.clone()
        pend = be.mu_cycle(h, d_in_d, f_in_d, None, out, False, 6, diis_on, slot, nd, want_grad=want_grad, reduce=inject)
        scal, status, grad = pend.get(), pend.get_extra(), pend.get_dtail()
        if diis_on:
            sdf = np.matmul(np.matmul(s, d_in), f_in)
            err = np.swapaxes(sdf, -1, -2) - sdf
            np.testing.assert_array_equal(be.to_host(h.diis_es[slot]), err.reshape(-1))  # exact
            np.testing.assert_array_equal(be.to_host(h.diis_xs[slot]), f_in.reshape(-1))
            a_d = be.gemm(be.gemm(s_b, d_in_d), f_in_d)
            err_d = (a_d.transpose(1, 2) - a_d).contiguous()
            be.diis_update_err(sk.MU_SPACE, slot, nd, f_in_d.reshape(-1), err_d.reshape(-1), ring["out"], ring["xs"],
                               ring["es"], ring["h"], ring["coef"])
            assert torch.equal(ring["es"][:nd], h.diis_es[:nd]) and torch.equal(ring["xs"][:nd], h.diis_xs[:nd])
            assert torch.equal(ring["h"], h.diis_h) and torch.equal(ring["out"], h.diis_xprev)
            assert torch.equal(ring["coef"][:nd], h.diis_coef[:nd])
        else:
            assert torch.equal(es_before[:nd], h.diis_es[:nd]) and torch.equal(h_before, h.diis_h)
        same(be.to_host(out["fock"]), f_ref)
        same(be.to_host(out["vhf"]), v_ref)
        c, dm = be.to_host(out["c"]), be.to_host(out["dm"])
        assert torch.equal(out["dm"], be.density_occ(out["c"], nocc))
        d_ref, d_bound = sk.density_reference(c, nocc)
        judge("density gemm", dm, d_ref, d_bound, f"mu N={N} cycle {t}")
        fock, vhf = be.to_host(out["fock"]), be.to_host(out["vhf"])
        worst = sk.check_scalars(scal, sk.scalars_reference(h1e, None, vhf, None, dm, d_in), exact=False)
        WORST["huz_scalars<16> hz=NULL"] = max(WORST.get("huz_scalars<16> hz=NULL", 0.0), worst)
        # the pinned slot: 4 scalars, 2 status words, [2 gradient sums,] then 1.0
        raw = pend._host.numpy()
        assert status is not None and status.shape == (2,) and raw.shape == (4 + 2 + (2 if want_grad else 0) + 1,)
        np.testing.assert_array_equal(raw[:4], scal)
        np.testing.assert_array_equal(raw[4:6], status.astype(np.float64))
        assert raw[-1] == 1.0
        if want_grad:
            np.testing.assert_array_equal(raw[6:8], grad)
            g_ref, g_bound = sk.grad_reference(c, fock, nocc)
            judge("vo_sumsq in the mu chain", grad, g_ref, g_bound, f"N={N} cycle {t}")
        else:
            assert grad is None
    print(f"mu chain N={N}: scalars worst error / bound {WORST['huz_scalars<16> hz=NULL']:.3e}")


# ------------------------------------------------------------------------------------------ orbital-gradient sum
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("N,nocc", sk.VO_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_vo_sumsq(be, N, nocc, kind):
    want = sk.VO_32_WG if (N, nocc) == sk.VO_CASES[-1] else sk.VO_ONE_WG
    assert be.lib.nbx_vo_sumsq_route(N, *nocc) == want
    fmo = sk.vo_operands(kind, N, nocc)  # NaN everywhere outside the virtual-occupied blocks
    got = be.to_host(be.vo_sumsq(be.asarray(fmo), nocc))
    ref, bound = sk.vo_reference(fmo, nocc)
    if kind == "exact" or not ref.any():
        same(got, ref)
    else:
        judge(f"vo_sumsq {sk.VO_NAMES[want]}", got, ref, bound, f"N={N} nocc={nocc}")


# ------------------------------------------------------------------------------------------ vector algebra
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("nvec", sk.VEC_NVECS)
@pytest.mark.parametrize("n", sk.VEC_NS)
def test_dots_lincomb_axpby(be, n, nvec, kind):
    x, vecs, coef = sk.vec_operands(kind, n, nvec)
    x_d, vecs_d = be.asarray(x), be.asarray(vecs)
    compare(kind, "dots", be.dots(x_d, vecs_d), *sk.dots_reference(x, vecs), f"n={n} nvec={nvec}")
    compare(kind, "lincomb", be.to_host(be.lincomb(list(coef), vecs_d)), *sk.lincomb_reference(coef, vecs), f"n={n} nvec={nvec}")
    a, b = (float(coef[0]), -0.5) if kind == "exact" else (float(coef[0]), -0.3)
    y = be.asarray(vecs[-1])
    be.axpby(a, x_d, b, y)
    compare(kind, "axpby", be.to_host(y), *sk.axpby_reference(a, x, b, vecs[-1]), f"n={n}")
    y = be.asarray(np.full(n, np.nan))
    be.axpby(a, x_d, 0.0, y)  # b == 0: y is not read
    np.testing.assert_array_equal(be.to_host(y), a * x)


@pytest.fixture(scope="module")
def past_grid(be):
    """Two integer vectors one element longer than a whole grid of 65536 x 256 passes over, on the device, once."""
    n = sk.PAST_GRID_N
    g = be.torch.Generator(device=be.device)
    g.manual_seed(20)
    p = sk.exact_bits(sk.lincomb_budget(2))
    return be.torch.randint(-(2 ** p), 2 ** p + 1, (2, n), generator=g, device=be.device).to(be.torch.float64)


def test_lincomb_and_axpby_past_the_grid_cap(be, past_grid):
    """n = 65536 * 256 + 257: the grid-stride loops make a second pass (exact operands; torch's own float64
    arithmetic on the same integers is exact too)."""
    vecs = past_grid
    out = be.lincomb([1.5, -2.0], vecs)
    assert be.torch.equal(out, 1.5 * vecs[0] - 2.0 * vecs[1])
    y = vecs[1].clone()
    be.axpby(-0.5, vecs[0], 4.0, y)
    assert be.torch.equal(y, -0.5 * vecs[0] + 4.0 * vecs[1])
    y.fill_(float("nan"))
    be.axpby(3.0, vecs[0], 0.0, y)
    assert be.torch.equal(y, 3.0 * vecs[0])


def test_vector_algebra_edges(be):
    n = 256
    x = be.asarray(np.arange(n, dtype=np.float64))
    vecs17 = be.zeros((17, n))
    out = be.asarray(np.full(n, -7.0))
    c17 = (ctypes.c_double * 17)(*([1.0] * 17))
    refused(be, be.lib.nbx_lincomb(be.ctx, n, 17, c17, ptr(vecs17), n, ptr(out)))
    assert float(out.min()) == float(out.max()) == -7.0
    h17 = (ctypes.c_double * 17)(*([-7.0] * 17))
    refused(be, be.lib.nbx_dots(be.ctx, n, 17, ptr(x), ptr(vecs17), n, h17))
    assert list(h17) == [-7.0] * 17
    # n = 0 returns without a launch (null pointers would fault in one)
    assert be.lib.nbx_axpby(be.ctx, 0, 2.0, None, 1.0, None) == _nbx.NBX_OK
    assert be.lib.nbx_lincomb(be.ctx, 0, 1, c17, ptr(vecs17), 0, ptr(out)) == _nbx.NBX_OK
    assert be.lib.nbx_threshold_scale(be.ctx, 0, 1e-8, 0.5, None) == _nbx.NBX_OK
    assert float(out.min()) == float(out.max()) == -7.0


# ------------------------------------------------------------------------------------------ transposes
@pytest.mark.parametrize("rows,cols", sk.TRANSPOSE_SHAPES)
def test_transpose_chem_to_phys_scale_cols(be, rows, cols):
    rng = np.random.default_rng([rows, cols, 21])
    a = sk.real_entries(rng, (3, rows, cols))
    a_d = be.asarray(a)
    np.testing.assert_array_equal(be.to_host(be.transpose(a_d)), np.swapaxes(a, -1, -2))
    np.testing.assert_array_equal(be.to_host(be.transpose(a_d[1].contiguous())), a[1].T)
    # chem_to_phys: out[a,c,d,b] = in[a,b,c,d] -- per a, the (n2) x (n3 n4) transpose
    n3 = 3 if cols % 3 == 0 else 1
    x4 = a.reshape(3, rows, n3, cols // n3)
    np.testing.assert_array_equal(be.to_host(be.chem_to_phys(be.asarray(x4))), x4.transpose(0, 2, 3, 1))
    s = sk.real_entries(rng, (2, cols))
    got = be.to_host(be.scale_cols(be.asarray(a[:2]), be.asarray(s)))
    np.testing.assert_array_equal(got, a[:2] * s[:, None, :])  # one IEEE product per element
    got1 = be.to_host(be.scale_cols(be.asarray(a[2]), be.asarray(s[1])))
    np.testing.assert_array_equal(got1, a[2] * s[1][None, :])


def test_transpose_two_batch_chunks_empty_extents_and_aliasing(be):
    rows, cols, batch = sk.TRANSPOSE_TWO_CHUNKS
    a = be.torch.arange(rows * cols * batch, dtype=be.torch.float64, device=be.device).reshape(batch, rows, cols)
    assert be.torch.equal(be.transpose(a), a.transpose(1, 2).contiguous())
    for shape in ((0, 5), (5, 0)):
        assert be.transpose(be.zeros(shape)).shape == shape[::-1]
    assert be.transpose(be.zeros((0, 4, 4))).shape == (0, 4, 4)
    assert be.chem_to_phys(be.zeros((2, 0, 3, 3))).shape == (2, 3, 3, 0)
    m = be.asarray(np.arange(12.0).reshape(3, 4))
    before = m.clone()
    refused(be, be.lib.nbx_transpose(be.ctx, 3, 4, 1, ptr(m), ptr(m)))
    assert be.torch.equal(m, before)


def test_huzinaga_fused_refuses_an_in_place_update(be):
    f3, ds3 = sk.huz_operands("exact", 17, 2)
    f, ds, hz = be.asarray(f3), be.asarray(ds3), be.asarray(np.full((2, 17, 17), -7.0))
    refused(be, be.lib.nbx_huzinaga_fused(be.ctx, 17, 2, ptr(f), ptr(ds), 1.0, ptr(hz), ptr(f)))
    np.testing.assert_array_equal(be.to_host(f), f3)
    assert float(hz.min()) == float(hz.max()) == -7.0


# ------------------------------------------------------------------------------------------ spin-orbital scatter
TOL = 1e-8


@pytest.mark.parametrize("n", [1, 2, 5, 20])  # n = 20: (2n)^4 = 2.56e6 elements, more than one grid pass of 8192 x 256
def test_spinorb_scatter_and_ranges(be, n):
    one, two = sk.spinorb_operands(n, TOL)
    one_d, two_d = be.asarray(one), be.asarray(two)
    for scale in (1.0, 0.5):
        h1_ref, h2_ref = sk.spinorb_restatement(one, two, TOL, scale)
        h1, h2 = be.spinorb_scatter(one_d, two_d, TOL, scale)
        np.testing.assert_array_equal(be.to_host(h1), h1_ref)
        np.testing.assert_array_equal(be.to_host(h2), h2_ref)
        h1b = be.empty((2 * n, 2 * n))
        be._call("nbx_spinorb_scatter_h1", n, ptr(one_d), TOL, ptr(h1b))
        np.testing.assert_array_equal(be.to_host(h1b), h1_ref)
    flat = h2_ref.reshape(-1)  # (scale 0.5)
    total = flat.size
    ranges = [(0, 0), (total, 0), (total - 1, 1), (0, min(total, 257)), (max(0, total - 300), min(total, 300))]
    if n == 20:
        ranges += [(123457, 8192 * 256 + 77), (total - 8192 * 256 - 3, 8192 * 256 + 3)]  # off any multiple of 256, two passes
    elif total > 700:
        ranges += [(259, 385), (131, total - 131 - 5)]
    for idx0, count in ranges:
        part = be.asarray(np.full(count + 2, -7.0))
        be._call("nbx_spinorb_scatter_range", n, ptr(two_d), TOL, 0.5, idx0, count, ptr(part))
        got = be.to_host(part)
        np.testing.assert_array_equal(got[:count], flat[idx0:idx0 + count], err_msg=str((idx0, count)))
        np.testing.assert_array_equal(got[count:], [-7.0, -7.0])  # nothing past the range
    refused(be, be.lib.nbx_spinorb_scatter_range(be.ctx, n, ptr(two_d), TOL, 0.5, total - 1, 2, ptr(part)))


@pytest.mark.parametrize("n", [1, 255, 257, 8192 * 256 + 77])
def test_threshold_scale_at_its_threshold(be, n):
    below = np.nextafter(TOL, 0.0)
    special = np.array([TOL, -TOL, below, -below, 0.0, 3.0 * TOL, -below / 2])
    rng = np.random.default_rng([n, 22])
    x = rng.choice(special, size=n)
    x[-1] = -TOL
    for scale in (1.0, 0.5):
        got = be.to_host(be.threshold_scale(be.asarray(x), TOL, scale))
        want = np.where(np.abs(x) < TOL, 0.0, x) * scale
        np.testing.assert_array_equal(got, want)
        assert got[-1] == -TOL * scale  # exactly -tol is kept
    assert (np.abs(x) == below).any() or n == 1


def test_zz_worst_ratios():
    """Not a check of its own: the worst error / bound per kernel over the real-valued cases above."""
    for k in sorted(WORST):
        print(f"{k:40s} {WORST[k]:.3e}")
    assert all(v <= 1.0 for v in WORST.values())
