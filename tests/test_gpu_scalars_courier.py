"""Deferred scalars of the settled SCF cycle: the last kernel of a cycle stops at its partial sums and the J/K build of
the next cycle (csrc/jk_m8.hip) takes them to the host in its prologue (csrc/scalars_courier.h), or nbx_huz_scalars_flush
does in a launch of its own.  Who finishes the sums and when must not change one bit of anything, so every comparison
here is byte for byte between the immediate form (nbx_huz_cycle) and the deferred one (nbx_huz_cycle_carry).

Sizes: N = 100, 116, 148 -- the 8-fold instances whose scalars kernel has 49, 64 and 100 workgroups: less than one
wavefront of partial sums, exactly one, two.  Whole runs of huzinaga_scf at N = 100.

Inputs: the synthetic embedded problem of oracle/synth.py on the generated integrals (be.synth_eri)."""

import ctypes

import numpy as np
import pytest

from oracle import synth

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

CASES = {100: ((24, 24), 10), 116: ((30, 29), 12), 148: ((33, 33), 20)}  # N: (occupied per spin with the environment, n_env)
BLOCKS = {100: 49, 116: 64, 148: 100}
RESULT_KEYS = ("dm", "c", "w", "hz")


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    yield HipBackend()
    _operands.clear()
    _immediate.clear()


_operands = {}  # the device operands of the size last used (one packed tensor at a time: 0.6 GB at N = 148)
_immediate = {}  # the immediate two-cycle run of that size: the reference of every comparison, computed once


def operands(be, n):
    if n not in _operands:
        _operands.clear()
        _immediate.clear()
        nocc, n_env = CASES[n]
        pr = synth.problem(n, nocc, n_env)
        s = pr["S"]
        w, u = np.linalg.eigh(s)
        x = (u / np.sqrt(w)) @ u.T
        hv = np.broadcast_to(pr["hcore"], (2, n, n)) + np.broadcast_to(pr["V_emb"], (2, n, n))
        _, c0 = synth.lowdin_orthonormal(s, pr["hcore"])
        dm0 = np.stack([c0[:, :k] @ c0[:, :k].T for k in pr["nelec"]])
        assert BLOCKS[n] == ((n + 15) // 16) ** 2
        assert be.lib.nbx_jk_packed_fold(n) == 8, "jk_m8.hip is the kernel that carries"
        _operands[n] = {
            "nelec": pr["nelec"], "packed": be.eri_pack(be.synth_eri(n), n), "hv": be.asarray(np.ascontiguousarray(hv)),
            "ds": be.asarray(np.ascontiguousarray(pr["D_env"] @ s)), "s_b": be.asarray(np.stack([s, s])),
            "x": be.asarray(0.5 * (x + x.T)), "dm0": be.asarray(dm0),
        }
    return _operands[n]


def new_state(be, n):
    op = operands(be, n)
    return be.huz_cycle_state(n, op["nelec"], op["packed"], op["hv"], op["ds"], op["s_b"], op["x"], be.jk_dts_new(n))


def seven(pend) -> bytes:
    return pend._host.numpy()[:7].tobytes()


def ready(pend) -> float:
    return float(pend._host.numpy()[6])


def two_cycles(be, n, defer: bool):
    """A guarded cycle from the core guess and one warm-started from its vectors behind it (a guarded cycle writes every
    result whatever its refinement decides: nothing compared here is memory that no kernel wrote).  Returns the bytes of
    everything the two cycles leave, and what the ready words said along the way."""
    op = operands(be, n)
    h = new_state(be, n)
    kw = {"defer": True} if defer else {}
    got, seen = {}, {}
    out1, out2 = h.sets[0], h.sets[1]
    p1 = be.huz_cycle(h, op["dm0"], None, out1, 0, 6, 0, 0, 0, False, **kw)
    fock2_1 = h.fock2.clone()  # (queued between the cycles: the second overwrites it)
    if defer:
        assert h.deferred is not None, "the cycle was not deferred"
        be.synchronize()
        seen["cycle 1 after its own kernels"] = ready(p1)
    p2 = be.huz_cycle(h, out1["dm"], out1["v"], out2, 0, 6, 0, 0, 0, True, **kw)
    if defer:
        be.synchronize()
        seen["cycle 1 after the next build"] = ready(p1)
        seen["cycle 2 after its own kernels"] = ready(p2)
        be.huz_flush(h)
        assert h.deferred is None
        be.synchronize()
        seen["cycle 2 after the flush"] = ready(p2)
    p1.get()
    p2.get()
    assert np.all(p1.get_extra() > 0) and np.all(p2.get_extra() > 0), "an eigensolve failed: its results are not written"
    be.synchronize()
    got["scalars 1"], got["scalars 2"] = seven(p1), seven(p2)
    got["fock2 1"] = be.to_host(fock2_1).tobytes()
    for name, t in (("fock2 2", h.fock2), ("jk 2", h.jk), ("fock 2", h.fock), ("vhf 2", h.vhf)):
        got[name] = be.to_host(t).tobytes()
    for i, out in ((1, out1), (2, out2)):
        for k in RESULT_KEYS:
            a = be.to_host(out[k])
            assert np.all(np.isfinite(a)), (i, k)
            got[f"{k} {i}"] = a.tobytes()
    assert np.all(np.isfinite(np.frombuffer(got["scalars 1"] + got["scalars 2"])))
    return got, seen


def immediate(be, n):
    if n not in _immediate:
        operands(be, n)
        _immediate[n] = two_cycles(be, n, False)[0]
    return _immediate[n]


@pytest.mark.parametrize("n", sorted(CASES))
def test_two_cycles_immediate_against_deferred(be, n):
    ref = immediate(be, n)
    got, seen = two_cycles(be, n, True)
    assert sorted(got) == sorted(ref)
    for key in ref:
        assert got[key] == ref[key], f"N = {n}: {key} differs between the immediate and the deferred cycle"
    # the deferral is real: nothing reaches the host before a later call carries or flushes it
    assert seen == {"cycle 1 after its own kernels": 0.0, "cycle 1 after the next build": 1.0,
                    "cycle 2 after its own kernels": 0.0, "cycle 2 after the flush": 1.0}


@pytest.mark.parametrize("n", sorted(CASES))
def test_flush_gives_the_same_seven_doubles(be, n):
    ref = immediate(be, n)
    op = operands(be, n)
    h = new_state(be, n)
    p = be.huz_cycle(h, op["dm0"], None, h.sets[0], 0, 6, 0, 0, 0, False, defer=True)
    assert h.deferred is not None
    assert (h.deferred.nblocks, h.deferred.nthreads, h.deferred.nstatus) == (BLOCKS[n], 128, 2)
    be.synchronize()
    assert ready(p) == 0.0
    be.huz_flush(h)
    p.get()
    assert seven(p) == ref["scalars 1"]
    be.huz_flush(h)  # nothing deferred: nothing queued
    be.synchronize()


@pytest.mark.parametrize("n", sorted(CASES))
def test_a_call_with_nothing_to_carry_writes_no_other_host_slot(be, n):
    """nbx_huz_cycle_carry with a courier whose partials pointer is NULL but whose destination is a poisoned slot: the
    slot keeps its poison, the cycle stores its own scalars as nbx_huz_cycle does."""
    from nbed_amd import _nbx

    ref = immediate(be, n)
    op = operands(be, n)
    h = new_state(be, n)
    out = h.sets[0]
    poison = be.torch.full((8,), float("nan"), dtype=be.torch.float64).pin_memory()
    before = poison.numpy().tobytes()
    own = be.torch.zeros(7, dtype=be.torch.float64).pin_memory()
    nothing = _nbx.ScalarsCourier()
    nothing.h_out, nothing.nblocks, nothing.nthreads, nothing.nstatus = poison.data_ptr(), BLOCKS[n], 128, 2
    left = _nbx.ScalarsCourier()
    be._call("nbx_huz_cycle_carry", ctypes.byref(h.st), be._p(op["dm0"]), None, be._p(out["dm"]), be._p(out["c"]),
             be._p(out["v"]), be._p(out["w"]), be._p(out["hz"]), 0, 6, 0, 0, 0, 0, be._p(own), be._p(out["status"]),
             ctypes.byref(nothing), 0, ctypes.byref(left))
    be.synchronize()
    assert not left.d_partial  # not requested: not deferred
    assert poison.numpy().tobytes() == before
    assert own.numpy().tobytes() == ref["scalars 1"]


# ------------------------------------------------------------------------------------------ whole runs
def whole_run(be, monkeypatch, defer: str, by_convergence: bool):
    from nbed_amd.scf import GpuUHF, History, Mole, huzinaga_scf

    n = 100
    nocc, n_env = CASES[n]
    pr = synth.problem(n, nocc, n_env)
    monkeypatch.setenv("NBED_DEFER_SCALARS", defer)
    mf = GpuUHF(Mole(n, pr["nelec"]), pr["S"], pr["hcore"], be.synth_eri(n), backend=be)
    assert mf.eri_packed_device() is not None
    if by_convergence:
        mf.conv_tol, mf.max_cycle = 1e-7, 60
    else:
        mf.conv_tol, mf.max_cycle = -1.0, 4
    flushed = []
    flush = type(be).huz_flush
    monkeypatch.setattr(be, "huz_flush", lambda h: (flushed.append(getattr(h, "deferred", None) is not None), flush(be, h))[1])
    hist = History()
    res = huzinaga_scf(mf, pr["V_emb"], pr["D_env"], dm_conv_tol=1e-6, use_DIIS=True, backend=be, history=hist)
    return res, hist, flushed


@pytest.mark.parametrize("by_convergence", [True, False], ids=["converged", "max_cycle"])
def test_whole_runs_are_identical(be, monkeypatch, by_convergence):
    operands(be, 100)  # (frees another size's packed tensor)
    (r_off, h_off, f_off), (r_on, h_on, f_on) = (whole_run(be, monkeypatch, d, by_convergence) for d in ("0", "1"))
    assert h_off.info["deferred_scalars"] is False and h_on.info["deferred_scalars"] is True
    assert f_off == [] and any(f_on), "the run with the deferral on ends with a flush of a deferred cycle"
    assert h_off.info["restarts"] == h_on.info["restarts"]
    assert len(h_on) == len(h_off) and r_on[4] == r_off[4] == by_convergence
    if not by_convergence:
        assert len(h_on) == 4
    for (e_on, d_on), (e_off, d_off) in zip(h_on, h_off):
        assert np.asarray(e_on).tobytes() == np.asarray(e_off).tobytes() and d_on == d_off
    for a_on, a_off in zip(r_on[:4], r_off[:4]):
        assert np.all(np.isfinite(a_on))
        assert np.asarray(a_on).tobytes() == np.asarray(a_off).tobytes()


# ------------------------------------------------------------------------------------------ every launch geometry
def dpp_wave_sum(v):
    """nbx_wave_sum_dpp on 64 lanes, addition by addition (csrc/nbx_common.h): neighbours, pairs, the mirrored half row
    of 8, the mirrored row of 16, then the four rows as (0 + 16) + (32 + 48).  IEEE additions in numpy: exact."""
    lane = np.arange(64)
    v = v + v[lane ^ 1]
    v = v + v[lane ^ 2]
    v = v + v[(lane & ~7) | (7 - (lane & 7))]
    v = v + v[(lane & ~15) | (15 - (lane & 15))]
    return (v[0] + v[16]) + (v[32] + v[48])


def last_stage_reference(partial, nthreads):
    """huz_scalars_kernel's last stage: thread tid takes blocks tid, tid + nthreads, ..; a sum per wave; waves in order."""
    nblocks = partial.shape[0]
    out = np.zeros(4)
    for o in range(4):
        tot = np.float64(0.0)
        for w in range(nthreads // 64):
            t = np.zeros(64)
            for lane in range(64):
                for b in range(w * 64 + lane, nblocks, nthreads):
                    t[lane] = t[lane] + partial[b, o]
            tot = tot + dpp_wave_sum(t)
        out[o] = np.sqrt(tot) if o >= 2 else tot
    return out


# 128 threads: less than a wave, two waves, the trailing loop; 256 threads: two of four waves, all four exactly, trailing loop
@pytest.mark.parametrize("nthreads,nblocks", [(128, 49), (128, 100), (128, 300), (256, 100), (256, 256), (256, 700)])
def test_courier_on_hand_made_partials(be, nthreads, nblocks):
    """nbx_huz_scalars_flush on partials made here, for both launch geometries the courier admits and block counts on
    either side of one block per virtual thread, against the last stage restated in numpy -- bit for bit (entries 2 and 3
    are non-negative, as sums of squares are)."""
    from nbed_amd import _nbx

    rng = np.random.default_rng([nthreads, nblocks])
    partial = rng.standard_normal((nblocks, 4))
    partial[:, 2:] = np.abs(partial[:, 2:])
    status = np.array([1003, -7], dtype=np.int32)
    d_partial, d_status = be.asarray(partial), be.torch.tensor(status, device=be.device)
    host = be.torch.zeros(7, dtype=be.torch.float64).pin_memory()
    c = _nbx.ScalarsCourier()
    c.d_partial, c.nblocks, c.nthreads = d_partial.data_ptr(), nblocks, nthreads
    c.d_status, c.nstatus, c.h_out = d_status.data_ptr(), 2, host.data_ptr()
    be._call("nbx_huz_scalars_flush", ctypes.byref(c))
    be.synchronize()
    want = np.concatenate([last_stage_reference(partial, nthreads), status.astype(np.float64), [1.0]])
    assert host.numpy().tobytes() == want.tobytes(), (host.numpy(), want)
    # a description the courier is not written for is refused, nothing queued
    c.nthreads = 64
    with pytest.raises(_nbx.NbxError):
        be._call("nbx_huz_scalars_flush", ctypes.byref(c))
    c.nthreads, c.d_partial = nthreads, d_partial.data_ptr() + 8  # (not 16-byte aligned)
    with pytest.raises(_nbx.NbxError):
        be._call("nbx_huz_scalars_flush", ctypes.byref(c))
