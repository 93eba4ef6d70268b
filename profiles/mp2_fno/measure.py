"""Timings of nbx_mp2_pairs, its composite baseline, solve_scf and the FNO + truncated Hamiltonian build."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
from nbed_amd import mp2  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402
from nbed_amd.ham_builder import HamiltonianBuilder  # noqa: E402
from nbed_amd.scf import GpuUHF, Mole, huzinaga_scf  # noqa: E402
from nbed_amd import synth  # noqa: E402

be = HipBackend(0)
be.use_current_stream()
out = {"device": torch.cuda.get_device_name(0)}


def timed(fn, warmup=3, reps=20, min_window=0.25):
    """Median of ``reps`` event-bracketed windows, each of enough calls to last min_window seconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); one = time.perf_counter() - t0
    inner = max(1, int(min_window / reps / max(one, 1e-6)))
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record(); b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "calls_per_window": inner, "windows": reps}


# ---------------------------------------------------------------- the kernel against the composite
kern = []
for no, nv in ((13, 115), (33, 115), (33, 256)):
    rng = np.random.default_rng(no * nv)
    x = rng.standard_normal((no * nv, no * nv))
    v = be.asarray((x + x.T).reshape(no, nv, no, nv))
    eo_h, ev_h = -1.0 - rng.random(no), 0.5 + rng.random(nv)
    eo, ev = be.asarray(eo_h), be.asarray(ev_h)
    d = be.asarray(((eo_h[:, None, None, None] + eo_h[None, None, :, None]) - ev_h[None, :, None, None]) - ev_h[None, None, None, :])
    n = v.numel()
    g_buf = be.empty(v.shape)

    def composite(device_sum=False):
        """The same (T in the kernel's layout, pair energy) from entry points that existed before the kernel."""
        g_buf.copy_(v)
        be.permute4(v, (0, 3, 2, 1), alpha=-1.0, beta=1.0, out=g_buf)   # g = V[iajb] - V[ibja]
        t = g_buf / d                                                      # the denominator tensor, made beforehand
        if device_sum:  # the energy stays on the device, as the fused call leaves it: no host round trip in the window
            e = 0.25 * torch.dot(t.reshape(-1), g_buf.reshape(-1))
        else:           # nbx_dots returns the value to the host: every call synchronises
            e = 0.25 * be.dots(t.reshape(-1), g_buf.reshape(1, -1))[0]
        return be.permute4(t, (1, 0, 2, 3)), e

    def fused():
        return be.mp2_pairs(v, eo, ev, eo, ev, True)

    t_f, e_f = fused()
    t_c, e_c = composite()
    e_d = float(composite(True)[1])
    e_f = float(be.to_host(e_f)[0])
    assert abs(e_f - e_c) <= 1e-10 * abs(e_c) and abs(e_d - e_c) <= 1e-10 * abs(e_c), (e_f, e_c, e_d)
    assert float((t_f - t_c).abs().max()) < 1e-12
    out.setdefault("bitwise_equal_to_composite", []).append(bool(torch.equal(t_f, t_c)))
    row = {"no": no, "nv": nv, "elements": n, "block_MB": 8 * n / 1e6,
           "fused_same": timed(fused), "composite_dots": timed(composite),
           "composite_device_sum": timed(lambda: composite(True)),
           "fused_opposite": timed(lambda: be.mp2_pairs(v, eo, ev, eo, ev, False))}
    for key in ("fused_same", "fused_opposite"):
        row[key]["GB_per_s"] = 16 * n / row[key]["median_ms"] / 1e6   # V read once, T written once
        row[key]["fraction_of_8TBps"] = row[key]["GB_per_s"] / 8000.0
    row["speedup_vs_composite_dots"] = row["composite_dots"]["median_ms"] / row["fused_same"]["median_ms"]
    row["speedup_vs_composite_device_sum"] = row["composite_device_sum"]["median_ms"] / row["fused_same"]["median_ms"]
    kern.append(row)
    print(json.dumps(row), flush=True)
    del v, d, g_buf, t_f, t_c
out["mp2_pairs"] = kern

# ---------------------------------------------------------------- solver and FNO on the bench's embedded shape
N, nocc, n_env, nact = 148, (33, 33), 20, 128
pr = synth.problem(be, N, nocc, n_env)
mf = GpuUHF(Mole(N, pr["nelec"]), pr["S"], pr["hcore"], be.synth_eri(N), backend=be)
mf.max_cycle, mf.conv_tol = 60, 1e-9
c, e, dm, hz, conv = huzinaga_scf(mf, pr["V_emb"], pr["D_env"], dm_conv_tol=1e-7)
mf.mo_coeff, mf.mo_energy = c[:, :, :nact], e[:, :nact]
mf.mo_occ = mf.get_occ(e, c)[:, :nact]
h3 = pr["hcore"] + hz + pr["V_emb"]
mf.get_hcore = lambda *a: h3
mf.e_tot = mf.energy_tot()
no = int(mf.mo_occ[0].sum()); nv = nact - no
k = 20  # (reduce_virtuals refuses k >= the number of occupied spin orbitals, 26 here)
out["embedded_shape"] = {"nao": N, "mo": nact, "no": no, "nv": nv, "converged": bool(conv), "k": k}


def wall(fn, reps=3):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "runs": reps}, r


out["solve_scf"], res = wall(lambda: mp2.solve_scf(mf, backend=be))
out["e_mp2"] = res.e_corr
out["build_full"], _ = wall(lambda: HamiltonianBuilder(mf, 0.0, backend=be).build_spatial_device())
out["build_by_order"], _ = wall(lambda: HamiltonianBuilder(mf, 0.0, n_frozen_virt=k, backend=be).build_spatial_device())


def fno_build():
    b = HamiltonianBuilder(mf, 0.0, n_frozen_virt=k, backend=be, virtual_selection="fno")
    b.build_spatial_device()
    return b.fno


out["fno_plus_truncated_build"], info = wall(fno_build)
out["fno_alone"], _ = wall(lambda: mp2.frozen_natural_orbitals(mf, n_frozen_virt=k, backend=be))
out["fno_info"] = {x: info[x] for x in ("n_virtual", "n_kept", "e_mp2_full", "e_mp2_kept", "e_correction")}
dst = Path(__file__).resolve().parent
dst.mkdir(exist_ok=True)
(dst / "mp2_measure_mi355x.json").write_text(json.dumps(out, indent=1))
print(json.dumps({x: out[x] for x in out if x != "mp2_pairs"}, indent=1))
