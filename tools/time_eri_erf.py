"""Cost of the attenuated tensor (pq| erf(omega r12) / r12 |rs) beside the plain one on the device,
by the method of tools/time_eri.py / profiles/eri_device: the class launches of HipBackend.eri bracketed by HIP events
(nbx_eri_class_ms), median of five runs after one warm-up, plain and attenuated alternating; the wall time of both calls;
and the extra exchange build of a range-separated Kohn-Sham cycle (the J/K kernel on the attenuated tensor) beside the
cycle's own J/K build.  Run with a library that has no nbx_eri_device_erf (NBX_LIB, an older build) it times the plain
tensor alone: that is the comparison with the commit before.

    python tools/time_eri_erf.py [octane|butane|propane] [basis] [out.json]"""
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from molecules import octane_xyz  # noqa: E402
from nbed_amd import _nbx, integrals  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402

MOLECULES = {"octane": octane_xyz, "propane": lambda: octane_xyz(3), "butane": lambda: octane_xyz(4)}
RUNS, OMEGA = 5, 0.33

name = sys.argv[1] if len(sys.argv) > 1 else "octane"
basis = sys.argv[2] if len(sys.argv) > 2 else "6-31g*"
out_path = sys.argv[3] if len(sys.argv) > 3 else None
have_erf = "nbx_eri_device_erf" in _nbx.SIGNATURES

be = HipBackend()
bs = integrals.Basis(integrals.parse_geometry(MOLECULES[name]()), basis)
n = bs.nao
print(f"{name} / {basis}: {n} AOs, {len(bs.shells)} shells, attenuated entry point: {have_erf}", flush=True)
variants = {"plain": {}}
if have_erf:
    variants["erf"] = {"omega": OMEGA}

be.profile(True, slots=[_nbx.PROF_ERI])
class_ms = {k: [] for k in variants}
for rnd in range(RUNS + 1):
    for key, kw in variants.items():
        d = be.eri(bs, **kw)
        ms = be.eri_class_ms()
        del d
        torch.cuda.empty_cache()
        if rnd:
            class_ms[key].append(ms)
be.profile(False)
wall = {k: [] for k in variants}
for rnd in range(RUNS + 1):
    for key, kw in variants.items():
        be.synchronize()
        t0 = time.perf_counter()
        d = be.eri(bs, **kw)
        be.synchronize()
        t1 = time.perf_counter()
        del d
        torch.cuda.empty_cache()
        if rnd:
            wall[key].append(t1 - t0)
result = {"molecule": name, "basis": basis, "nao": n, "runs": RUNS, "omega": OMEGA, "library_has_erf": have_erf, "tensors": {}}
for key in variants:
    sums = [float(m.sum()) for m in class_ms[key]]
    result["tensors"][key] = {"class_ms_sum": statistics.median(sums), "class_ms_sum_all": sums,
                              "class_ms": np.median(np.array(class_ms[key]), axis=0).tolist(),
                              "wall_s": statistics.median(wall[key]), "wall_s_all": wall[key]}
    print(f"{key}: class launches {statistics.median(sums):.3f} ms ({min(sums):.3f} .. {max(sums):.3f}), wall "
          f"{statistics.median(wall[key]) * 1e3:.1f} ms", flush=True)
if have_erf:
    t = result["tensors"]
    result["erf_over_plain_class_ms"] = t["erf"]["class_ms_sum"] / t["plain"]["class_ms_sum"]
    print(f"attenuated / plain (class launches): {result['erf_over_plain_class_ms']:.4f}")
    # the extra exchange build of a Kohn-Sham cycle: the J/K kernel GpuUKS runs on the attenuated tensor, beside the
    # build on the plain tensor by the same kernel and by the packed kernel the cycle itself uses
    eri, eri_lr = be.eri(bs), be.eri(bs, omega=OMEGA)
    rng = np.random.default_rng(0)
    dm = rng.normal(size=(2, n, n))
    dm_d = be.asarray(dm + dm.transpose(0, 2, 1))
    packed = be.eri_pack(eri, n) if be.jk_packed_supported(n) else None

    def timed(fn):
        out = []
        for rnd in range(RUNS + 1):
            be.synchronize()
            t0 = time.perf_counter()
            fn()
            be.synchronize()
            if rnd:
                out.append(time.perf_counter() - t0)
        return statistics.median(out), out

    builds = {"k_lr_jk_sym": lambda: be.jk_sym(eri_lr, dm_d), "plain_jk_sym": lambda: be.jk_sym(eri, dm_d)}
    if packed is not None:
        builds["plain_jk_packed"] = lambda: be.jk_packed(packed, dm_d)
    result["jk_builds_s"] = {}
    for key, fn in builds.items():
        med, rows = timed(fn)
        result["jk_builds_s"][key] = {"median": med, "all": rows}
        print(f"{key}: {med * 1e3:.3f} ms ({min(rows) * 1e3:.3f} .. {max(rows) * 1e3:.3f})", flush=True)
print(json.dumps({k: v for k, v in result.items() if k != "tensors"}))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
