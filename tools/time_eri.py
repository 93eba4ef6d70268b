"""(pq|rs) of a molecule by the two routes of BuiltinHFProvider: wall time of the host route
(integrals.two_electron_native + be.asarray, with 16 threads and with nthreads = 0 = every hardware thread) and of the
device route (HipBackend.eri: pair data on the host, their upload, the class launches, a final synchronise), each the
median of five runs after one warm-up, alternating the routes; then the class launches one by one from HIP events (a
run of its own: the event pairs hold the stream), the quartets per class, and the largest difference of the two tensors.

    python tools/time_eri.py [octane|butane|propane|ethane|water|h2o2] [basis] [out.json]"""
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

MOLECULES = {
    "octane": octane_xyz,
    "ethane": lambda: octane_xyz(2), "propane": lambda: octane_xyz(3), "butane": lambda: octane_xyz(4),
    "water": lambda: "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459",
    "h2o2": lambda: "4\n\nO   0.000  0.734  -0.052\nO   0.000  -0.734  -0.052\nH   0.839  0.881  0.419\nH   -0.839  -0.881  0.419",
}
RUNS = 5

name = sys.argv[1] if len(sys.argv) > 1 else "octane"
basis = sys.argv[2] if len(sys.argv) > 2 else "6-31g*"
out_path = sys.argv[3] if len(sys.argv) > 3 else None

be = HipBackend()
bs = integrals.Basis(integrals.parse_geometry(MOLECULES[name]()), basis)
n = bs.nao
print(f"{name} / {basis}: {n} AOs, {len(bs.shells)} shells, tensor {8 * n ** 4 / 1e9:.3f} GB", flush=True)


def host_route(nthreads):
    be.synchronize()
    t0 = time.perf_counter()
    h = integrals.two_electron_native(bs, nthreads=nthreads)
    t1 = time.perf_counter()
    d = be.asarray(h)
    be.synchronize()
    t2 = time.perf_counter()
    return d, {"total_s": t2 - t0, "engine_s": t1 - t0, "upload_s": t2 - t1}


def device_route():
    be.synchronize()
    t0 = time.perf_counter()
    d = be.eri(bs)
    t1 = time.perf_counter()  # (the call returns once the pair data are uploaded and the launches queued)
    be.synchronize()
    t2 = time.perf_counter()
    return d, {"total_s": t2 - t0, "host_part_s": t1 - t0, "wait_s": t2 - t1}


routes = {"host_16_threads": lambda: host_route(16), "host_all_threads": lambda: host_route(0), "device": device_route}
samples = {k: [] for k in routes}
for rnd in range(RUNS + 1):  # round 0 is the warm-up of every route (code objects, allocator, pinned staging)
    for key, fn in routes.items():
        d, t = fn()
        del d
        torch.cuda.empty_cache()
        if rnd:
            samples[key].append(t)
result = {"molecule": name, "basis": basis, "nao": n, "nshell": len(bs.shells), "tensor_bytes": 8 * n ** 4, "runs": RUNS,
          "routes": {}}
for key, rows in samples.items():
    result["routes"][key] = {f: statistics.median(r[f] for r in rows) for f in rows[0]}
    result["routes"][key]["total_s_all"] = [r["total_s"] for r in rows]
    print(f"{key}: " + ", ".join(f"{f} {v * 1e3:.1f} ms" for f, v in result["routes"][key].items() if f != "total_s_all")
          + f"  (totals {min(r['total_s'] for r in rows) * 1e3:.1f} .. {max(r['total_s'] for r in rows) * 1e3:.1f} ms)", flush=True)
result["device_over_host_16"] = result["routes"]["device"]["total_s"] / result["routes"]["host_16_threads"]["total_s"]

# the class launches, bracketed by events
import ctypes  # noqa: E402

ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
counts = (ctypes.c_int64 * 25)()
lds, block, grid = (ctypes.c_int * 25)(), (ctypes.c_int * 25)(), (ctypes.c_int64 * 25)()
_nbx.check(be.lib, be.lib.nbx_eri_plan(len(bs.shells), *(ptr(a) for a in integrals._shell_arrays(bs)), 1e-16, counts, lds, block,
                                       grid))
be.profile(True, slots=[_nbx.PROF_ERI])
per_class = []
for _ in range(RUNS + 1):
    d = be.eri(bs)
    per_class.append(be.eri_class_ms())
    del d
be.profile(False)
ms = np.median(np.array(per_class[1:]), axis=0)
result["classes"] = [{"l_ab": a, "l_cd": c, "quartets": int(counts[5 * a + c]), "lds_bytes": int(lds[5 * a + c]),
                      "workgroups": int(grid[5 * a + c]), "ms": float(ms[a, c])} for a in range(5) for c in range(5)]
result["class_ms_sum"] = float(ms.sum())
print(f"class launches (events), sum {ms.sum():.2f} ms; quartets {sum(counts[:])}")
for row in result["classes"]:
    if row["quartets"]:
        print(f"  ({row['l_ab']},{row['l_cd']}): {row['quartets']:>9d} quartets, {row['workgroups']:>5d} workgroups, "
              f"LDS {row['lds_bytes']:>6d} B, {row['ms']:9.3f} ms, {row['ms'] * 1e6 / row['quartets']:9.1f} ns per quartet")

d_dev = be.eri(bs)
d_host, _ = host_route(16)
result["max_abs_difference"] = float((d_dev - d_host).abs().max())
print(f"max |device - host| = {result['max_abs_difference']:.3e}")
print(json.dumps({k: v for k, v in result.items() if k != "classes"}))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
