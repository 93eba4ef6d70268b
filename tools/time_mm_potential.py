"""The MM potential V_mm of a molecule in a shell of point charges, three ways:

  baseline   nbx_host_1e with the charges passed as its atoms, 16 threads: the only way to such a matrix before
             nbx_host_mm_potential / nbx_mm_potential existed (it also fills S and T, which it cannot be asked to skip)
  host       integrals.mm_potential_native (nbx_host_mm_potential), 16 threads
  device     HipBackend.mm_potential (nbx_mm_potential): pair data on the host, uploads, launches, final synchronise --
             the whole call, from host arrays to a finished device matrix

for M = 1 024, 16 384 and 65 536 charges at fixed-seed positions 5 to 30 bohr from the nearest atom.  One warm-up round,
then RUNS rounds alternating the routes; a route whose call takes more than SLOW_S seconds is run once.  Medians, all
samples, the work (primitive pairs x charges) and the largest |device - host| go to the JSON file.

    python tools/time_mm_potential.py [octane|water] [basis] [out.json] [M ...]"""
import ctypes
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np  # noqa: E402

from molecules import octane_xyz  # noqa: E402
from nbed_amd import _nbx, integrals  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402

MOLECULES = {"octane": octane_xyz,
             "water": lambda: "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"}
RUNS, SLOW_S, THREADS = 5, 2.0, 16

name = sys.argv[1] if len(sys.argv) > 1 else "octane"
basis = sys.argv[2] if len(sys.argv) > 2 else ("6-31g*" if name == "octane" else "cc-pvdz")
out_path = sys.argv[3] if len(sys.argv) > 3 else None
sizes = [int(a) for a in sys.argv[4:]] or [1024, 16384, 65536]

be = HipBackend()
lib = _nbx.load_library()
atoms = integrals.parse_geometry(MOLECULES[name]())
bs = integrals.Basis(atoms, basis)
arrays = integrals._shell_arrays(bs)
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
nprim = [len(sh.exps) for sh in bs.shells]
prim_pairs = sum(a * b for i, a in enumerate(nprim) for b in nprim[: i + 1])
print(f"{name} / {basis}: {bs.nao} AOs, {len(bs.shells)} shells, {prim_pairs} primitive pairs", flush=True)


def environment(m, seed=20251019):
    """m charges of +-0.4 .. 0.8 e, each 5 to 30 bohr from the nearest atom (rejection from a box around the molecule)."""
    rng = np.random.default_rng(seed + m)
    pos = np.array([p for _, p in atoms])
    lo, hi = pos.min(axis=0) - 30.0, pos.max(axis=0) + 30.0
    out = np.empty((0, 3))
    while len(out) < m:
        c = rng.uniform(lo, hi, (4 * m, 3))
        d = np.linalg.norm(c[:, None, :] - pos[None, :, :], axis=2).min(axis=1)
        out = np.concatenate([out, c[(d >= 5.0) & (d <= 30.0)]])
    q = rng.uniform(0.4, 0.8, m) * rng.choice([-1.0, 1.0], m)
    return np.ascontiguousarray(out[:m]), np.ascontiguousarray(q)


def baseline(xyz, q):
    out = [np.empty((bs.nao, bs.nao)) for _ in range(3)]
    t0 = time.perf_counter()
    _nbx.check(lib, lib.nbx_host_1e(len(bs.shells), *(ptr(a) for a in arrays), len(q), ptr(q), ptr(xyz), THREADS,
                                    *(ptr(o) for o in out)))
    return out[2], time.perf_counter() - t0


def host(xyz, q):
    t0 = time.perf_counter()
    v = integrals.mm_potential_native(bs, xyz, q, nthreads=THREADS)
    return v, time.perf_counter() - t0


def device(xyz, q):
    be.synchronize()
    t0 = time.perf_counter()
    v = be.mm_potential(bs, xyz, q)  # (returns with the stream idle)
    be.synchronize()
    return v, time.perf_counter() - t0


result = {"molecule": name, "basis": basis, "nao": bs.nao, "nshell": len(bs.shells), "primitive_pairs": prim_pairs,
          "threads": THREADS, "runs": RUNS, "chunk": be.MM_CHUNK, "sizes": []}
device(*environment(64))  # code objects, allocator
for m in sizes:
    xyz, q = environment(m)
    routes = {"baseline_host_1e": baseline, "host": host, "device": device}
    samples, slow, keep = {k: [] for k in routes}, set(), {}
    for rnd in range(RUNS + 1):  # round 0 is the warm-up; its time decides whether a route is repeated at all
        for key, fn in routes.items():
            if key in slow:
                continue
            v, t = fn(xyz, q)
            keep[key] = be.to_host(v) if key == "device" else v
            if rnd == 0 and t > SLOW_S:
                slow.add(key)
                samples[key].append(t)
            elif rnd:
                samples[key].append(t)
    row = {"charges": m, "work": prim_pairs * m,
           "max_abs_device_minus_host": float(np.abs(keep["device"] - keep["host"]).max()),
           "max_abs_host_minus_baseline": float(np.abs(keep["host"] - keep["baseline_host_1e"]).max()),
           "max_abs_v": float(np.abs(keep["host"]).max()), "routes": {}}
    for key, ts in samples.items():
        row["routes"][key] = {"median_s": statistics.median(ts), "all_s": ts, "single_run": key in slow}
    row["baseline_over_device"] = row["routes"]["baseline_host_1e"]["median_s"] / row["routes"]["device"]["median_s"]
    row["host_over_device"] = row["routes"]["host"]["median_s"] / row["routes"]["device"]["median_s"]
    result["sizes"].append(row)
    print(f"M = {m}: " + ", ".join(f"{k} {r['median_s'] * 1e3:.2f} ms" for k, r in row["routes"].items())
          + f"; |device - host| {row['max_abs_device_minus_host']:.1e}", flush=True)
    if out_path:  # (after every size: a run that is cut short leaves what it measured)
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)
print(json.dumps(result))
