"""The pivoted Cholesky factor of (pq|rs) on the device (HipBackend.eri_cholesky) for the molecules
of DESIGN.md section 12's table at tol = 1e-4, 1e-6, 1e-8: rank, rank / N, steps, columns computed, and wall time up to
a final synchronise as the median of five runs after one warm-up.  Beside it, from the same process and alternating with
it, the device route's dense tensor (HipBackend.eri) -- the thing to compare against -- unless ``--no-dense`` (a molecule
whose tensor is not wanted).  The factor's largest residual against that dense tensor is reported where it was made.

    python tools/time_eri_cholesky.py [octane|butane|propane|ethane|water|h2o2|dodecane|hexadecane] [basis] [out.json] [--no-dense]"""
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import torch  # noqa: E402

from molecules import octane_xyz  # noqa: E402
from nbed_amd import integrals  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402

MOLECULES = {
    "octane": octane_xyz,
    "ethane": lambda: octane_xyz(2), "propane": lambda: octane_xyz(3), "butane": lambda: octane_xyz(4),
    "dodecane": lambda: octane_xyz(12), "hexadecane": lambda: octane_xyz(16),
    "water": lambda: "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459",
    "h2o2": lambda: "4\n\nO   0.000  0.734  -0.052\nO   0.000  -0.734  -0.052\nH   0.839  0.881  0.419\nH   -0.839  -0.881  0.419",
}
RUNS = 5
TOLS = (1e-4, 1e-6, 1e-8)

args = [a for a in sys.argv[1:] if not a.startswith("--")]
with_dense = "--no-dense" not in sys.argv
name = args[0] if args else "octane"
basis = args[1] if len(args) > 1 else "6-31g*"
out_path = args[2] if len(args) > 2 else None

be = HipBackend()
bs = integrals.Basis(integrals.parse_geometry(MOLECULES[name]()), basis)
n = bs.nao
print(f"{name} / {basis}: {n} AOs, {len(bs.shells)} shells, {n * (n + 1) // 2} pairs, dense tensor {8 * n ** 4 / 1e9:.3f} GB", flush=True)


def dense():
    be.synchronize()
    t0 = time.perf_counter()
    d = be.eri(bs)
    be.synchronize()
    return d, time.perf_counter() - t0


def cholesky(tol):
    be.synchronize()
    t0 = time.perf_counter()
    b = be.eri_cholesky(bs, tol=tol)
    be.synchronize()
    return b, time.perf_counter() - t0


samples = {tol: [] for tol in TOLS}
dense_s = []
info = {}
for rnd in range(RUNS + 1):  # round 0 warms every route up (code objects, allocator)
    if with_dense:
        d, t = dense()
        del d
        torch.cuda.empty_cache()
        if rnd:
            dense_s.append(t)
    for tol in TOLS:
        b, t = cholesky(tol)
        info[tol] = dict(be.eri_cholesky_info)
        del b
        torch.cuda.empty_cache()
        if rnd:
            samples[tol].append(t)

result = {"molecule": name, "basis": basis, "nao": n, "nshell": len(bs.shells), "pairs": n * (n + 1) // 2, "runs": RUNS,
          "dense_device_s": statistics.median(dense_s) if dense_s else None, "dense_device_s_all": dense_s, "tols": []}
if dense_s:
    print(f"dense tensor on the device: {result['dense_device_s'] * 1e3:.1f} ms ({min(dense_s) * 1e3:.1f} .. {max(dense_s) * 1e3:.1f})")
ref = be.eri(bs).reshape(n * n, n * n) if with_dense and 8 * n ** 4 < 8e9 else None
for tol in TOLS:
    med = statistics.median(samples[tol])
    row = {"tol": tol, **info[tol], "rank_over_n": info[tol]["rank"] / n, "factor_bytes": 8 * info[tol]["rank"] * n * n,
           "seconds": med, "seconds_all": samples[tol],
           "over_dense": med / result["dense_device_s"] if dense_s else None}
    if ref is not None:
        b2 = be.eri_cholesky(bs, tol=tol).reshape(-1, n * n)
        row["max_abs_residual_vs_device_tensor"] = float((ref - be.gemm(b2, b2, "T", "N")).abs().max())  # (not timed)
        del b2
    result["tols"].append(row)
    print(f"tol {tol:g}: rank {row['rank']} ({row['rank_over_n']:.2f} N), {row['steps']} steps, {row['columns']} columns, "
          f"{med * 1e3:.1f} ms ({min(samples[tol]) * 1e3:.1f} .. {max(samples[tol]) * 1e3:.1f})"
          + (f", {row['over_dense']:.2f} of the dense time" if dense_s else "")
          + (f", max |R| = {row['max_abs_residual_vs_device_tensor']:.2e}" if ref is not None else ""), flush=True)
print(json.dumps(result))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
