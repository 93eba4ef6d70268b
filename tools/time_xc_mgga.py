"""Cost of one XCProvider evaluation with a meta-GGA beside a GGA on the device: ``tpss`` against
``pbe`` in the same process on the same grid and AO arrays, the two alternating, medians of five runs after a warm-up,
the whole evaluation (wall time, synchronised) and each of its three kernels bracketed by HIP events.

    python tools/time_xc_mgga.py [octane|butane|propane] [basis] [out.json]"""
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from molecules import octane_xyz  # noqa: E402
from nbed_amd import _nbx, integrals, xc  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402

MOLECULES = {"octane": octane_xyz, "propane": lambda: octane_xyz(3), "butane": lambda: octane_xyz(4)}
RUNS = 5

name = sys.argv[1] if len(sys.argv) > 1 else "octane"
basis = sys.argv[2] if len(sys.argv) > 2 else "6-31g*"
out_path = sys.argv[3] if len(sys.argv) > 3 else None

be = HipBackend()
atoms = integrals.parse_geometry(MOLECULES[name]())
bs = integrals.Basis(atoms, basis)
n = bs.nao
prov = {"pbe": xc.XCProvider(atoms, bs, "pbe", device=be.device)}
prov["tpss"] = xc.XCProvider.__new__(xc.XCProvider)  # the same grid and AO arrays: one copy of the 3 (G, nao) planes
prov["tpss"].__dict__.update(prov["pbe"].__dict__)
prov["tpss"].xc = "tpss"
npts = prov["pbe"].points.shape[0]
print(f"{name} / {basis}: {n} AOs, {npts} grid points", flush=True)
rng = np.random.default_rng(0)
c = np.linalg.qr(rng.normal(size=(n, n)))[0][:, : max(1, n // 5)] * 0.3
dm = np.stack([c @ c.T, c @ c.T])
dmd = be.asarray(dm)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def kernels(p):
    ao, dao, w = p._ao, p._dao, p._w
    if p.xc == "tpss":
        (rho, grad, tau), t0 = timed(lambda: be.xc_rho_tau(ao, dao, dmd))
        (vr, vec, vt, _), t1 = timed(lambda: be.xc_functional_mgga(_nbx.XC_MGGA_CODES["tpss"], rho, grad, tau, w, p.RHO_FLOOR))
        _, t2 = timed(lambda: be.xc_vmat_tau(ao, dao, vr, vec, vt))
    else:
        (rho, grad), t0 = timed(lambda: be.xc_rho(ao, dao, dmd))
        (vr, vec, _), t1 = timed(lambda: be.xc_functional(_nbx.XC_CODES["pbe"], rho, grad, w, p.RHO_FLOOR))
        _, t2 = timed(lambda: be.xc_vmat(ao, dao, vr, vec))
    return {"rho": t0, "functional": t1, "vmat": t2}


def whole(p):
    torch.cuda.synchronize()
    t = time.perf_counter()
    p(dm)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


for p in prov.values():  # warm-up
    whole(p)
    kernels(p)
runs = {k: {"whole_ms": [], "rho": [], "functional": [], "vmat": []} for k in prov}
for _ in range(RUNS):
    for k, p in prov.items():
        runs[k]["whole_ms"].append(whole(p))
        for kk, v in kernels(p).items():
            runs[k][kk].append(v)
res = {"molecule": name, "basis": basis, "nao": int(n), "npts": int(npts), "runs": RUNS,
       "median_ms": {k: {kk: statistics.median(v) for kk, v in r.items()} for k, r in runs.items()}, "all_ms": runs}
for k, r in res["median_ms"].items():
    print(k, " ".join(f"{kk} {v:.3f} ms" for kk, v in r.items()), flush=True)
print("tpss / pbe:", " ".join(f"{kk} {res['median_ms']['tpss'][kk] / res['median_ms']['pbe'][kk]:.2f}" for kk in
                              ("whole_ms", "rho", "functional", "vmat")))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
