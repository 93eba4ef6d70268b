"""The four-index transform from a factor of the integrals (HipBackend.ao2mo_factor): wall time up
to a final synchronise as the median of five runs after one warm-up, the routes alternating within one process.

    python tools/time_ao2mo_factor.py stage1 [out.json]   fused stage 1 against half="gemm", random inputs, two spin sets,
                                                          (N, n, naux) = (148, 148, 1203) and (220, 60, 1794); the whole
                                                          ao2mo_factor with either stage 1 beside it
    python tools/time_ao2mo_factor.py route [out.json]    octane / 6-31G*, tol = 1e-6, the three blocks of n = N orbitals:
                                                          eri_cholesky + ao2mo_factor against the dense route
                                                          eri + eri_pack_rs + ao2mo_pair_sym (x 2); peak device memory
    python tools/time_ao2mo_factor.py nbed [out.json]     nbed(config) on octane / 6-31G* (4 active atoms, SPADE + CL, both
                                                          projectors, spatial Hamiltonians): eri_engine="cholesky"
                                                          (tol = 1e-6) against "device"; time and peak device memory"""
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import torch  # noqa: E402

from molecules import octane_xyz  # noqa: E402
from nbed_amd import NbedConfig, integrals, nbed  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402
from nbed_amd.driver import BuiltinHFProvider  # noqa: E402

RUNS = 5
mode = sys.argv[1] if len(sys.argv) > 1 else "stage1"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
be = HipBackend()


def timed(fn):
    """(seconds, peak device bytes above what was allocated before) of one call, synchronised on both sides."""
    be.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    be.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt, torch.cuda.max_memory_allocated() - base


def alternate(routes):
    """{name: (median seconds, all seconds, largest peak bytes)}: round 0 warms every route up."""
    secs = {k: [] for k in routes}
    peak = {k: 0 for k in routes}
    for rnd in range(RUNS + 1):
        for name, fn in routes.items():
            be.release_workspaces()
            dt, pk = timed(fn)
            if rnd:
                secs[name].append(dt)
                peak[name] = max(peak[name], pk)
    return {k: {"seconds": statistics.median(v), "seconds_all": v, "peak_bytes": peak[k]} for k, v in secs.items()}


def show(name, row):
    v = row["seconds_all"]
    print(f"  {name:<28} {row['seconds'] * 1e3:9.2f} ms ({min(v) * 1e3:.2f} .. {max(v) * 1e3:.2f}), peak {row['peak_bytes'] / 1e9:.3f} GB",
          flush=True)


result = {"mode": mode, "runs": RUNS}
if mode == "stage1":
    result["shapes"] = []
    for big_n, n, naux in ((148, 148, 1203), (220, 60, 1794)):
        g = torch.Generator(device="cpu").manual_seed(big_n)
        b = torch.randn((naux, big_n, big_n), dtype=torch.float64, generator=g)
        b = be.asarray(0.5 * (b + b.transpose(1, 2)))
        ca, cb = (be.asarray(torch.randn((big_n, n), dtype=torch.float64, generator=g)) for _ in range(2))
        print(f"N = {big_n}, n = {n}, naux = {naux}, two spin sets", flush=True)
        rows = alternate({
            "stage 1 fused": lambda: be.ao2mo_factor_half(b, ca, cb, half="fused"),
            "stage 1 gemm": lambda: be.ao2mo_factor_half(b, ca, cb, half="gemm"),
            "ao2mo_factor fused": lambda: be.ao2mo_factor(b, ca, cb, half="fused"),
            "ao2mo_factor gemm": lambda: be.ao2mo_factor(b, ca, cb, half="gemm"),
        })
        for k, row in rows.items():
            show(k, row)
        diff = float((be.ao2mo_factor_half(b, ca, cb, half="fused") - be.ao2mo_factor_half(b, ca, cb, half="gemm")).abs().max())
        npair = n * (n + 1) // 2
        result["shapes"].append({"nao": big_n, "n": n, "naux": naux, "nset": 2, "stage1_flop": 2 * 2 * naux * big_n * n * (big_n + n),
                                 "stage2_flop": 3 * 2 * naux * npair * npair, "max_abs_fused_minus_gemm": diff, "routes": rows})
        del b, ca, cb
elif mode == "route":
    tol = 1e-6
    bs = integrals.Basis(integrals.parse_geometry(octane_xyz()), "6-31g*")
    n = bs.nao
    g = torch.Generator(device="cpu").manual_seed(n)
    ca, cb = (be.asarray(torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, generator=g))[0]) for _ in range(2))
    print(f"octane / 6-31G*: {n} AOs, n = {n} orbitals per spin, tol = {tol:g}", flush=True)

    def factor_route():
        return be.ao2mo_factor(be.eri_cholesky(bs, tol=tol), ca, cb)

    def dense_route():  # HamiltonianBuilder._two_body_device on the dense tensor
        rs = be.eri_pack_rs(be.eri(bs), n)
        aaaa, aabb = be.ao2mo_pair_sym(rs, ca, ca, ca, cb, cb, rs_packed=True)
        return aaaa, be.ao2mo_pair_sym(rs, cb, cb, cb, rs_packed=True), aabb

    fac = be.eri_cholesky(bs, tol=tol)
    rank = int(fac.shape[0])
    rows = alternate({
        "factor: cholesky + ao2mo": factor_route,
        "dense: eri + pack + ao2mo": dense_route,
        "factor: eri_cholesky alone": lambda: be.eri_cholesky(bs, tol=tol),
        "factor: ao2mo_factor alone": lambda: be.ao2mo_factor(fac, ca, cb),
    })
    for k, row in rows.items():
        show(k, row)
    got, want = factor_route(), dense_route()
    diff = max(float((x - y).abs().max()) for x, y in zip(got, want))
    print(f"  rank {rank}; max |factor route - dense route| over the three blocks = {diff:.3e}")
    result.update({"molecule": "octane", "basis": "6-31g*", "nao": n, "n": n, "tol": tol, "rank": rank, "routes": rows,
                   "max_abs_factor_minus_dense": diff, "output_bytes": 3 * 8 * n ** 4})
elif mode == "nbed":
    tol = 1e-6
    cfg = NbedConfig(geometry=octane_xyz(), n_active_atoms=4, basis="6-31g*", xc_functional="b3lyp", convergence=1e-8,
                     max_hf_cycles=100, max_dft_cycles=100, projector="both", localization="spade", virtual_localization="cl",
                     max_shells=4)
    energies = {}

    def run(engine):
        def go():
            prov = BuiltinHFProvider(be, xc_grid=(96, 28), eri_engine=engine, cholesky_tol=tol)
            drv = nbed(cfg, provider=prov, backend=be, hamiltonian_format="spatial")
            energies[engine] = {"e_ks": float(drv._global_ks.e_tot), "mu_e_rhf": float(drv.mu["e_rhf"]),
                                "huzinaga_e_rhf": float(drv.huzinaga["e_rhf"]), "n_mo": int(drv.mu["scf"].mo_coeff.shape[-1])}
            return None
        return go

    rows = alternate({"nbed cholesky": run("cholesky"), "nbed device": run("device")})
    for k, row in rows.items():
        show(k, row)
    print("  ", energies)
    result.update({"molecule": "octane", "basis": "6-31g*", "tol": tol, "routes": rows, "energies": energies,
                   "abs_energy_differences": {k: abs(energies["cholesky"][k] - energies["device"][k])
                                              for k in ("e_ks", "mu_e_rhf", "huzinaga_e_rhf")}})
else:
    raise SystemExit(__doc__)
print(json.dumps(result))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
