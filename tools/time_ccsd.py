"""Device CCSD (nbed_amd/ccsd_gpu.py) on the embedded object of a real molecule: seconds per cycle and bytes planned.
Default: octane / 6-31G*, 4 active atoms, SPADE + concentric localisation, Huzinaga projector, HF-in-HF -- about 128
embedded MOs, 256 spin orbitals, far past the 40 of the host solver.

    python tools/time_ccsd.py [octane|water] [basis] [n_active_atoms] [max_cycle] [--triples] [--density] [--json FILE]

``--triples``: the (T) step after the loop (from whatever amplitudes ``max_cycle`` left), its seconds against the cycle's.
``--density``: the Lambda loop and the one-particle density after the amplitude loop (``max_cycle`` bounds either loop):
median seconds of a Lambda cycle against an amplitude cycle of the same run, each without its first (warm-up) cycle, and
the bytes the plan adds.  ``--json FILE``: the numbers printed, as one JSON object."""
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from molecules import octane_xyz  # noqa: E402
from nbed_amd import NbedConfig, ccsd_gpu, nbed  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402
from nbed_amd.driver import BuiltinHFProvider  # noqa: E402
from nbed_amd.ham_builder import HamiltonianBuilder  # noqa: E402

argv = sys.argv[1:]
json_path = None
if "--json" in argv:
    json_path = argv[argv.index("--json") + 1]
    del argv[argv.index("--json"):argv.index("--json") + 2]
triples, density = "--triples" in argv, "--density" in argv
args = [a for a in argv if a not in ("--triples", "--density")]
name = args[0] if len(args) > 0 else "octane"
basis = args[1] if len(args) > 1 else "6-31g*"
nact = int(args[2]) if len(args) > 2 else 4
max_cycle = int(args[3]) if len(args) > 3 else 200
geom = octane_xyz() if name == "octane" else "3\n\nO 0 0 0.115\nH 0 0.754 -0.459\nH 0 -0.754 -0.459"

be = HipBackend()
cfg = NbedConfig(geometry=geom, n_active_atoms=max(nact, 1), basis=basis, xc_functional="hf", convergence=1e-8, max_hf_cycles=100,
                 projector="huzinaga", localization="spade", virtual_localization="cl", max_shells=4)
t0 = time.perf_counter()
if nact > 0:
    drv = nbed(cfg, provider=BuiltinHFProvider(be), backend=be, hamiltonian_format="spatial")
    emb = drv.embedded_scf
else:  # n_active_atoms = 0: no embedding, the molecule's own Hartree-Fock object (water / cc-pVDZ: 48 spin orbitals)
    emb = BuiltinHFProvider(be).global_hf(cfg)
torch.cuda.synchronize()
t1 = time.perf_counter()
n = np.asarray(emb.mo_coeff).shape[-1]
print(f"{name}/{basis}: embedded object of {n} MOs ({2 * n} spin orbitals), embedding {t1 - t0:.2f} s", flush=True)
mo_occ = np.asarray(emb.mo_occ)
if mo_occ.ndim == 1:
    mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
occupied = [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]
spatial = HamiltonianBuilder(emb, emb.energy_nuc(), backend=be).build_spatial_device()
torch.cuda.synchronize()
t2 = time.perf_counter()
print(f"spatial Hamiltonian blocks on the device: {t2 - t1:.2f} s", flush=True)
torch.cuda.reset_peak_memory_stats()
held_before = torch.cuda.memory_allocated()  # (the embedding driver's tensors and the spatial blocks: inside every peak below)
stats = {}
cc = ccsd_gpu.solve_spatial(spatial, occupied, conv_tol=1e-8, max_cycle=max_cycle, backend=be, stats=stats, triples=triples,
                            density=density)
torch.cuda.synchronize()
lam = np.array(stats.get("lambda_cycle_seconds", []))
t3 = time.perf_counter() - stats.get("triples_seconds", 0.0) - lam.sum() - stats.get("lambda_setup_seconds", 0.0)
cyc = np.array(stats["cycle_seconds"])
plan = stats["plan"]
print(f"CCSD: {stats['nocc']} occupied + {stats['nvir']} virtual spin orbitals, {cc.iterations} cycles, converged={cc.converged}, "
      f"E_corr = {cc.e_corr:.10f}, E_tot = {cc.e_tot:.10f}")
print(f"total {t3 - t2:.2f} s (blocks + MP2 start {t3 - t2 - cyc.sum():.2f} s); per cycle: median {np.median(cyc) * 1e3:.1f} ms, "
      f"first {cyc[0] * 1e3:.1f} ms, min {cyc.min() * 1e3:.1f} ms")
print("bytes planned: " + ", ".join(f"{k} {v / 1e9:.2f} GB" for k, v in plan.items())
      + f"; peak allocated by torch {torch.cuda.max_memory_allocated() / 1e9:.2f} GB, of which {held_before / 1e9:.2f} GB "
      "were held before the solver started")
if triples:
    tplan = stats["triples_plan"]
    print(f"(T): E_T = {cc.e_t:.10f}, {stats['triples']} triples, {stats['triples_batch']} cubes in flight, "
          f"{stats['triples_seconds']:.2f} s = {stats['triples_seconds'] / np.median(cyc):.1f} CCSD cycles")
    print("(T) bytes planned: " + ", ".join(f"{k} {v / 1e9:.2f} GB" for k, v in tplan.items()))
record = {"molecule": name, "basis": basis, "spin_orbitals": 2 * n, "nocc": stats["nocc"], "nvir": stats["nvir"],
          "iterations": cc.iterations, "converged": cc.converged, "cycle_ms_median": float(np.median(cyc[1:] if len(cyc) > 1 else cyc) * 1e3),
          "plan_bytes": {k: int(v) for k, v in plan.items()}, "peak_allocated_bytes": int(torch.cuda.max_memory_allocated()),
          "held_before_solver_bytes": int(held_before)}
if density:
    warm_t, warm_l = (cyc[1:] if len(cyc) > 1 else cyc), (lam[1:] if len(lam) > 1 else lam)
    ratio = float(np.median(warm_l) / np.median(warm_t))
    occs = cc.natural_occupations()
    print(f"Lambda: {cc.lambda_iterations} cycles, converged={cc.lambda_converged}, intermediates {stats['lambda_setup_seconds'] * 1e3:.1f} ms; "
          f"per cycle after the first: median {np.median(warm_l) * 1e3:.1f} ms against {np.median(warm_t) * 1e3:.1f} ms of an "
          f"amplitude cycle: ratio {ratio:.2f}; the plan adds {plan['lambda'] / 1e9:.3f} GB; max |cross-spin| "
          f"{stats['lambda_cross_spin']:.1e}; natural occupations {occs[0]:.6f} .. {occs[-1]:.2e}")
    record.update(lambda_iterations=cc.lambda_iterations, lambda_converged=cc.lambda_converged,
                  lambda_cycle_ms_median=float(np.median(warm_l) * 1e3), lambda_setup_ms=stats["lambda_setup_seconds"] * 1e3,
                  lambda_to_amplitude_cycle_ratio=ratio, lambda_extra_bytes=int(plan["lambda"]),
                  lambda_cycle_ms=[float(x * 1e3) for x in lam], cycle_ms=[float(x * 1e3) for x in cyc])
if json_path:
    with open(json_path, "w") as fh:
        json.dump(record, fh, indent=1)
