"""Device CCSD (nbed_amd/ccsd_gpu.py) on the embedded object of a real molecule: seconds per cycle and bytes planned.
Default: octane / 6-31G*, 4 active atoms, SPADE + concentric localisation, Huzinaga projector, HF-in-HF -- about 128
embedded MOs, 256 spin orbitals, far past the 40 of the host solver.

    python tools/time_ccsd.py [octane|water] [basis] [n_active_atoms] [max_cycle] [--triples]

``--triples``: the (T) step after the loop (from whatever amplitudes ``max_cycle`` left), its seconds against the cycle's."""
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

triples = "--triples" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != "--triples"]
name = args[0] if len(args) > 0 else "octane"
basis = args[1] if len(args) > 1 else "6-31g*"
nact = int(args[2]) if len(args) > 2 else 4
max_cycle = int(args[3]) if len(args) > 3 else 200
geom = octane_xyz() if name == "octane" else "3\n\nO 0 0 0.115\nH 0 0.754 -0.459\nH 0 -0.754 -0.459"

be = HipBackend()
cfg = NbedConfig(geometry=geom, n_active_atoms=nact, basis=basis, xc_functional="hf", convergence=1e-8, max_hf_cycles=100,
                 projector="huzinaga", localization="spade", virtual_localization="cl", max_shells=4)
t0 = time.perf_counter()
drv = nbed(cfg, provider=BuiltinHFProvider(be), backend=be, hamiltonian_format="spatial")
emb = drv.embedded_scf
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
stats = {}
cc = ccsd_gpu.solve_spatial(spatial, occupied, conv_tol=1e-8, max_cycle=max_cycle, backend=be, stats=stats, triples=triples)
torch.cuda.synchronize()
t3 = time.perf_counter() - stats.get("triples_seconds", 0.0)
cyc = np.array(stats["cycle_seconds"])
plan = stats["plan"]
print(f"CCSD: {stats['nocc']} occupied + {stats['nvir']} virtual spin orbitals, {cc.iterations} cycles, converged={cc.converged}, "
      f"E_corr = {cc.e_corr:.10f}, E_tot = {cc.e_tot:.10f}")
print(f"total {t3 - t2:.2f} s (blocks + MP2 start {t3 - t2 - cyc.sum():.2f} s); per cycle: median {np.median(cyc) * 1e3:.1f} ms, "
      f"first {cyc[0] * 1e3:.1f} ms, min {cyc.min() * 1e3:.1f} ms")
print("bytes planned: " + ", ".join(f"{k} {v / 1e9:.2f} GB" for k, v in plan.items())
      + f"; peak allocated by torch {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
if triples:
    tplan = stats["triples_plan"]
    print(f"(T): E_T = {cc.e_t:.10f}, {stats['triples']} triples, {stats['triples_batch']} cubes in flight, "
          f"{stats['triples_seconds']:.2f} s = {stats['triples_seconds'] / np.median(cyc):.1f} CCSD cycles")
    print("(T) bytes planned: " + ", ".join(f"{k} {v / 1e9:.2f} GB" for k, v in tplan.items()))
