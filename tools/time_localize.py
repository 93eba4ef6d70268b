"""One Pipek-Mezey ('lowdin') and one Boys call on octane / 6-31G* (both spins in one launch), timed with HIP
events, and the numpy restatement of the same sweeps (tests/loc_reference.py) on the host for comparison."""

import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import loc_reference as ref  # noqa: E402
from molecules import octane_xyz  # noqa: E402
from nbed_amd import NbedConfig  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402
from nbed_amd.driver import BuiltinHFProvider  # noqa: E402


def timed(fn, reps=5):
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return out, float(np.median(ms)), min(ms)


be = HipBackend()
cfg = NbedConfig(geometry=octane_xyz(), n_active_atoms=4, basis="6-31G*", xc_functional="hf", convergence=1e-10,
                 max_hf_cycles=100, max_dft_cycles=100)
hf = BuiltinHFProvider(be).global_hf(cfg)
nocc = int(np.count_nonzero(hf.mo_occ[0]))
c = np.array([np.asarray(hf.mo_coeff[x])[:, :nocc] for x in (0, 1)])
s = np.asarray(hf.get_ovlp())
w, v = np.linalg.eigh(s)
x = np.einsum("pq,bqi->bpi", (v * np.sqrt(w)) @ v.T, c)
r = hf.mol.intor_symmetric("int1e_r", comp=3)
q = np.array([ref.boys_matrices(c[b], r) for b in range(2)])
sl = np.asarray(hf.mol.aoslice_by_atom())
offs = np.concatenate([[0], sl[:, 3]]).astype(np.int64)
x_d, q_d = be.asarray(x), be.asarray(q)
print(f"octane / 6-31G*: nao = {x.shape[1]}, n_occ = {nocc}, natm = {len(offs) - 1}, batch = 2 (alpha, beta)")
(u, sw, f), med, best = timed(lambda: be.localize_pm(x_d, None, offs))
print(f"nbx_loc_pm   ('lowdin', X = Y): {med:.3f} ms per call (min {best:.3f}), sweeps {list(sw)}, f {f[0]:.12f}")
(u, sw, f), med, best = timed(lambda: be.localize_boys(q_d))
print(f"nbx_loc_boys                  : {med:.3f} ms per call (min {best:.3f}), sweeps {list(sw)}, f {f[0]:.12f}")
t = time.perf_counter()
_, sw_ref, f_ref, _ = ref.localize_pm(x[0], None, offs)
t_pm = time.perf_counter() - t
t = time.perf_counter()
_, swb_ref, fb_ref, _ = ref.localize_boys(q[0])
t_boys = time.perf_counter() - t
cores = len(os.sched_getaffinity(0))
print(f"numpy restatement, one spin, {cores} host cores: PM {t_pm * 1e3:.1f} ms ({sw_ref} sweeps), "
      f"Boys {t_boys * 1e3:.1f} ms ({swb_ref} sweeps)")
