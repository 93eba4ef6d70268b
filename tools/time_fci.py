"""Device FCI (nbed_amd/fci_gpu.py): seconds per sigma split into gather / GEMM / scatter with the bytes and flops of
each phase, and Davidson iterations to convergence, for the global Hamiltonian of water / 6-31G (13 orbitals, (5, 5),
1.66e6 determinants) and one larger synthetic sector (default n = 14, (6, 6), 9.0e6 determinants).

    python tools/time_fci.py [n] [n_alpha] [n_beta] [chunk_rows]

With ``--rdm``: water / 6-31G only, medians of five after a warm-up, in one process: seconds per sigma (the yardstick),
per ``rdm12`` split into gather / GEMM / finish, per direct ``rdm1``, and the GEMM with one slab against the default.

    python tools/time_fci.py --rdm"""
import sys
import time
from math import comb

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fci_reference import synthetic  # noqa: E402
from nbed_amd import NbedConfig, fci_gpu  # noqa: E402
from nbed_amd.backend import HipBackend  # noqa: E402
from nbed_amd.driver import BuiltinHFProvider  # noqa: E402
from nbed_amd.ham_builder import HamiltonianBuilder  # noqa: E402

RDM = "--rdm" in sys.argv
args = [a for a in sys.argv[1:] if a != "--rdm"]
n_syn = int(args[0]) if len(args) > 0 else 14
na_syn = int(args[1]) if len(args) > 1 else 6
nb_syn = int(args[2]) if len(args) > 2 else 6
chunk_rows = int(args[3]) if len(args) > 3 else None
WATER = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"

be = HipBackend()


def time_sigma(label, spatial, nelec, repeats=3):
    sb = fci_gpu.SigmaBuilder(be, spatial, nelec, space=12, chunk_rows=chunk_rows)
    n, g, ndet = sb.n, 2 * sb.n * sb.n, sb.ndet
    c = be.asarray(np.random.default_rng(0).standard_normal((sb.n_a, sb.n_b)))
    out = be.empty((sb.n_a, sb.n_b))
    sb(c, out)  # (first launches, allocator)
    be.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        sb(c, out)
    be.synchronize()
    whole = (time.perf_counter() - t0) / repeats
    sb.seconds = {"gather": 0.0, "gemm": 0.0, "scatter": 0.0}
    for _ in range(repeats):
        sb(c, out)
    sec = {k: v / repeats for k, v in sb.seconds.items()}
    sb.seconds = None
    s_a, s_b = sb.na * (n - sb.na + 1), sb.nb * (n - sb.nb + 1)
    # gather: writes D, reads the s_a + s_b source elements of every determinant and the beta table
    gather_bytes = 8 * (g + 1) * ndet + 8 * (s_a + 1) * ndet + 4 * n * n * ndet
    gemm_flops = 2 * g * (g + 1) * ndet
    gemm_bytes = 8 * (2 * g + 1) * ndet
    # scatter: per chunk every output element is touched; it reads the alpha rows that hit, all beta rows and the table
    scatter_bytes = 8 * (s_a + n * n) * ndet + 4 * n * n * ndet + 8 * 2 * ndet * sb.plan["chunks"]
    print(f"{label}: n = {n}, ({sb.na}, {sb.nb}), {ndet} determinants, {sb.plan['chunks']} chunk(s) of {sb.rows} alpha rows; "
          f"planned " + ", ".join(f"{k} {sb.plan[k] / 1e9:.2f} GB" for k in ("vectors", "work", "chunk", "tables", "total")))
    print(f"  sigma {whole * 1e3:.1f} ms (phases synchronised one by one: gather {sec['gather'] * 1e3:.1f} ms, "
          f"{gather_bytes / 1e9:.1f} GB, {gather_bytes / sec['gather'] / 1e12:.2f} TB/s; GEMM {sec['gemm'] * 1e3:.1f} ms, "
          f"{gemm_flops / 1e12:.2f} TFLOP, {gemm_flops / sec['gemm'] / 1e12:.1f} TFLOP/s, {gemm_bytes / 1e9:.1f} GB; "
          f"scatter {sec['scatter'] * 1e3:.1f} ms, {scatter_bytes / 1e9:.1f} GB, {scatter_bytes / sec['scatter'] / 1e12:.2f} TB/s)",
          flush=True)
    del sb, c, out
    torch.cuda.empty_cache()


def time_solve(label, spatial, nelec, occupied, conv_tol):
    stats = {}
    be.synchronize()
    t0 = time.perf_counter()
    res = fci_gpu.solve_spatial(spatial, nelec, occupied, conv_tol=conv_tol, backend=be, chunk_rows=chunk_rows, stats=stats)
    be.synchronize()
    t1 = time.perf_counter()
    it = np.array(stats["iteration_seconds"]) if stats["iteration_seconds"] else np.array([0.0])
    print(f"  Davidson to |r| < {conv_tol:g}: {res.iterations} iterations, converged={res.converged}, E = {res.e_tot:.10f}, "
          f"|r| = {res.residual_norm:.2e}, {t1 - t0:.2f} s in all, median iteration {np.median(it) * 1e3:.1f} ms", flush=True)
    torch.cuda.empty_cache()


def median_of_five(fn):
    fn()  # (first launches, allocator)
    be.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        fn()
        be.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def time_rdm(label, spatial, nelec):
    sb = fci_gpu.SigmaBuilder(be, spatial, nelec, space=1, chunk_rows=chunk_rows)
    n, ndet, g1 = sb.n, sb.ndet, 2 * sb.n * sb.n + 1
    c = be.asarray(np.random.default_rng(0).standard_normal((sb.n_a, sb.n_b)))
    c /= float(c.norm())
    out = be.empty((sb.n_a, sb.n_b))
    t_sigma = median_of_five(lambda: sb(c, out))
    del sb, out
    torch.cuda.empty_cache()
    print(f"{label}: n = {n}, {nelec}, {ndet} determinants", flush=True)
    print(f"  sigma {t_sigma * 1e3:.2f} ms", flush=True)
    gemm = {}
    for slabs in (None, 1):
        rb = fci_gpu.RdmBuilder(be, n, nelec, chunk_rows=chunk_rows, slabs=slabs, held=8 * ndet)
        whole = median_of_five(lambda: rb.rdm12(c))
        phases = {"gather": [], "gemm": [], "finish": []}
        for _ in range(5):
            rb.seconds = {"gather": 0.0, "gemm": 0.0, "finish": 0.0}
            rb.rdm12(c)
            for k, v in rb.seconds.items():
                phases[k].append(v)
        rb.seconds = None
        sec = {k: float(np.median(v)) for k, v in phases.items()}
        gemm[rb.slabs] = sec["gemm"]
        flops = 2 * g1 * g1 * ndet
        print(f"  rdm12, {rb.slabs} slab(s), {rb.plan['chunks']} chunk(s): {whole * 1e3:.2f} ms = {whole / t_sigma:.2f} sigma "
              f"(phases synchronised one by one: gather {sec['gather'] * 1e3:.2f} ms, GEMM {sec['gemm'] * 1e3:.2f} ms, "
              f"{flops / sec['gemm'] / 1e12:.1f} TFLOP/s, finish {sec['finish'] * 1e3:.2f} ms)", flush=True)
        if slabs is None:
            t_rdm1 = median_of_five(lambda: rb.rdm1(c))
            print(f"  direct rdm1 {t_rdm1 * 1e3:.2f} ms = {t_rdm1 / t_sigma:.2f} sigma", flush=True)
        del rb
        torch.cuda.empty_cache()
    print("  GEMM by slabs: " + ", ".join(f"{k}: {v * 1e3:.2f} ms" for k, v in gemm.items()), flush=True)


cfg = NbedConfig(geometry=WATER, n_active_atoms=1, basis="6-31g", xc_functional="hf", convergence=1e-10)
hf = BuiltinHFProvider(be).global_hf(cfg)
spatial = HamiltonianBuilder(hf, hf.energy_nuc(), backend=be).build_spatial_device()
mo_occ = np.asarray(hf.mo_occ)
if mo_occ.ndim == 1:
    mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
occupied = [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]
nelec = tuple(int(x) for x in hf.mol.nelec)
if RDM:
    time_rdm("water / 6-31G", spatial, nelec)
    sys.exit(0)
time_sigma("water / 6-31G", spatial, nelec)
time_solve("water / 6-31G", spatial, nelec, occupied, 1e-8)

ham = synthetic(n_syn, 7)
assert comb(n_syn, nb_syn) <= fci_gpu.MAX_ROW
time_sigma("synthetic", ham, (na_syn, nb_syn))
time_solve("synthetic", ham, (na_syn, nb_syn), None, 1e-8)
