"""GPU-backed SCF objects implementing the protocol the reference drives PySCF through.

The reference never touches integrals itself: it calls ``get_ovlp / get_hcore / get_veff /
get_j / get_occ / make_rdm1 / get_fock / energy_tot / kernel`` on a PySCF ``scf.UHF``
(nbed/driver.py:241, call sites listed in SURVEY.md section 8b).  ``GpuUHF`` offers the same
methods (numpy in, numpy out, same argument meaning) with the arithmetic in libnbx:

* ``get_jk`` / ``get_veff``  -> ``nbx_jk_dense`` on the device-resident (pq|rs)
* ``make_rdm1`` / ``eig``    -> ``nbx_gemm`` / ``nbx_eigh``
* ``kernel``                -> PySCF's ``scf.hf.kernel`` control flow (CDIIS, conv_check),
                               used by the mu-shift embedding (nbed/driver.py:533)

and device-level twins (``*_device``) that keep everything in HBM for ``huzinaga_scf``.
The ERI may be sharded by its first AO index over the ranks of a process group
(``nbed_amd.dist.Shards``); the J/K row slabs are then all-gathered once per call.
"""

from __future__ import annotations

import logging
import os

import numpy as np

from ..backend import get_backend
from ..dist import Shards
from .pyscf_compat import RHF, RKS, UHF, UKS


logger = logging.getLogger(__name__)


class _TrackedCycleRejected(RuntimeError):
    """A cycle solved by unguarded refinement did not pass its acceptance test: kernel() is repeated guarded."""


class Mole:
    """The ``gto.Mole`` attributes the path reads."""

    def __init__(self, nao, nelec, ao_slices=None, e_nuc=0.0, atom=None, basis=None, charge=0, dipole=None):
        """``dipole``: a callable returning the (3, nao, nao) dipole matrices of the geometry, unit and basis of the
        overlap this molecule goes with (called on first use: only Boys localisation asks for them)."""
        self.nao = int(nao)
        self.atom = atom
        self.basis = basis
        self.charge = charge
        self._ao_slices = ao_slices
        self._e_nuc = float(e_nuc)
        self._dipole = dipole
        self.nelec = (int(nelec[0]), int(nelec[1]))

    @property
    def nelec(self):
        return self._nelec

    @nelec.setter
    def nelec(self, value):
        self._nelec = (int(value[0]), int(value[1]))
        self.nelectron = self._nelec[0] + self._nelec[1]
        self.spin = self._nelec[0] - self._nelec[1]

    def nao_nr(self):
        return self.nao

    def aoslice_by_atom(self):
        """(natm, 4) int array [shell0, shell1, ao0, ao1]."""
        if self._ao_slices is None:
            return np.array([[0, 1, 0, self.nao]])
        return np.asarray(self._ao_slices)

    def energy_nuc(self):
        return self._e_nuc

    def intor(self, intor, comp=None, **kwargs):
        """``gto.Mole.intor`` for the one integral the path asks a molecule for: "int1e_r" (origin 0)."""
        name = str(intor)
        for suffix in ("_sph", "_cart"):
            name = name.removesuffix(suffix)
        if name != "int1e_r":
            raise NotImplementedError(f"the built-in molecule has no integral {intor!r} (only 'int1e_r')")
        if self._dipole is None:
            raise NotImplementedError("this molecule has no source of dipole integrals (int1e_r): it comes from "
                                      "neither PySCF nor the built-in integral provider")
        return np.array(self._dipole(), dtype=np.float64)

    def intor_symmetric(self, intor, comp=None, **kwargs):
        return self.intor(intor, comp, **kwargs)


# Below this many basis functions the packed J/K kernel has no edge over the symmetric one (both
# are launch bound) and the packed copy would only cost memory.  The symmetric kernel needs an even
# N, though: odd sizes would drop to the plain dense kernel (4x the bytes), so they go packed
# (zero-padded to the next size the kernel has an instance for) from PACKED_JK_MIN_NAO_ODD on.
PACKED_JK_MIN_NAO = 100
PACKED_JK_MIN_NAO_ODD = 48


def _sign_fix(c: np.ndarray) -> np.ndarray:
    """PySCF ``hf.eig``: make each eigenvector's largest-|component| positive."""
    idx = np.argmax(np.abs(c), axis=0)
    c[:, c[idx, np.arange(c.shape[1])] < 0] *= -1
    return c


class _GpuSCF:
    """Shared machinery: device-resident S, hcore, (pq|rs) (possibly a row slab)."""

    def __init__(self, mol: Mole, ovlp, hcore, eri=None, backend=None, shards: Shards | None = None,
                 eri_packed=None, eri_factor=None):
        """``eri_packed``: the packed J/K copy of the same slab (``eri_packed_device()`` of another
        object over the same integrals), so that objects sharing a molecule share it.
        ``eri_factor``: instead of the tensor, a device (naux, N, N) factor with (pq|rs) = sum_L B[L, p, q] B[L, r, s]
        (``HipBackend.eri_cholesky``); J/K then come from ``backend.jk_factor`` and the loops run step by step, since the
        one-call-per-cycle paths read the tensor.  Single rank only."""
        self.be = backend if backend is not None else get_backend()
        self.mol = mol
        self._s_h = np.asarray(ovlp, dtype=np.float64)
        self._h_h = np.asarray(hcore, dtype=np.float64)
        self._s_d = self.be.asarray(self._s_h)
        self._h_d = self.be.asarray(self._h_h)
        nao = self._s_h.shape[0]
        self.shards = shards if shards is not None else Shards(nao)
        if eri is not None:
            eri = self.be.asarray(eri)
            if tuple(eri.shape) != (self.shards.size, nao, nao, nao):
                raise ValueError(
                    f"ERI slab has shape {tuple(eri.shape)}, expected {(self.shards.size, nao, nao, nao)}"
                )
        if eri_factor is not None:
            if eri is not None or eri_packed is not None:
                raise ValueError("eri_factor excludes eri and eri_packed: give the tensor or its factor, not both")
            if self.shards.world != 1 or self.shards.size != nao:
                raise ValueError("eri_factor is single rank only: the decomposition is not split over row slabs")
            eri_factor = self.be.asarray(eri_factor)
            if eri_factor.ndim != 3 or tuple(eri_factor.shape[1:]) != (nao, nao):
                raise ValueError(f"eri_factor has shape {tuple(eri_factor.shape)}, expected (naux, {nao}, {nao})")
            if not hasattr(self.be, "jk_factor"):
                raise ValueError("this backend has no jk_factor: it cannot run on a factor of the integrals")
        self._eri_d = eri
        self._eri_factor_d = eri_factor
        self._eri_packed_d = eri_packed  # 4-fold packed copy of the slab for the J/K kernel, made on first use
        self._x_d = None  # S^-1/2, built on first use
        self.mo_coeff = None
        self.mo_occ = None
        self.mo_energy = None
        self.e_tot = None
        self.converged = False
        self.max_cycle = 50
        self.conv_tol = 1e-9
        self.max_memory = 4000
        self.verbose = 1
        self.scf_summary = {}
        self.cycles = 0

    # ---- protocol: integrals
    def get_ovlp(self, mol=None):
        return self._s_h

    def get_hcore(self, mol=None):
        return self._h_h

    def energy_nuc(self):
        return self.mol.energy_nuc()

    @property
    def nelec(self):
        return self.mol.nelec

    # ---- device-level access for the fused paths
    def eri_device(self):
        if self._eri_d is None:
            raise ValueError("this SCF object was built without two-electron integrals")
        return self._eri_d

    def eri_factor_device(self):
        """The device (naux, N, N) factor this object was built on (``eri_factor=``), or None: what
        ``HamiltonianBuilder`` transforms instead of ``eri_device()``."""
        return self._eri_factor_d

    def x_device(self):
        if self._x_d is None:
            # S^-1/2 (nbed/scf/huzinaga_scf.py:128) by GEMMs where the backend has the iteration
            fast = getattr(self.be, "sym_pow_fast", None)
            self._x_d = fast(self._s_d, -0.5, self._s_h) if fast is not None else self.be.sym_pow(self._s_d, -0.5)
        return self._x_d

    def eri_packed_device(self):
        """This rank's slab in the packed tile format of nbx_jk_packed (q <= p, s <= r: a quarter of
        the dense bytes; PySCF holds ``mf._eri`` packed too), made once -- the integrals are
        constant over the SCF.  None where the packed kernel does not apply."""
        be = self.be
        nao = self._s_h.shape[0]
        if self._eri_packed_d is None and self._eri_d is not None and hasattr(be, "jk_packed"):
            if nao >= (PACKED_JK_MIN_NAO_ODD if nao % 2 else PACKED_JK_MIN_NAO) and be.jk_packed_supported(nao):
                self._eri_packed_d = be.eri_pack(self._eri_d, nao, self.shards.lo, self.shards.hi)
        return self._eri_packed_d

    # the rs-packed copy is 4 N^4 bytes: kept with the object only while that is small beside HBM
    ERI_RS_CACHE_MAX_BYTES = 32 << 30

    def eri_rs_device(self):
        """(pq|rs) with the pairs (r, s <= r) packed -- the input form of the four-index transform's
        quarters 1-2 (nbx_eri_pack_rs; PySCF's ao2mo takes "s2kl" input the same way).  Made once per
        molecule and kept: both Hamiltonian builds of a projector="both" run (nbed/driver.py:869,893)
        reuse it.  None when it does not apply (row-slab object, backend without it, too large)."""
        be = self.be
        nao = self._s_h.shape[0]
        if self._eri_factor_d is not None:
            return None
        shared = getattr(self, "_eri_shared", None)  # set by a provider whose objects share one molecule
        if getattr(self, "_eri_rs_d", None) is None and shared is not None:
            self._eri_rs_d = shared.get("rs")
        if getattr(self, "_eri_rs_d", None) is None:
            self._eri_rs_d = None
            whole = self.shards.world == 1 and self._eri_d is not None
            if whole and hasattr(be, "eri_pack_rs") and 4 * nao**4 <= self.ERI_RS_CACHE_MAX_BYTES:
                self._eri_rs_d = be.eri_pack_rs(self._eri_d, nao)
                if shared is not None:
                    shared["rs"] = self._eri_rs_d
        return self._eri_rs_d

    def jk_device(self, dm_d):
        """(1+ndm, N, N) on device: J(sum dm), K(dm[x]).  The packed / symmetric kernels read only the
        tiles q <= p of this rank's slab and return full-size partial matrices, summed over ranks
        by one all-reduce; a backend without them computes plain row slabs and all-gathers them."""
        be, sh = self.be, self.shards
        if self._eri_factor_d is not None:
            return be.jk_factor(self._eri_factor_d, dm_d)
        packed = self.eri_packed_device()
        if packed is not None:
            return sh.all_reduce(be, be.jk_packed(packed, dm_d, sh.lo, sh.hi))
        if hasattr(be, "jk_sym"):
            return sh.all_reduce(be, be.jk_sym(self.eri_device(), dm_d, sh.lo, sh.hi))
        slab = be.jk(self.eri_device(), dm_d, sh.lo, sh.hi)
        return sh.all_gather(be, slab, axis=1)

    def fused_fock_available(self, hv_d) -> bool:
        sh = self.shards
        single = sh.world == 1 and not sh.force_collective
        return (self.eri_packed_device() is not None and single and hasattr(self.be, "jk_packed_fock")
                and hv_d.dim() == 3)

    def dts_device(self):
        """The Dtot' table the packed J/K build multiplies the staged tiles with; a loop that calls
        ``huz_cycle_scalars_async(..., dts=this)`` on a density may pass ``dts_ready=True`` to
        ``fock_device`` for the build on that same density (one launch less).  None if the fused
        build does not apply."""
        if getattr(self, "_dts_d", None) is None:
            self._dts_d = None
            if self.eri_packed_device() is not None and hasattr(self.be, "jk_dts_new"):
                try:
                    self._dts_d = self.be.jk_dts_new(self._s_h.shape[0])
                except ValueError:  # a zero-padded size: the build prepares its own table
                    self._dts_d = None
        return self._dts_d

    def fock_device(self, dm_d, hv_d, dts_ready: bool = False):
        """(fock, vhf) = (hv + J - K[x], J - K[x]) of a two-spin density: one J/K build; on a single
        device with the packed kernel the Fock assembly rides on its reduction kernel."""
        be = self.be
        if self.fused_fock_available(hv_d):
            dts = self.dts_device() if dts_ready else None
            return be.jk_packed_fock(self.eri_packed_device(), dm_d, hv_d, dts=dts)
        return be.fock_uhf(hv_d, None, self.jk_device(dm_d))

    def _eig_device(self, fock_d, warm: dict | None = None):
        """Generalised eigenproblem F C = S C e through Loewdin orthogonalisation.  ``warm``: a
        dict carried across SCF cycles; the previous cycle's orthonormal eigenvectors kept in it
        seed the solver (GEMM refinement / few sweeps instead of a cold Jacobi solve)."""
        x = self.x_device()
        fo = self.be.gemm(self.be.gemm(x, fock_d), x)
        e, c = self.be.eigh(fo, v0=None if warm is None else warm.get("v"))
        if warm is not None:
            warm["v"] = c
        return e, self.be.gemm(x, c)


class GpuUHF(_GpuSCF, UHF):
    """Unrestricted HF over dense S, hcore, (pq|rs); arrays carry a leading spin axis."""

    # ---- J/K
    def get_jk(self, mol=None, dm=None, hermi=1):
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        jk = self.be.to_host(self.jk_device(self.be.asarray(dm.reshape(-1, *dm.shape[-2:]))))
        ndm = jk.shape[0] - 1
        # PySCF returns J per density matrix; the kernel returns J of the summed density,
        # which is what every call site of the path needs (J_a + J_b): split it only on request.
        if ndm == 1:
            return jk[0].reshape(dm.shape), jk[1].reshape(dm.shape)
        vk = jk[1:]
        vj = np.stack([self.be.to_host(self.jk_device(self.be.asarray(dm[x : x + 1])))[0] for x in range(ndm)])
        return vj, vk

    def get_j(self, mol=None, dm=None, hermi=1):
        return self.get_jk(mol, dm)[0]

    def get_veff(self, mol=None, dm=None, dm_last=0, vhf_last=0, hermi=1):
        """vhf[x] = J_a + J_b - K_x (PySCF UHF.get_veff; huzinaga_scf.py:156)."""
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        if dm.ndim == 2:
            dm = np.array((dm * 0.5, dm * 0.5))
        return self.be.to_host(self.get_veff_device(self.be.asarray(dm)))

    def get_veff_device(self, dm_d):
        jk = self.jk_device(dm_d)
        vhf = self.be.copy(jk[1:])
        # vhf[x] = J - K[x]
        self.be.axpby(1.0, jk[0], -1.0, vhf[0])
        self.be.axpby(1.0, jk[0], -1.0, vhf[1])
        return vhf

    # ---- occupations / densities
    def get_occ(self, mo_energy=None, mo_coeff=None):
        mo_energy = self.mo_energy if mo_energy is None else np.asarray(mo_energy)
        mo_occ = np.zeros_like(mo_energy)
        na, nb = self.mol.nelec
        mo_occ[0, np.argsort(mo_energy[0])[:na]] = 1
        mo_occ[1, np.argsort(mo_energy[1])[:nb]] = 1
        return mo_occ

    def make_rdm1_device(self, c_d, occ_h):
        """D[x] = (C[x] * occ[x]) C[x]^T on device."""
        scaled = self.be.scale_cols(self.be.copy(c_d), self.be.asarray(occ_h))
        return self.be.gemm(scaled, c_d, "N", "T")

    def make_rdm1(self, mo_coeff=None, mo_occ=None):
        mo_coeff = self.mo_coeff if mo_coeff is None else mo_coeff
        mo_occ = self.mo_occ if mo_occ is None else mo_occ
        return self.be.to_host(self.make_rdm1_device(self.be.asarray(np.asarray(mo_coeff)), np.asarray(mo_occ)))

    # ---- Fock / energies
    def get_fock(self, h1e=None, s1e=None, vhf=None, dm=None, cycle=-1, diis=None):
        h1e = self.get_hcore() if h1e is None else h1e
        if vhf is None:
            vhf = self.get_veff(self.mol, self.make_rdm1() if dm is None else dm)
        return np.asarray(h1e) + vhf

    def energy_elec(self, dm=None, h1e=None, vhf=None):
        """PySCF ``uhf.energy_elec`` (2-D hcore); the driver swaps in the 3-D aware one."""
        from .embedded_hcore_funcs import energy_elec

        h1e = self.get_hcore() if h1e is None else np.asarray(h1e)
        if h1e.ndim == 2:
            h1e = np.array((h1e, h1e))
        return energy_elec(self, dm, h1e, vhf)

    def energy_tot(self, dm=None, h1e=None, vhf=None):
        return self.energy_elec(dm, h1e, vhf)[0] + self.energy_nuc()

    def eig(self, fock, s=None):
        e, c = self._eig_device(self.be.asarray(np.asarray(fock)))
        e, c = self.be.to_host(e), self.be.to_host(c)
        return e, np.array([_sign_fix(c[0]), _sign_fix(c[1])])

    def get_init_guess(self, mol=None, key="1e"):
        """Core-Hamiltonian guess (the reference's 'minao' needs tabulated atomic densities)."""
        h = np.asarray(self.get_hcore())
        if h.ndim == 2:
            h = np.array((h, h))
        e, c = self.eig(h)
        return self.make_rdm1(c, self.get_occ(e, c))

    def kernel(self, dm0=None):
        """``scf.hf.kernel`` control flow: CDIIS from cycle 1, stop on
        |dE| < conv_tol and |g| < sqrt(conv_tol), then one DIIS-free conv_check cycle."""
        from .diis import CDIIS

        be = self.be
        patched = any(k in vars(self) for k in ("get_veff", "get_occ", "make_rdm1", "get_fock"))
        if not patched and self._device_kernel_ok:
            # (an object on a factor of the integrals takes the step-by-step loop: nbx_mu_cycle reads the tensor)
            if (hasattr(be, "mu_cycle") and os.environ.get("NBED_CYCLE_CALL", "1") != "0"
                    and self._eri_factor_d is None):
                return self._kernel_cycle_calls(dm0)
            if all(hasattr(be, a) for a in ("huz_cycle_scalars_async", "density_occ", "vo_sumsq", "async_to_host")):
                return self._kernel_device(dm0)
        h1e = np.asarray(self.get_hcore())  # possibly patched by the driver: evaluated once
        if h1e.ndim == 2:
            h1e = np.array((h1e, h1e))
        h_d = be.asarray(h1e)
        dm_d = be.asarray(self.get_init_guess() if dm0 is None else np.asarray(dm0))

        def fock_and_energy(dm_dev):
            fock, e1, e2 = self._fock_energy_device(h_d, dm_dev)
            return fock, float(e1 + e2 + self.energy_nuc()), float(e1), float(e2)

        fock, e_tot, e1, e2 = fock_and_energy(dm_d)
        diis = CDIIS(be, self._s_d)
        warm = {}
        conv_tol_grad = np.sqrt(self.conv_tol)
        self.converged = False
        mo_energy = mo_coeff = mo_occ = None
        for cycle in range(self.max_cycle):
            last_e = e_tot
            f_use = diis.update(dm_d, fock) if cycle >= 1 else fock
            e_d, c_d = self._eig_device(f_use, warm)
            mo_energy = be.to_host(e_d)
            mo_occ = self.get_occ(mo_energy)
            dm_d = self.make_rdm1_device(c_d, mo_occ)
            fock, e_tot, e1, e2 = fock_and_energy(dm_d)
            norm_gorb = self._grad_norm(c_d, mo_occ, fock)
            self.cycles = cycle + 1
            if abs(e_tot - last_e) < self.conv_tol and norm_gorb < conv_tol_grad:
                self.converged = True
                break
        if self.converged:
            e_d, c_d = self._eig_device(fock, warm)
            mo_energy = be.to_host(e_d)
            mo_occ = self.get_occ(mo_energy)
            dm_d = self.make_rdm1_device(c_d, mo_occ)
            fock, e_tot, e1, e2 = fock_and_energy(dm_d)
        c_h = be.to_host(c_d)
        self.mo_coeff = np.array([_sign_fix(c_h[0]), _sign_fix(c_h[1])])
        self.mo_energy, self.mo_occ = mo_energy, mo_occ
        self.e_tot = e_tot
        self.scf_summary["e1"], self.scf_summary["e2"] = e1, e2
        return e_tot

    _device_kernel_ok = True  # the look-ahead loop below assumes veff = J - K[x] (Hartree-Fock)
    cycle_callback = None  # callable(cycle) or None: called by the one-call-per-cycle kernel() loop
    kernel_info = None  # how the last kernel() went: cycle_call, split, tracked_cycles, guarded_cycles, restarts

    def _fock_energy_device(self, h_d, dm_dev):
        """(fock, e1, e2) of a two-spin density on the device: F = h + J - K[x], e1 = tr(h D),
        e2 = 1/2 tr(vhf D) (PySCF uhf.energy_elec)."""
        be = self.be
        fock, vhf = be.fock_uhf(h_d, None, self.jk_device(dm_dev))
        e1 = be.trace_prod(h_d, dm_dev).sum()
        e2 = 0.5 * be.trace_prod(vhf, dm_dev).sum()
        return fock, float(e1), float(e2)

    def _kernel_cycle_calls(self, dm0=None):
        """``scf.hf.kernel`` with ONE C call per cycle (nbx_mu_cycle: CDIIS -> eigensolve -> density -> J/K + Fock
        -> orbital gradient -> scalars stored into pinned memory), cycle i judged after cycle i+1 has been queued.
        The same kernels in the same order as ``_kernel_device`` issues one by one (``NBED_CYCLE_CALL=0``), so the
        guarded form is bit-identical to it; as in ``huzinaga_scf`` the eigenproblem of a cycle is solved by
        refining the previous cycle's pair on the pencil (F, S) with no fallback queued ("tracked") once a cycle has
        shown that refinement is accepted within two iterations -- and a rejected tracked cycle makes the whole run
        repeat with the guarded solver, the path the parity tests pin.  Over several ranks (J/K row slabs) the
        cycle is three calls around the all-reduce of the J/K partials."""
        tracked = os.environ.get("NBED_TRACKED_EIG", "1") != "0"
        self.kernel_info = {"restarts": []}
        for _ in range(2):
            try:
                return self._kernel_cycle_calls_once(dm0, tracked)
            except _TrackedCycleRejected as exc:
                logger.warning("tracked eigensolve rejected a cycle (%s): repeating kernel() with the guarded solver", exc)
                tracked = False
                self.kernel_info = {"restarts": self.kernel_info["restarts"] + [str(exc)]}
        raise RuntimeError("kernel(): the guarded run cannot raise _TrackedCycleRejected")  # pragma: no cover

    def _kernel_cycle_calls_once(self, dm0, allow_tracked):
        be = self.be
        h1e = np.asarray(self.get_hcore())  # possibly patched by the driver (mu P + V_emb): evaluated once
        if h1e.ndim == 2:
            h1e = np.array((h1e, h1e))
        n = h1e.shape[-1]
        nelec = tuple(int(x) for x in self.mol.nelec)
        gsize = max(sum((n - k) * k for k in nelec), 1)
        e_nuc = self.energy_nuc()
        dm_h = np.ascontiguousarray(self.get_init_guess() if dm0 is None else np.asarray(dm0), dtype=np.float64)
        sh = self.shards
        split = sh.world > 1 or sh.force_collective
        reduce = (lambda jk: sh.all_reduce(be, jk)) if split else None
        if hasattr(be, "asarray_many"):
            h_d, dm_d = be.asarray_many([h1e, dm_h])
        else:
            h_d, dm_d = be.asarray(h1e), be.asarray(dm_h)
        s_b = be.torch.stack([self._s_d] * 2).contiguous() if hasattr(be, "torch") and isinstance(
            self._s_d, be.torch.Tensor) else be.asarray(np.stack([self._s_h] * 2))
        packed_d = self.eri_packed_device()
        hstate = be.mu_cycle_state(n, nelec, packed_d, h_d, s_b, self.x_device(),
                                   eri=None if packed_d is not None else self.eri_device(), p0=sh.lo, p1=sh.hi)
        info = getattr(self, "kernel_info", None) or {}
        info.update(cycle_call=True, split=bool(split), tracked_cycles=0, guarded_cycles=0)
        self.kernel_info = info

        def energy(handle):
            return float(handle.get()[:2].sum() + e_nuc)

        first = hstate.sets[2]
        first["dm"] = dm_d  # (the starting density is the caller's: not a result buffer)
        last_e = e_tot = energy(be.mu_cycle_fock(hstate, dm_d, first, reduce=reduce))
        conv_tol_grad = np.sqrt(self.conv_tol)
        self.converged = False
        warm = {"v": None, "c": None, "iters": 3, "tracked": False}
        can_track = bool(allow_tracked)

        def judge(st):
            nonlocal last_e, e_tot
            handle = st["handle"]
            e_now = energy(handle)
            norm_gorb = float(np.sqrt(handle.get_dtail().sum()) / np.sqrt(gsize))
            status = handle.get_extra()
            if st["tracked"]:
                if np.any(status <= 0):
                    raise _TrackedCycleRejected(f"cycle {st['cycle']}: status {status.tolist()}")
            # launch-count policy of the eigensolver (results do not depend on it), as in huzinaga_scf: every
            # matrix accepted by refinement within two iterations -> refine without the guard from the next cycle
            # queued on, one iteration in reserve while the energy still moves
            accepted = bool(np.all(status >= 1001))
            needed = int(np.max(status)) - 1000 if accepted else 99
            warm["tracked"] = bool(can_track and needed <= 2)
            if warm["tracked"]:
                warm["iters"] = needed + (1 if abs(e_now - last_e) > 1e-9 else 0)
            else:
                warm["iters"] = 3
            self.cycles = st["cycle"] + 1
            ok = abs(e_now - last_e) < self.conv_tol and norm_gorb < conv_tol_grad
            logger.debug("kernel() cycle %s E = %.12f dE = %.3e |g| = %.3e status %s", st["cycle"], e_now,
                         e_now - last_e, norm_gorb, status.tolist())
            last_e = e_tot = e_now
            return ok

        head = nd = 0  # pyscf.lib.diis ring position of CDIIS (space 8)
        space = 8
        prev, pending, final = first, None, None
        for cycle in range(self.max_cycle):
            if self.cycle_callback is not None:
                self.cycle_callback(cycle)  # (host side, before cycle `cycle` is queued: bench.py separates warm-up cycles)
            out = hstate.sets[cycle % 3]
            diis_on = cycle >= 1
            slot = 0
            if diis_on:
                slot = head % space
                head += 1
                nd = min(nd + 1, space)
            tracked_now = bool(warm["tracked"] and warm["c"] is not None)
            c_in = warm["c"] if tracked_now else warm["v"]
            handle = be.mu_cycle(hstate, prev["dm"], prev["fock"], c_in, out, tracked_now, warm["iters"], diis_on, slot,
                                 nd, want_grad=True, reduce=reduce)
            info["tracked_cycles" if tracked_now else "guarded_cycles"] += 1
            warm["c"] = out["c"]
            if not tracked_now:
                warm["v"] = out["v"]
            cur = {"cycle": cycle, "set": out, "handle": handle, "tracked": tracked_now}
            if pending is not None and judge(pending):
                self.converged, final = True, pending
                break
            pending, prev = cur, out
        if not self.converged and pending is not None:
            self.converged = judge(pending)
            final = pending
        if final is None:  # max_cycle == 0
            res = first
            c_d = w_d = None
        else:
            res = final["set"]
            c_d, w_d = res["c"], res["w"]
        if self.converged:  # one DIIS-free cycle from the converged Fock matrix (conv_check)
            k = final["cycle"]
            out = hstate.sets[(k + 2) % 3]  # (k + 1 may be the look-ahead cycle still in flight: any set but k's is safe)
            tracked_now = bool(warm["tracked"] and warm["c"] is not None)
            # the warm start is whatever the LAST queued cycle left (the look-ahead cycle included): a start, not data
            c_in = warm["c"] if tracked_now else warm["v"]
            if c_in is not None and (c_in is out["c"] or c_in is out["v"]):
                c_in = be.copy(c_in)
            handle = be.mu_cycle(hstate, res["dm"], res["fock"], c_in, out, tracked_now, warm["iters"], False, 0, 0,
                                 want_grad=False, reduce=reduce)
            e_tot = energy(handle)
            status = handle.get_extra()
            if tracked_now and np.any(status <= 0):
                raise _TrackedCycleRejected(f"conv_check: status {status.tolist()}")
            res, c_d, w_d = out, out["c"], out["w"]
        mo_occ = np.zeros((2, n))
        mo_occ[0, : nelec[0]] = 1
        mo_occ[1, : nelec[1]] = 1
        if c_d is not None:
            if hasattr(be, "to_host_many"):
                c_h, w_h = be.to_host_many([c_d, w_d])
            else:
                c_h, w_h = be.to_host(c_d), be.to_host(w_d)
            self.mo_coeff = np.array([_sign_fix(c_h[0]), _sign_fix(c_h[1])])
            self.mo_energy = w_h
        self.mo_occ = mo_occ
        self.e_tot = e_tot
        self.scf_summary["e1"] = float(be.trace_prod(h_d, res["dm"]).sum())
        self.scf_summary["e2"] = float(0.5 * be.trace_prod(res["vhf"], res["dm"]).sum())
        return e_tot

    def _kernel_device(self, dm0=None):
        """The same control flow with nothing in a cycle waiting for the host (HIP backend): CDIIS,
        energy and orbital-gradient norm are computed on the device, the scalars come back through
        stream-ordered copies and cycle i is judged after cycle i+1 has been queued (dropped if
        cycle i had converged); occupations are the fixed aufbau vector because the eigensolver
        returns ascending eigenvalues.  Same numbers as the synchronous loop."""
        from .diis import CDIIS

        be = self.be
        h1e = np.asarray(self.get_hcore())  # possibly patched by the driver: evaluated once
        if h1e.ndim == 2:
            h1e = np.array((h1e, h1e))
        h_d = be.asarray(h1e)
        n = h1e.shape[-1]
        nelec = tuple(int(x) for x in self.mol.nelec)
        zero = be.zeros((2, n, n))
        gsize = max(sum((n - k) * k for k in nelec), 1)
        e_nuc = self.energy_nuc()
        dm_d = be.asarray(self.get_init_guess() if dm0 is None else np.asarray(dm0))

        def build(dm_dev, c_dev=None):
            """Fock from dm_dev, its energy and (given the orbitals) the gradient norm, all queued."""
            fock, vhf = self.fock_device(dm_dev, h_d)
            pend_e = be.huz_cycle_scalars_async(h_d, None, vhf, zero, dm_dev, dm_dev)
            pend_g = None
            if c_dev is not None:
                fmo = be.gemm(be.gemm(c_dev, fock, "T", "N"), c_dev)
                pend_g = be.async_to_host(be.vo_sumsq(fmo, nelec))
            return fock, vhf, pend_e, pend_g

        def energy(pend_e):
            return float(pend_e.get()[:2].sum() + e_nuc)

        fock, vhf, pend_e, _ = build(dm_d)
        last_e = energy(pend_e)  # energy of the starting density
        diis = CDIIS(be, self._s_d)
        warm = {}
        conv_tol_grad = np.sqrt(self.conv_tol)
        self.converged = False
        prev = {"dm": dm_d, "fock": fock, "vhf": vhf}
        pending = final = None
        e_tot = last_e

        def judge(st):
            nonlocal last_e, e_tot
            e_now = energy(st["pend_e"])
            norm_gorb = float(np.sqrt(st["pend_g"].get().sum()) / np.sqrt(gsize))
            self.cycles = st["cycle"] + 1
            ok = abs(e_now - last_e) < self.conv_tol and norm_gorb < conv_tol_grad
            last_e = e_tot = e_now
            return ok

        for cycle in range(self.max_cycle):
            f_use = diis.update(prev["dm"], prev["fock"]) if cycle >= 1 else prev["fock"]
            e_d, c_d = self._eig_device(f_use, warm)
            dm_new = be.density_occ(c_d, nelec)
            fock_new, vhf_new, pe, pg = build(dm_new, c_d)
            cur = {"cycle": cycle, "dm": dm_new, "fock": fock_new, "vhf": vhf_new, "e": e_d, "c": c_d, "pend_e": pe,
                   "pend_g": pg}
            if pending is not None and judge(pending):
                self.converged, final = True, pending
                break
            pending = prev = cur
        if not self.converged and pending is not None:
            self.converged = judge(pending)
            final = pending
        if final is None:  # max_cycle == 0
            final = {"dm": dm_d, "fock": fock, "vhf": vhf, "e": None, "c": None}
        if self.converged:  # one DIIS-free cycle from the converged Fock matrix (conv_check)
            e_d, c_d = self._eig_device(final["fock"], warm)
            dm_f = be.density_occ(c_d, nelec)
            fock_f, vhf_f, pe, _ = build(dm_f)
            e_tot = energy(pe)
            final = {"dm": dm_f, "fock": fock_f, "vhf": vhf_f, "e": e_d, "c": c_d}
        mo_occ = np.zeros((2, n))
        mo_occ[0, : nelec[0]] = 1
        mo_occ[1, : nelec[1]] = 1
        if final["c"] is not None:
            c_h = be.to_host(final["c"])
            self.mo_coeff = np.array([_sign_fix(c_h[0]), _sign_fix(c_h[1])])
            self.mo_energy = be.to_host(final["e"])
        self.mo_occ = mo_occ
        self.e_tot = e_tot
        self.scf_summary["e1"] = float(be.trace_prod(h_d, final["dm"]).sum())
        self.scf_summary["e2"] = float(0.5 * be.trace_prod(final["vhf"], final["dm"]).sum())
        return e_tot

    def _grad_norm(self, c_d, mo_occ, fock_d) -> float:
        """|| C_vir^T F C_occ || / sqrt(size) over both spins (PySCF get_grad + kernel)."""
        be = self.be
        fmo = be.gemm(be.gemm(c_d, fock_d, "T", "N"), c_d)  # (2, n, n) MO-basis Fock
        fmo_h = be.to_host(fmo)
        g = []
        for x in range(2):
            occ = mo_occ[x] > 0
            g.append(fmo_h[x][~occ][:, occ].ravel())
        g = np.hstack(g)
        return float(np.linalg.norm(g) / np.sqrt(max(g.size, 1)))


class TaggedVeff(np.ndarray):
    """ndarray carrying ``.ecoul`` / ``.exc`` / ``.vj`` / ``.vk`` like the tagged array PySCF's
    Kohn-Sham ``get_veff`` returns (read at nbed/scf/huzinaga_scf.py:55-56, nbed/driver.py:361-365)."""

    ecoul = exc = vj = vk = None


def _check_eri_lr(mf, eri_lr):
    """The attenuated tensor of a range-separated Kohn-Sham object on its device (None when beta = 0)."""
    if mf.beta == 0.0:
        return None
    if eri_lr is None:
        raise ValueError(f"beta = {mf.beta}: a range-separated hybrid needs eri_lr, the tensor over erf(omega r12) / r12")
    if mf._eri_factor_d is not None:
        raise ValueError("a range-separated hybrid runs on dense tensors: eri_factor has no attenuated counterpart")
    nao = mf._s_h.shape[0]
    eri_lr = mf.be.asarray(eri_lr)
    if tuple(eri_lr.shape) != (mf.shards.size, nao, nao, nao):
        raise ValueError(f"eri_lr has shape {tuple(eri_lr.shape)}, expected {(mf.shards.size, nao, nao, nao)}")
    return eri_lr


def _k_lr_device(mf, dm_d):
    """K_lr[x] (ndm, N, N) on device: the J/K build of ``jk_device`` on the attenuated tensor, J dropped."""
    be, sh = mf.be, mf.shards
    if hasattr(be, "jk_sym"):
        return sh.all_reduce(be, be.jk_sym(mf._eri_lr_d, dm_d, sh.lo, sh.hi))[1:]
    return sh.all_gather(be, be.jk(mf._eri_lr_d, dm_d, sh.lo, sh.hi), axis=1)[1:]


class GpuUKS(GpuUHF, UKS):
    """Unrestricted Kohn-Sham object over dense S, hcore, (pq|rs): what the reference builds as
    ``dft.UKS`` (nbed/driver.py:163,303) and hands to ``huzinaga_scf`` (KS branch,
    nbed/scf/huzinaga_scf.py:36-62,176-180), ``_subsystem_dft`` (:315-431) and the embedding
    potential (:845-852).  The Coulomb and exact-exchange parts are libnbx J/K builds,

        veff[x] = J - hyb K[x] + v_xc[x],   ecoul = 1/2 tr(D_tot J),
        exc     = E_xc[D] - hyb/2 sum_x tr(D[x] K[x]),

    or, for a range-separated hybrid (``beta`` != 0: ``eri_lr`` is the dense device tensor over erf(omega r12) / r12,
    ``backend.eri(basis, omega=omega)``, and ``alpha`` another name for ``hyb``),

        veff[x] = J - alpha K[x] - beta K_lr[x] + v_xc[x],
        exc     = E_xc[D] - 1/2 sum_x tr(D[x] (alpha K[x] + beta K_lr[x])),

    with K_lr from the same J/K kernels run on ``eri_lr`` (the J they return beside it is dropped: there is no K-only
    kernel).  With beta = 0 nothing of this runs: the arithmetic and the launches are those above.  The semi-local part (E_xc, v_xc) comes from ``xc_provider(dm (2,N,N)) -> (E_xc, v_xc (2,N,N))``
    (``nbed_amd.xc``; None = no semi-local part, i.e. a pure exact-exchange hybrid: with hyb = 1
    this object is Hartree-Fock with Kohn-Sham bookkeeping)."""

    _device_kernel_ok = False

    def __init__(self, mol, ovlp, hcore, eri=None, backend=None, shards=None, xc="hf", hyb=1.0, xc_provider=None,
                 eri_packed=None, eri_factor=None, omega=0.0, alpha=None, beta=0.0, eri_lr=None):
        super().__init__(mol, ovlp, hcore, eri, backend=backend, shards=shards, eri_packed=eri_packed, eri_factor=eri_factor)
        self.xc = xc
        self.hyb = float(hyb if alpha is None else alpha)
        self.xc_provider = xc_provider
        self.omega, self.beta = float(omega), float(beta)
        self._eri_lr_d = _check_eri_lr(self, eri_lr)

    @property
    def alpha(self) -> float:
        return self.hyb

    def _veff_parts_device(self, dm_d):
        """(veff (2,N,N) device, ecoul, exc, jk (3,N,N) device) of a two-spin density."""
        be = self.be
        jk = self.jk_device(dm_d)
        veff = be.copy(jk[1:])
        for x in range(2):  # veff[x] = J - hyb K[x]
            be.axpby(1.0, jk[0], -self.hyb, veff[x])
        tr_j = be.trace_prod(jk[0], dm_d[0]) + be.trace_prod(jk[0], dm_d[1])
        ecoul = 0.5 * float(tr_j)
        exc = -0.5 * self.hyb * float(be.trace_prod(jk[1:], dm_d).sum())
        if self.beta != 0.0:  # veff[x] -= beta K_lr[x]
            k_lr = _k_lr_device(self, dm_d)
            for x in range(2):
                be.axpby(-self.beta, k_lr[x], 1.0, veff[x])
            exc -= 0.5 * self.beta * float(be.trace_prod(k_lr, dm_d).sum())
        if self.xc_provider is not None:
            e_sl, v_sl = self.xc_provider(be.to_host(dm_d))
            exc += float(e_sl)
            be.axpby(1.0, be.asarray(np.asarray(v_sl)), 1.0, veff)
        return veff, ecoul, exc, jk

    def get_veff(self, mol=None, dm=None, dm_last=0, vhf_last=0, hermi=1):
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        if dm.ndim == 2:
            dm = np.array((dm * 0.5, dm * 0.5))
        veff, ecoul, exc, jk = self._veff_parts_device(self.be.asarray(dm))
        out = self.be.to_host(veff).view(TaggedVeff)
        jk_h = self.be.to_host(jk)
        out.ecoul, out.exc, out.vj, out.vk = ecoul, exc, jk_h[0], jk_h[1:]
        return out

    def get_veff_device(self, dm_d):
        return self._veff_parts_device(dm_d)[0]

    def fused_fock_available(self, hv_d) -> bool:
        return False  # the fused build assembles the Hartree-Fock F = h + J - K[x]

    def fock_device(self, dm_d, hv_d, dts_ready: bool = False):
        veff = self.get_veff_device(dm_d)
        fock = self.be.copy(hv_d)
        self.be.axpby(1.0, veff, 1.0, fock)
        return fock, veff

    def _fock_energy_device(self, h_d, dm_dev):
        be = self.be
        veff, ecoul, exc, _ = self._veff_parts_device(dm_dev)
        fock = be.copy(h_d)
        be.axpby(1.0, veff, 1.0, fock)
        return fock, float(be.trace_prod(h_d, dm_dev).sum()), ecoul + exc

    def energy_elec(self, dm=None, h1e=None, vhf=None):
        """PySCF ``uks.energy_elec``: e1 + ecoul + exc from the tagged veff."""
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        if dm.ndim == 2:
            dm = np.array((dm * 0.5, dm * 0.5))
        h1e = self.get_hcore() if h1e is None else np.asarray(h1e)
        if h1e.ndim == 2:
            h1e = np.array((h1e, h1e))
        if vhf is None or getattr(vhf, "ecoul", None) is None:
            vhf = self.get_veff(self.mol, dm)
        e1 = float(self.be.trace_prod(self.be.asarray(h1e), self.be.asarray(dm)).sum())
        e2 = float(vhf.ecoul + vhf.exc)
        self.scf_summary.update(e1=e1, coul=float(vhf.ecoul), exc=float(vhf.exc), e2=e2)
        return e1 + e2, e2


class GpuRKS(_GpuSCF, RKS):
    """Restricted Kohn-Sham object (2-D arrays; the density carries the factor 2): ``dft.RKS`` as the
    reference's tests hand it to ``huzinaga_scf`` (tests/test_scf.py:19-40).  J and the exact-exchange
    fraction are libnbx builds; the semi-local part comes from ``xc_provider`` (``nbed_amd.xc``), called
    with the two equal spin halves of the density."""

    def __init__(self, mol, ovlp, hcore, eri=None, backend=None, xc="lda,vwn", hyb=0.0, xc_provider=None, omega=0.0,
                 alpha=None, beta=0.0, eri_lr=None):
        """``omega``, ``alpha`` (another name for ``hyb``), ``beta``, ``eri_lr``: the exact part alpha K + beta K_lr of a
        range-separated hybrid, as in ``GpuUKS``."""
        super().__init__(mol, ovlp, hcore, eri, backend=backend)
        self.xc, self.hyb, self.xc_provider = xc, float(hyb if alpha is None else alpha), xc_provider
        self.omega, self.beta = float(omega), float(beta)
        self._eri_lr_d = _check_eri_lr(self, eri_lr)

    def get_veff(self, mol=None, dm=None, dm_last=0, vhf_last=0, hermi=1):
        be = self.be
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        jk = be.to_host(self.jk_device(be.asarray(dm[None])))
        veff = jk[0] - 0.5 * self.hyb * jk[1]
        ecoul = 0.5 * float(np.einsum("ij,ji->", jk[0], dm))
        exc = -0.25 * self.hyb * float(np.einsum("ij,ji->", jk[1], dm))
        if self.beta != 0.0:
            k_lr = be.to_host(_k_lr_device(self, be.asarray(dm[None])))[0]
            veff = veff - 0.5 * self.beta * k_lr
            exc -= 0.25 * self.beta * float(np.einsum("ij,ji->", k_lr, dm))
        if self.xc_provider is not None:
            e_sl, v_sl = self.xc_provider(np.array((0.5 * dm, 0.5 * dm)))
            exc += float(e_sl)
            veff = veff + 0.5 * (np.asarray(v_sl)[0] + np.asarray(v_sl)[1])
        out = np.asarray(veff).view(TaggedVeff)
        out.ecoul, out.exc, out.vj, out.vk = ecoul, exc, jk[0], jk[1]
        return out

    def get_occ(self, mo_energy=None, mo_coeff=None):
        mo_energy = self.mo_energy if mo_energy is None else np.asarray(mo_energy)
        mo_occ = np.zeros_like(mo_energy)
        mo_occ[np.argsort(mo_energy)[: self.mol.nelectron // 2]] = 2
        return mo_occ

    def make_rdm1(self, mo_coeff=None, mo_occ=None):
        mo_coeff = np.asarray(self.mo_coeff if mo_coeff is None else mo_coeff)
        mo_occ = np.asarray(self.mo_occ if mo_occ is None else mo_occ)
        return (mo_coeff * mo_occ) @ mo_coeff.T

    def energy_elec(self, dm=None, h1e=None, vhf=None):
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        h1e = self.get_hcore() if h1e is None else np.asarray(h1e)
        if vhf is None or getattr(vhf, "ecoul", None) is None:
            vhf = self.get_veff(self.mol, dm)
        e1 = float(np.einsum("ij,ji->", h1e, dm))
        e2 = float(vhf.ecoul + vhf.exc)
        self.scf_summary.update(e1=e1, coul=float(vhf.ecoul), exc=float(vhf.exc), e2=e2)
        return e1 + e2, e2


class GpuRHF(_GpuSCF, RHF):
    """Restricted flavour (2-D arrays; density carries the factor 2)."""

    def get_jk(self, mol=None, dm=None, hermi=1):
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        jk = self.be.to_host(self.jk_device(self.be.asarray(dm[None])))
        return jk[0], jk[1]

    def get_j(self, mol=None, dm=None, hermi=1):
        return self.get_jk(mol, dm)[0]

    def get_veff(self, mol=None, dm=None, dm_last=0, vhf_last=0, hermi=1):
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        return self.be.to_host(self.get_veff_device(self.be.asarray(dm)))

    def get_veff_device(self, dm_d):
        jk = self.jk_device(dm_d.reshape(1, *dm_d.shape[-2:]))
        vhf = self.be.copy(jk[0])
        self.be.axpby(-0.5, jk[1], 1.0, vhf)  # J - K/2
        return vhf

    def get_occ(self, mo_energy=None, mo_coeff=None):
        mo_energy = self.mo_energy if mo_energy is None else np.asarray(mo_energy)
        mo_occ = np.zeros_like(mo_energy)
        mo_occ[np.argsort(mo_energy)[: self.mol.nelectron // 2]] = 2
        return mo_occ

    def make_rdm1_device(self, c_d, occ_h):
        scaled = self.be.scale_cols(self.be.copy(c_d), self.be.asarray(occ_h))
        return self.be.gemm(scaled, c_d, "N", "T")

    def make_rdm1(self, mo_coeff=None, mo_occ=None):
        mo_coeff = self.mo_coeff if mo_coeff is None else mo_coeff
        mo_occ = self.mo_occ if mo_occ is None else mo_occ
        return self.be.to_host(self.make_rdm1_device(self.be.asarray(np.asarray(mo_coeff)), np.asarray(mo_occ)))

    def get_fock(self, h1e=None, s1e=None, vhf=None, dm=None, cycle=-1, diis=None):
        h1e = self.get_hcore() if h1e is None else h1e
        if vhf is None:
            vhf = self.get_veff(self.mol, self.make_rdm1() if dm is None else dm)
        return np.asarray(h1e) + vhf

    def energy_elec(self, dm=None, h1e=None, vhf=None):
        dm = self.make_rdm1() if dm is None else np.asarray(dm)
        h1e = self.get_hcore() if h1e is None else np.asarray(h1e)
        vhf = self.get_veff(self.mol, dm) if vhf is None else np.asarray(vhf)
        be = self.be
        dm_d = be.asarray(dm)
        e1 = float(be.trace_prod(be.asarray(h1e), dm_d))
        e_coul = 0.5 * float(be.trace_prod(be.asarray(vhf), dm_d))
        self.scf_summary["e1"], self.scf_summary["e2"] = e1, e_coul
        return e1 + e_coul, e_coul

    def energy_tot(self, dm=None, h1e=None, vhf=None):
        return self.energy_elec(dm, h1e, vhf)[0] + self.energy_nuc()

    def eig(self, fock, s=None):
        e, c = self._eig_device(self.be.asarray(np.asarray(fock)))
        return self.be.to_host(e), _sign_fix(self.be.to_host(c))
