"""Pipek-Mezey and Boys localizers on libnbx's Jacobi-sweep kernels (mirror of nbed/localizers/occupied/pyscf.py).

Both maximise f(U) = sum_k sum_i ((U^T Q_k U)_ii)^2 over rotations U of the occupied orbitals C_occ
(Pipek & Mezey, J. Chem. Phys. 90, 4916 (1989)):

* Boys (``pyscf.lo.boys.Boys``, pyscf.py:378): Q_k = C_occ^T r_k C_occ, k = x, y, z, with the AO dipole matrices
  ``int1e_r`` (origin 0: the origin shifts f by a constant).
* Pipek-Mezey (``pyscf.lo.PipekMezey``, pyscf.py:317-324, exponent 2): one Q_A per atom,
  Q_A = 1/2 (X_A^T Y_A + Y_A^T X_A) over the atom's AO rows, with
  'mulliken'     X = C_occ, Y = S C_occ (PySCF's Mulliken populations);
  'lowdin'       X = Y = S^1/2 C_occ, the symmetric Loewdin basis of the AOs themselves -- PySCF's 'lowdin' first
                 projects on its ANO reference basis, which is not the same;
  'meta-lowdin'  X = Y = O^T S C_occ with O the meta-Loewdin orthogonal AOs (the reference's choice: they need
                 PySCF's ANO basis, so they come from ``pop_ao`` or from pyscf.lo.orth_ao on a PySCF molecule).

The sweeps run on the GPU in one launch per call (``nbx_loc_pm`` / ``nbx_loc_boys``; both spins of an
unrestricted calculation as one batch) and start from the canonical orbitals.  PySCF starts from its 'atomic'
guess, which needs the ANO basis: the functional is the same, but a different start can reach a different local
maximum.  The active / environment split is ``PySCFLocalizer._localize_spin`` (pyscf.py:90-180) as it stands.
"""

from __future__ import annotations

import logging

import numpy as np

from ..system import LocalizedSystem
from .base import OccupiedLocalizer

logger = logging.getLogger(__name__)


def _is_pyscf_mol(mol) -> bool:
    return type(mol).__module__.split(".")[0] == "pyscf"


class JacobiLocalizer(OccupiedLocalizer):
    """What PMLocalizer and BOYSLocalizer share: PySCFLocalizer (pyscf.py:18-262) with the PySCF call replaced by a
    rotation of C_occ computed on the GPU (``_rotations``)."""

    max_sweeps = 1000
    tol = 1e-10

    def __init__(self, global_scf, n_active_atoms: int, occ_cutoff: float = 0.95, virt_cutoff: float = 0.95,
                 backend=None):
        self.occ_cutoff = self._valid_threshold(occ_cutoff)
        self.virt_cutoff = self._valid_threshold(virt_cutoff)
        self.enviro_selection_condition = None
        self.sweeps: list[int] = []
        self.functional: list[float] = []
        self._done = []
        self._check_inputs(global_scf)
        super().__init__(global_scf, n_active_atoms, backend=backend)

    def _valid_threshold(self, threshold: float) -> float:
        if 0.0 <= threshold <= 1.0:
            logger.debug("Localizer threshold valid.")
            return threshold
        logger.error("Localizer threshold not valid.")
        raise ValueError(f"threshold: {threshold} is not in range [0,1] inclusive")

    def _check_inputs(self, global_scf) -> None:
        """Refuse what cannot be computed before anything runs."""

    def _rotations(self, c_d):
        """(U (batch, n, n) device, sweeps, f) for the (batch, nao, n) device array of occupied orbitals."""
        raise NotImplementedError

    def _localize_occ(self, blocks):
        """C_occ U of each (nao, n) block (all of one shape), in one launch."""
        be = self._be
        c_d = be.asarray(np.stack(blocks))
        u, sweeps, f = self._rotations(c_d)
        self.sweeps.extend(int(s) for s in sweeps)
        self.functional.extend(float(v) for v in f)
        c_loc = be.to_host(be.gemm(c_d, u))
        return [np.ascontiguousarray(c_loc[i]) for i in range(len(blocks))]

    def localize(self) -> LocalizedSystem:
        """The base class's localize(); alpha and beta are rotated together first when their occupied blocks have
        the same shape."""
        scf = self._global_scf
        self._done = []
        if not self.spinless:
            blocks = [np.ascontiguousarray(np.asarray(scf.mo_coeff[x])[:, : int(np.count_nonzero(scf.mo_occ[x]))])
                      for x in (0, 1)]
            if blocks[0].shape == blocks[1].shape and blocks[0].shape[1] > 0:
                self._done = list(zip(blocks, self._localize_occ(blocks)))
        try:
            return super().localize()
        finally:
            self._done = []

    def _localize_spin(self, c_matrix: np.ndarray, occupancy: np.ndarray,
                       n_mo_overwrite: int | None = None) -> LocalizedSystem:
        """pyscf.py:90-180; ``n_mo_overwrite`` is accepted and ignored, as there."""
        n_occupied_orbitals = np.count_nonzero(occupancy)
        c_std_occ = np.ascontiguousarray(np.asarray(c_matrix)[:, :n_occupied_orbitals])

        c_loc_occ = next((loc for c, loc in self._done if c.shape == c_std_occ.shape and np.array_equal(c, c_std_occ)),
                         None)
        if c_loc_occ is None:
            c_loc_occ = self._localize_occ([c_std_occ])[0] if c_std_occ.shape[1] > 0 else c_std_occ

        ao_slice_matrix = self._global_scf.mol.aoslice_by_atom()

        # find indices of AO of active atoms
        ao_active_inds = np.arange(ao_slice_matrix[0, 2], ao_slice_matrix[self._n_active_atoms - 1, 3])
        # active AOs coeffs for a given MO j
        numerator_all = np.einsum("ij->j", (c_loc_occ[ao_active_inds, :]) ** 2)
        # all AOs coeffs for a given MO j
        denominator_all = np.einsum("ij->j", c_loc_occ**2)

        mo_active_share = numerator_all / denominator_all

        logger.debug(f"(active_AO^2)/(all_AO^2): {np.around(mo_active_share, 4)}")
        logger.debug(f"threshold for active part: {self.occ_cutoff}")

        active_mo_inds = np.where(mo_active_share > self.occ_cutoff)[0]

        all_ao_shares_same_bool = np.allclose(
            np.zeros_like(mo_active_share),
            mo_active_share - mo_active_share.sum() / len(mo_active_share),
        )

        if all_ao_shares_same_bool:
            # highly symmetric molecules: the share is the same everywhere, split half and half
            logger.warning("AO subsystem selection % same everywhere. Splitting half and half")
            logger.warning(f"mo_active_share: {mo_active_share}")
            active_mo_inds = np.array(range(0, c_loc_occ.shape[1] // 2), dtype=int)
        elif len(active_mo_inds) == 0:
            # if no active indices, then take largest possible overlap
            mo_active_percentage_inshare = mo_active_share.argsort()[::-1]
            active_mo_inds = mo_active_percentage_inshare[:1]  # take first element
            logger.warning("no active AOs - forcing one to be active")
            logger.warning(f"active system %: {mo_active_share[active_mo_inds][0]}")

        enviro_mo_inds = np.array([i for i in range(c_loc_occ.shape[1]) if i not in active_mo_inds])

        # define active MO orbs and environment
        #    take MO (columns of C_matrix) that have high dependence from active AOs
        c_active = c_loc_occ[:, active_mo_inds]

        if len(enviro_mo_inds) == 0:
            # case for when no environement
            logger.warning("No environment electronic density")
            c_enviro = np.zeros((c_active.shape[0], 1))
        else:
            c_enviro = c_loc_occ[:, enviro_mo_inds]

        # storing condition used to select env system
        self.enviro_selection_condition = mo_active_share

        logger.debug("Jacobi-sweep localization complete.")
        return LocalizedSystem(active_mo_inds, enviro_mo_inds, c_active, c_enviro, c_loc_occ, backend=self._be)

    def localize_virtual(self, local_scf):
        """pyscf.py:245-262: not available for these localizers."""
        raise NotImplementedError("Virtual orbital localization not implemented for PySCF methods.")


class BOYSLocalizer(JacobiLocalizer):
    """Boys localisation (pyscf.py:327-379): maximises sum_i |<i| r |i>|^2, i.e. minimises the orbitals' spread."""

    def __init__(self, global_scf, n_active_atoms: int, occ_cutoff: float = 0.95, virt_cutoff: float = 0.95,
                 backend=None):
        self._r = None
        super().__init__(global_scf, n_active_atoms, occ_cutoff=occ_cutoff, virt_cutoff=virt_cutoff, backend=backend)

    def _check_inputs(self, global_scf) -> None:
        if not hasattr(global_scf.mol, "intor_symmetric"):
            raise NotImplementedError(f"Boys localisation needs the dipole integrals (int1e_r) of the molecule; "
                                      f"{type(global_scf.mol).__name__} cannot provide them")

    def _rotations(self, c_d):
        be = self._be
        if self._r is None:
            self._r = be.asarray(np.asarray(self._global_scf.mol.intor_symmetric("int1e_r", comp=3)))
        batch, _, n = (int(v) for v in c_d.shape)
        q = be.empty((batch, 3, n, n))
        for b in range(batch):
            be.gemm(c_d[b], be.gemm(self._r, c_d[b]), "T", "N", out=q[b])  # C^T r_k C
        return be.localize_boys(q, self.max_sweeps, self.tol)


class PMLocalizer(JacobiLocalizer):
    """Pipek-Mezey localisation (pyscf.py:265-324): maximises the sum of the squared atomic populations of the
    orbitals.  ``pop_method``: 'meta-lowdin' (the reference's), 'mulliken' or 'lowdin' (module docstring);
    ``pop_ao``: the (nao, nao) orthogonal AOs of 'meta-lowdin', when the caller has them."""

    POP_METHODS = ("mulliken", "lowdin", "meta-lowdin")

    def __init__(self, global_scf, n_active_atoms: int, occ_cutoff: float = 0.95, virt_cutoff: float = 0.95,
                 pop_method: str = "meta-lowdin", pop_ao=None, backend=None):
        self.pop_method = str(pop_method).lower().replace("_", "-")
        self.pop_ao = pop_ao
        self._ops = None
        super().__init__(global_scf, n_active_atoms, occ_cutoff=occ_cutoff, virt_cutoff=virt_cutoff, backend=backend)

    def _check_inputs(self, global_scf) -> None:
        if self.pop_method not in self.POP_METHODS:
            raise ValueError(f"pop_method {self.pop_method!r} is not one of {self.POP_METHODS}")
        if self.pop_method == "meta-lowdin" and self.pop_ao is None:
            mol = getattr(global_scf, "mol", None)
            if not _is_pyscf_mol(mol):
                raise NotImplementedError(
                    "Pipek-Mezey with pop_method='meta-lowdin' (the reference's populations) needs the meta-Loewdin "
                    "orthogonal AOs, which are built on PySCF's ANO reference basis: pass pop_ao=, or use "
                    "pop_method='mulliken' or pop_method='lowdin'")
            from pyscf import lo

            self.pop_ao = lo.orth_ao(mol, "meta_lowdin")

    def _ao_offsets(self) -> np.ndarray:
        sl = np.asarray(self._global_scf.mol.aoslice_by_atom())
        return np.concatenate([[sl[0, 2]], sl[:, 3]]).astype(np.int64)

    def _rotations(self, c_d):
        be = self._be
        if self._ops is None:  # (W, V): X = W C (C itself if W is None), Y = V C (Y = X if V is None)
            s = np.asarray(self._global_scf.get_ovlp())
            s_d = be.asarray(s)
            if self.pop_method == "mulliken":
                self._ops = (None, s_d)
            elif self.pop_method == "lowdin":
                fast = getattr(be, "sym_pow_fast", None)
                self._ops = (fast(s_d, 0.5, s) if fast is not None else be.sym_pow(s_d, 0.5), None)
            else:
                self._ops = (be.gemm(be.asarray(np.asarray(self.pop_ao)), s_d, "T", "N"), None)
        w, v = self._ops
        x = c_d if w is None else be.gemm(w, c_d)
        y = None if v is None else be.gemm(v, c_d)
        return be.localize_pm(x, y, self._ao_offsets(), self.max_sweeps, self.tol)
