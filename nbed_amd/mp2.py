"""Second-order perturbation theory of the embedded determinant, and frozen natural orbitals from it.

The reference offers its users CCSD and FCI on the embedded SCF object (nbed/driver.py:1044-1135) and one control
over the size of the active space besides the localisation: ``n_frozen_virt`` (nbed/ham_builder.py:257-285), which
drops the LAST virtual columns in whatever order they are.  The standard way to choose which virtual directions to
drop is second order: the virtual-virtual block of the one-particle density of the first-order wavefunction, whose
eigenvectors are the MP2 natural virtual orbitals ("frozen natural orbitals", FNO: Taube, Bartlett, Collect. Czech.
Chem. Commun. 70, 837 (2005)).  Its ingredients are the (ia|jb) block and an elementwise amplitude step.

Definitions (the contract of the kernel, the two solvers and the tests).  The reference determinant is ANY
determinant: f_ov != 0 and non-diagonal f_oo, f_vv are allowed (an embedded object after the concentric localisation
has all three).  For each spin f_oo and f_vv are diagonalised -- alpha never mixes with beta, as in
``ccsd.spin_block_eigh`` -- and in that semicanonical basis, with eigenvalues e:

    singles        t_ia   = f_ia / (e_i - e_a)                         E_s  = sum f_ia t_ia
    same spin      t_iajb = [(ia|jb) - (ib|ja)] / d                    E_ss = 1/4 sum t_iajb [(ia|jb) - (ib|ja)]
    opposite spin  t_iaJB = (ia|JB) / d                                E_ab = sum t_iaJB (ia|JB)
    d = ((e_i + e_j) - e_a) - e_b   (in this order)                    E(2) = E_s + E_aa + E_bb + E_ab
    D^a_ab = sum_i t_ia t_ib + 1/2 sum_{ijc in a} t_iajc t_ibjc + sum_{i in a, JC in b} t_iaJC t_ibJC

(D^b the same with the spins exchanged), D rotated back to the input virtual basis.  A restricted object runs the
alpha formulas once with C_b = C_a.

``solve`` is the host solver on the output of ``HamiltonianBuilder.build()`` (numpy, the conventions of
``ccsd.solve``); ``solve_scf`` the device solver that works from an SCF object and never forms the n^4 MO tensor;
``frozen_natural_orbitals`` truncates the virtual space of an SCF object in the natural-orbital basis.
"""

from __future__ import annotations

import logging

import numpy as np

from . import ccsd
from .backend import get_backend
from .scf.pyscf_compat import is_restricted

logger = logging.getLogger(__name__)

MAX_SPIN_ORBITALS = ccsd.MAX_SPIN_ORBITALS  # of the host solver, as ``ccsd.solve``
MEMORY_FRACTION = 0.6  # of the free device memory ``solve_scf`` plans with


class MP2Result:
    """``e_scf``, ``e_corr``, ``e_tot`` = ``e_scf + e_corr``; the parts ``e_singles``, ``e_same`` (alpha-alpha +
    beta-beta), ``e_opposite``; ``dvv``: the virtual-virtual block of the first-order wavefunction's one-particle
    density per spin, in the input virtual basis (the virtual orbitals of a spin in ascending order of their index),
    symmetrised -- an array (2, nv, nv), or a list of two square arrays where the spins have different numbers of
    virtuals (an open shell)."""

    def __init__(self, e_scf, e_singles, e_same, e_opposite, dvv):
        self.e_scf = float(e_scf)
        self.e_singles, self.e_same, self.e_opposite = float(e_singles), float(e_same), float(e_opposite)
        self.e_corr = self.e_singles + self.e_same + self.e_opposite
        self.e_tot = self.e_scf + self.e_corr
        d = [0.5 * (np.asarray(x, dtype=float) + np.asarray(x, dtype=float).T) for x in dvv]
        self.dvv = np.array(d) if d[0].shape == d[1].shape else d

    def natural_occupations(self):
        """Eigenvalues of ``dvv`` per spin, descending: (2, nv), or a list of two vectors (see ``dvv``)."""
        occ = [np.linalg.eigvalsh(d)[::-1].copy() if d.size else np.zeros(0) for d in self.dvv]
        return np.array(occ) if occ[0].shape == occ[1].shape else occ


# ---------------------------------------------------------------------------------------------------- host solver
def solve(constant: float, h1: np.ndarray, h2: np.ndarray, occupied) -> MP2Result:
    """MP2 of the determinant that occupies the spin orbitals ``occupied`` of the Hamiltonian ``build()`` returns
    (alpha on the even indices), by the definitions of this module's docstring over spin orbitals."""
    nso = h1.shape[0]
    if nso > MAX_SPIN_ORBITALS:
        raise ValueError(f"nbed_amd.mp2.solve is limited to {MAX_SPIN_ORBITALS} spin orbitals (got {nso})")
    occ = np.array(sorted(int(i) for i in occupied), dtype=int)
    vir = np.array([p for p in range(nso) if p not in set(occ.tolist())], dtype=int)
    g = ccsd.antisymmetrized(np.asarray(h2, dtype=float))
    f = np.asarray(h1, dtype=float) + np.einsum("piqi->pq", g[:, occ][:, :, :, occ])
    e_hf = constant + np.trace(h1[np.ix_(occ, occ)]) + 0.5 * np.einsum("ijij->", g[np.ix_(occ, occ, occ, occ)])
    so, sv = occ & 1, vir & 1
    eo, uo = ccsd.spin_block_eigh(f[np.ix_(occ, occ)], so)
    ev, uv = ccsd.spin_block_eigh(f[np.ix_(vir, vir)], sv)
    fov = uo.T @ f[np.ix_(occ, vir)] @ uv
    oovv = np.einsum("ijab,ip,jq,ar,bs->pqrs", g[np.ix_(occ, occ, vir, vir)], uo, uo, uv, uv, optimize=True)
    t1 = fov / (eo[:, None] - ev[None, :])
    d2 = ((eo[:, None, None, None] + eo[None, :, None, None]) - ev[None, None, :, None]) - ev[None, None, None, :]
    t2 = oovv / d2
    same = (so[:, None] == so[None, :])[:, :, None, None]
    pair = 0.25 * t2 * oovv
    dens = t1.T @ t1 + 0.5 * np.einsum("ijac,ijbc->ab", t2, t2)
    dens = uv @ dens @ uv.T
    dvv = [dens[np.ix_(np.flatnonzero(sv == s), np.flatnonzero(sv == s))] for s in (0, 1)]
    return MP2Result(e_hf, np.sum(fov * t1), np.sum(pair * same), np.sum(pair * ~same), dvv)


# ---------------------------------------------------------------------------------------------------- device solver
def memory_plan(no: int, nv: int, naux: int | None = None, capacity: int | None = None) -> dict:
    """Host arithmetic, before anything is allocated: the bytes ``solve_scf`` needs for one spin pair of ``no``
    occupied and ``nv`` virtual orbitals per spin.  ``row_bytes``: one occupied index i of the (ia|jb) block and of the
    amplitudes (the two tensors the pair kernel reads and writes); ``fixed_bytes``: what does not shrink with the
    slice -- the two v x v densities and, on a factor of ``naux`` vectors, both M_L = C_o^T B_L C_v; ``total_bytes``
    the unsliced need.  With a ``capacity`` in bytes, ``rows`` is the number of occupied indices one slice takes
    (``no`` = no slicing; at least 1) and ``slices`` their count.  On a factor a row also counts the copy of the
    slice's rows of M_L.  NOT counted: the work space of ``ao2mo`` on the tensor route (the backend sizes it per call,
    from the AO dimension the plan does not know) and the o x o, v x v and N x v matrices of the semicanonicalisation;
    ``MEMORY_FRACTION`` of the free memory as the default capacity is the headroom left for them."""
    no, nv = int(no), int(nv)
    row = 2 * 8 * nv * no * nv + (0 if naux is None else 8 * int(naux) * nv)
    fixed = 2 * 8 * nv * nv + (0 if naux is None else 2 * 8 * int(naux) * no * nv)
    plan = {"row_bytes": row, "fixed_bytes": fixed, "total_bytes": fixed + no * row, "rows": no, "slices": 1 if no else 0}
    if capacity is not None and no > 0:
        rows = max(1, min(no, (int(capacity) - fixed) // row if row else no))
        plan["rows"], plan["slices"] = rows, -(-no // rows)
    return plan


def _spin_orbitals(scf_method):
    """(restricted, C (2, N, n), occupied masks (2, n)) of an SCF object; a restricted one gives C twice."""
    restricted = is_restricted(scf_method)
    c = np.asarray(scf_method.mo_coeff, dtype=float)
    mo_occ = np.asarray(scf_method.mo_occ)
    if restricted:
        if np.any((mo_occ > 0) != (mo_occ > 1)):
            raise ValueError("a restricted object with singly occupied orbitals has no MP2 here")
        return True, np.array([c, c]), np.array([mo_occ > 0, mo_occ > 0])
    return False, c, mo_occ > 0


def _ao_fock(scf_method):
    f = np.asarray(scf_method.get_fock(), dtype=float)
    return np.array([f, f]) if f.ndim == 2 else f


def _scf_energy(scf_method) -> float:
    e = getattr(scf_method, "e_tot", None)
    return float(scf_method.energy_tot() if e is None else e)


class _Integrals:
    """(ia|jb) blocks of an SCF object on the device: from (pq|rs) by ``ao2mo``, or from a factor B by
    M_L = C_o^T B_L C_v (two batched gemms) and one gemm over L -- (pq|rs) is then never asked for."""

    def __init__(self, scf_method, be):
        from .ham_builder import _ao_eri_device, _ao_eri_factor_device

        self.be = be
        self.factor = _ao_eri_factor_device(scf_method, be, None)
        self.eri = None if self.factor is not None else _ao_eri_device(scf_method, be)
        self.naux = None if self.factor is None else int(self.factor.shape[0])
        self._m = {}

    def half(self, key, co, cv):
        """M[L, i, a] of one spin, made once."""
        if key not in self._m:
            be = self.be
            self._m[key] = be.gemm(be.gemm(co, self.factor, "T", "N"), cv)
        return self._m[key]

    def block(self, k1, co1, cv1, k2, co2, cv2, i0, i1):
        """V[i, a, j, b] for i in [i0, i1), contiguous (i1 - i0, nv1, no2, nv2)."""
        be = self.be
        if self.factor is None:
            return be.ao2mo(self.eri, co1, cv1, co2, cv2, i0, i1)
        m1, m2 = self.half(k1, co1, cv1), self.half(k2, co2, cv2)
        rows = m1 if (i0, i1) == (0, m1.shape[1]) else m1[:, i0:i1, :].contiguous()
        naux = self.naux
        v = be.gemm(rows.reshape(naux, -1), m2.reshape(naux, -1), "T", "N")
        return v.reshape(i1 - i0, m1.shape[2], m2.shape[1], m2.shape[2])


def solve_scf(scf_method, backend=None, virtuals=None, capacity: int | None = None) -> MP2Result:
    """MP2 of the determinant of an SCF object (``mo_coeff``, ``mo_occ``, ``get_fock``, the integrals) on the device:
    f = C^T get_fock() C per spin, semicanonicalised by rotating the coefficient matrices (``eigh`` of the o x o and
    v x v blocks), the (ia|jb) block of each spin pair from ``ao2mo`` or from the object's factor, amplitudes and pair
    energies from ``mp2_pairs``, the densities from ``gemm`` on the amplitudes as the kernel leaves them; the singles
    term (o x v numbers) on the host.  ``virtuals``: per spin (one matrix for a restricted object) AO coefficients
    that span the virtual space to correlate in, instead of the object's own unoccupied columns.  ``capacity``: bytes
    to plan with (default: ``MEMORY_FRACTION`` of the free device memory); a spin pair whose block does not fit
    (``memory_plan``) is walked in slices over i."""
    be = backend if backend is not None else (getattr(scf_method, "be", None) or get_backend())
    if not hasattr(be, "mp2_pairs"):
        raise ValueError(f"the {getattr(be, 'name', type(be).__name__)} backend has no mp2_pairs")
    restricted, c, occ = _spin_orbitals(scf_method)
    fock = _ao_fock(scf_method)
    if virtuals is not None:
        virtuals = [np.asarray(virtuals, dtype=float)] * 2 if restricted else [np.asarray(v, dtype=float) for v in virtuals]
    ints = _Integrals(scf_method, be)
    if capacity is None:
        free = getattr(be, "free_bytes", None)
        capacity = int(MEMORY_FRACTION * free()) if free is not None else None

    spins = (0,) if restricted else (0, 1)
    co, cv, eo, ev, uv, dens, e_singles = {}, {}, {}, {}, {}, {}, 0.0
    for s in spins:
        f_d = be.asarray(fock[s])
        co_in = be.asarray(c[s][:, occ[s]])
        cv_in = be.asarray(virtuals[s] if virtuals is not None else c[s][:, ~occ[s]])
        no, nv = int(co_in.shape[1]), int(cv_in.shape[1])
        eo[s] = ev[s] = uv[s] = None
        co[s], cv[s] = co_in, cv_in
        if no:
            eo[s], uo = be.eigh(be.gemm(be.gemm(co_in, f_d, "T", "N"), co_in))
            co[s] = be.gemm(co_in, uo)
        if nv:
            ev[s], uv[s] = be.eigh(be.gemm(be.gemm(cv_in, f_d, "T", "N"), cv_in))
            cv[s] = be.gemm(cv_in, uv[s])
        t1t1 = np.zeros((nv, nv))
        if no and nv:  # the singles term: o x v numbers, on the host
            fov = be.to_host(be.gemm(be.gemm(co[s], f_d, "T", "N"), cv[s]))
            t1 = fov / (be.to_host(eo[s])[:, None] - be.to_host(ev[s])[None, :])
            e_singles += float(np.sum(fov * t1)) * (2.0 if restricted else 1.0)
            t1t1 = t1.T @ t1
        dens[s] = be.asarray(t1t1)

    def pair(s1, s2, kinds):
        """Energies of the block (s1 s1|s2 s2), one per entry of ``kinds`` (True: the same-spin amplitudes of the block,
        False: the opposite-spin ones); the amplitudes' contributions go to ``dens``.  A restricted object asks for both
        kinds of its one block, which is transformed once per slice."""
        no1, nv1, no2, nv2 = int(co[s1].shape[1]), int(cv[s1].shape[1]), int(co[s2].shape[1]), int(cv[s2].shape[1])
        energy = [0.0] * len(kinds)
        if not (no1 and nv1 and no2 and nv2):
            return energy
        rows = min(no1, memory_plan(max(no1, no2), max(nv1, nv2), ints.naux, capacity)["rows"])
        for i0 in range(0, no1, rows):
            i1 = min(no1, i0 + rows)
            v = ints.block(s1, co[s1], cv[s1], s2, co[s2], cv[s2], i0, i1)
            for n, same in enumerate(kinds):
                t, e = be.mp2_pairs(v, eo[s1][i0:i1].contiguous(), ev[s1], eo[s2], ev[s2], same)
                energy[n] += float(be.to_host(e).reshape(-1)[0])
                tm = t.reshape(nv1, -1)
                be.gemm(tm, tm, "N", "T", alpha=0.5 if same else 1.0, beta=1.0, out=dens[s1])
                if not same and not restricted:
                    tm = t.reshape(-1, nv2)
                    be.gemm(tm, tm, "T", "N", alpha=1.0, beta=1.0, out=dens[s2])
                del t
            del v
        return energy

    if restricted:
        e_aa, e_opposite = pair(0, 0, (True, False))
        e_same = 2.0 * e_aa
    else:
        e_same = pair(0, 0, (True,))[0] + pair(1, 1, (True,))[0]
        e_opposite = pair(0, 1, (False,))[0]
    dvv = []
    for s in spins:  # back to the input virtual basis
        d = dens[s]
        if uv[s] is not None:
            d = be.gemm(be.gemm(uv[s], d), uv[s], "N", "T")
        dvv.append(be.to_host(d))
    if restricted:
        dvv = [dvv[0], dvv[0].copy()]
    return MP2Result(_scf_energy(scf_method), e_singles, e_same, e_opposite, dvv)


# ---------------------------------------------------------------------------------------------------- frozen natural orbitals
def frozen_natural_orbitals(scf_method, n_frozen_virt: int | None = None, threshold: float | None = None, backend=None,
                            capacity: int | None = None):
    """``(scf_reduced, info)``: a copy of the SCF object whose columns are the occupied ones, untouched, followed by
    the canonicalised kept MP2 natural virtual orbitals.  Per spin: the eigenpairs of D^s sorted by (-occupation,
    index), the first nv - k eigenvectors kept and rotated among themselves so that f_vv is diagonal in the kept
    space (``mo_energy`` holds those eigenvalues).  Exactly one selector: ``n_frozen_virt`` = k virtuals dropped per
    spin, or an occupation ``threshold`` -- both spins then drop the same number, the smaller of the two spins' counts
    of occupations below the threshold, and every spin keeps at least one virtual.  A spin without an occupied orbital
    (D^s = 0) keeps its lowest-e_a virtuals.  ``info``: ``n_virtual``, ``n_kept`` (ints, or per-spin tuples where the
    spins differ), ``n_frozen_virt`` (the k that was applied), ``occupations`` (per spin, descending), ``e_mp2_full``,
    ``e_mp2_kept`` and ``e_correction`` = E(2)[all virtuals] - E(2)[kept virtuals], which is NOT added to anything
    here, and ``mp2``, the ``MP2Result`` of the full virtual space."""
    if (n_frozen_virt is None) == (threshold is None):
        raise ValueError("frozen_natural_orbitals: give n_frozen_virt or threshold, one of the two")
    be = backend if backend is not None else (getattr(scf_method, "be", None) or get_backend())
    restricted, c, occ = _spin_orbitals(scf_method)
    spins = (0,) if restricted else (0, 1)
    nvirt = [int(np.sum(~occ[s])) for s in (0, 1)]
    if n_frozen_virt is not None:
        k = int(n_frozen_virt)
        if k < 0:
            raise ValueError("frozen_natural_orbitals: n_frozen_virt must not be negative")
        if k >= min(nvirt):
            logger.error("Attempting to reduce the virtual space by more than exist.")
            raise ValueError("Atempting to reduce virtual space by more than exist.")
    full = solve_scf(scf_method, be, capacity=capacity)
    fock = _ao_fock(scf_method)

    vectors, occupations = {}, {}
    for s in spins:
        nv = nvirt[s]
        cv_d, f_d = be.asarray(c[s][:, ~occ[s]]), be.asarray(fock[s])
        if np.any(occ[s]):
            w, u = (be.to_host(x) for x in be.eigh(be.asarray(full.dvv[s])))
            order = np.lexsort((np.arange(nv), -w))
        else:  # D = 0: the lowest-e_a virtuals, stable
            e, u = (be.to_host(x) for x in be.eigh(be.gemm(be.gemm(cv_d, f_d, "T", "N"), cv_d)))
            w, order = np.zeros(nv), np.argsort(e, kind="stable")
        vectors[s], occupations[s] = u[:, order], w[order]
    if restricted:
        vectors[1], occupations[1] = vectors[0], occupations[0]
    if threshold is not None:
        k = min(nvirt[s] - int(np.sum(occupations[s] >= float(threshold))) for s in (0, 1))
        k = max(0, min(k, min(nvirt) - 1))
    kept = [nvirt[s] - k for s in (0, 1)]

    new_c, new_e, new_occ, fno = {}, {}, {}, {}
    mo_energy = getattr(scf_method, "mo_energy", None)
    mo_energy = None if mo_energy is None else np.asarray(mo_energy, dtype=float)
    for s in spins:
        cv_d, f_d = be.asarray(c[s][:, ~occ[s]]), be.asarray(fock[s])
        ck = be.gemm(cv_d, be.asarray(vectors[s][:, : kept[s]]))
        e, u = be.eigh(be.gemm(be.gemm(ck, f_d, "T", "N"), ck))  # canonicalise inside the kept space
        fno[s] = be.to_host(be.gemm(ck, u))
        c_occ = c[s][:, occ[s]]
        new_c[s] = np.concatenate([c_occ, fno[s]], axis=1)
        if mo_energy is not None and mo_energy.shape == np.asarray(scf_method.mo_occ).shape:
            e_occ = (mo_energy if restricted else mo_energy[s])[occ[s]]
        else:
            e_occ = np.einsum("pi,pq,qi->i", c_occ, fock[s], c_occ)
        new_e[s] = np.concatenate([e_occ, be.to_host(e)])
        old = np.asarray(scf_method.mo_occ) if restricted else np.asarray(scf_method.mo_occ)[s]
        new_occ[s] = np.concatenate([old[occ[s]], np.zeros(kept[s], dtype=old.dtype)])

    reduced = scf_method.copy()
    if restricted:
        reduced.mo_coeff, reduced.mo_energy, reduced.mo_occ = new_c[0], new_e[0], new_occ[0]
        fno[1] = fno[0]
    else:
        if new_c[0].shape != new_c[1].shape:
            raise ValueError("frozen_natural_orbitals: the two spins must keep the same number of orbitals")
        reduced.mo_coeff = np.array([new_c[0], new_c[1]])
        reduced.mo_energy = np.array([new_e[0], new_e[1]])
        reduced.mo_occ = np.array([new_occ[0], new_occ[1]])
    small = solve_scf(scf_method, be, virtuals=fno[0] if restricted else (fno[0], fno[1]), capacity=capacity)

    def both(x):
        return int(x[0]) if x[0] == x[1] else (int(x[0]), int(x[1]))

    occs = [occupations[0], occupations[1]]
    info = {
        "n_virtual": both(nvirt), "n_kept": both(kept), "n_frozen_virt": int(k),
        "occupations": np.array(occs) if nvirt[0] == nvirt[1] else occs,
        "e_mp2_full": full.e_corr, "e_mp2_kept": small.e_corr, "e_correction": full.e_corr - small.e_corr,
        "mp2": full,
    }
    return reduced, info
