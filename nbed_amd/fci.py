"""Exact diagonalisation of a small second-quantised Hamiltonian (consumer of the path).

The reference computes the embedded FCI energy with PySCF's ``fci.FCI`` on the embedded SCF object
(nbed/driver.py:1044-1102) and checks that the Hamiltonian ``HamiltonianBuilder.build()`` returns has the
same ground state (tests/test_builder.py:55-120).  For active spaces of a few orbitals -- the
reference's own examples: 5-6 spatial orbitals -- the same number follows from diagonalising

    H = constant + sum_pq h1[p,q] a+_p a_q + sum_pqrs h2[p,q,r,s] a+_p a+_q a_r a_s

(the ``(constant, h1, h2)`` of ``build()``, spin orbitals interleaved alpha/beta, the 1/2 already in
h2) in the determinants with the embedded molecule's (n_alpha, n_beta).  Host code, dense, brute
force: meant for <= 16 spin orbitals.
"""

from __future__ import annotations

import itertools

import numpy as np

MAX_SPIN_ORBITALS = 16


class FCIResult:
    """Duck-typed stand-in for the solver object the reference reads ``.e_tot`` from."""

    def __init__(self, e_tot, energies, ci, dets, converged=True, norb=None, nelec=None):
        self.e_tot = float(e_tot)
        self.energies = energies
        self.ci = ci
        self.determinants = dets
        self.converged = converged
        self.norb = norb
        self.nelec = None if nelec is None else (int(nelec[0]), int(nelec[1]))

    # -- densities, by brute force from the operator definition, in the conventions of ``nbed_amd.fci_gpu``:
    #    dm1 (2,n,n)[s][p,q] = <b| a+_ps a_qs |c>,  dm2 (3,n,n,n,n)[x][p,q,r,s] = <b| a+_ps a+_qt a_rt a_ss |c> for
    #    (s,t) = aa, bb, ab -- the blocks and index order of ``SpatialHamiltonian.two_body``.
    def _root(self, root):
        if self.norb is None or self.nelec is None:
            raise ValueError("this FCIResult was made without norb and nelec: the density methods need both")
        ci = np.asarray(self.ci)
        ci = ci.reshape(ci.shape[0], -1)
        if not (isinstance(root, (int, np.integer)) and 0 <= root < ci.shape[1]):
            raise ValueError(f"root {root!r}: this result holds {ci.shape[1]} root(s)")
        return ci[:, int(root)]

    def _trans(self, i, j, two_particle):
        bra, ket = self._root(i), self._root(j)
        n, dets = self.norb, self.determinants
        index = {d: k for k, d in enumerate(dets)}
        dm1, dm2 = np.zeros((2, n, n)), np.zeros((3, n, n, n, n))
        for k, det in enumerate(dets):
            ck = ket[k]
            if ck == 0.0:
                continue
            occ = [P for P in range(2 * n) if (det >> P) & 1]
            for Q in occ:
                for P in range(Q & 1, 2 * n, 2):
                    sg, nd = _apply(det, (P,), (Q,))
                    if sg:
                        dm1[P & 1, P >> 1, Q >> 1] += sg * bra[index[nd]] * ck
            for S in occ if two_particle else ():
                for R in occ:
                    if R == S or (R & 1) < (S & 1):  # blocks aa, bb and ab: the spin of S is that of P, of R that of Q
                        continue
                    x = 2 if (R & 1) != (S & 1) else (S & 1)
                    s1, rest = _apply(det, (), (R, S))
                    for P in range(S & 1, 2 * n, 2):
                        if (rest >> P) & 1:
                            continue
                        for Q in range(R & 1, 2 * n, 2):
                            s2, nd = _apply(rest, (P, Q), ())
                            if s2:
                                dm2[x, P >> 1, Q >> 1, R >> 1, S >> 1] += s1 * s2 * bra[index[nd]] * ck
        return dm1, dm2

    def trans_rdm12(self, i, j):
        """(dm1, dm2) between roots i (bra) and j (ket)."""
        return self._trans(i, j, True)

    def trans_rdm1(self, i, j):
        return self._trans(i, j, False)[0]

    def rdm12(self, root=0):
        return self.trans_rdm12(root, root)

    def rdm1(self, root=0):
        return self._trans(root, root, False)[0]

    def spin_square(self, root=0) -> float:
        """<S^2> = S_z (S_z + 1) + n_beta - sum_pq dm2[ab][p,q,p,q]."""
        dm2 = self.rdm12(root)[1]
        sz = 0.5 * (self.nelec[0] - self.nelec[1])
        return float(sz * (sz + 1.0) + self.nelec[1] - np.einsum("pqpq->", dm2[2]))

    def natural_occupations(self, root=0) -> np.ndarray:
        """Eigenvalues of dm1[alpha] + dm1[beta], descending."""
        dm1 = self.rdm1(root)
        total = dm1[0] + dm1[1]
        return np.linalg.eigvalsh(0.5 * (total + total.T))[::-1].copy()


def _apply(det: int, creators, annihilators):
    """a+_{c0} a+_{c1} ... a_{a0} a_{a1} ... applied to the bit string ``det`` (rightmost acts first).
    Returns (sign, new_det) or (0, 0)."""
    sign = 1
    for a in reversed(annihilators):
        if not (det >> a) & 1:
            return 0, 0
        if bin(det & ((1 << a) - 1)).count("1") & 1:
            sign = -sign
        det &= ~(1 << a)
    for c in reversed(creators):
        if (det >> c) & 1:
            return 0, 0
        if bin(det & ((1 << c) - 1)).count("1") & 1:
            sign = -sign
        det |= 1 << c
    return sign, det


def ground_state(constant: float, h1: np.ndarray, h2: np.ndarray, nelec: tuple[int, int], nroots: int = 1) -> FCIResult:
    """Lowest eigenpair(s) of the Hamiltonian in the (n_alpha, n_beta) sector; alpha spin orbitals are
    the even indices (nbed/ham_builder.py:180-210)."""
    nq = h1.shape[0]
    if nq > MAX_SPIN_ORBITALS:
        raise ValueError(f"exact diagonalisation is limited to {MAX_SPIN_ORBITALS} spin orbitals (got {nq})")
    n = nq // 2
    na, nb = int(nelec[0]), int(nelec[1])
    dets = []
    for occ_a in itertools.combinations(range(n), na):
        for occ_b in itertools.combinations(range(n), nb):
            d = 0
            for p in occ_a:
                d |= 1 << (2 * p)
            for p in occ_b:
                d |= 1 << (2 * p + 1)
            dets.append(d)
    index = {d: i for i, d in enumerate(dets)}
    dim = len(dets)
    ham = np.zeros((dim, dim))
    one = [(p, q, h1[p, q]) for p, q in zip(*np.nonzero(h1))]
    two = [(p, q, r, s, h2[p, q, r, s]) for p, q, r, s in zip(*np.nonzero(h2))]
    for j, d in enumerate(dets):
        for p, q, v in one:
            sg, nd = _apply(d, (p,), (q,))
            if sg:
                ham[index[nd], j] += sg * v
        for p, q, r, s, v in two:
            sg, nd = _apply(d, (p, q), (r, s))
            if sg:
                i = index.get(nd)
                if i is not None:
                    ham[i, j] += sg * v
    ham = 0.5 * (ham + ham.T)
    w, c = np.linalg.eigh(ham)
    return FCIResult(w[0] + constant, w[:nroots] + constant, c[:, :nroots], dets, norb=n, nelec=(na, nb))
