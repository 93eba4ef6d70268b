"""Reference for the device FCI (nbed_amd/fci_gpu.py) that shares nothing with it: synthetic Hamiltonians with the
symmetries of real integrals, and rows of the Hamiltonian matrix taken straight from the operator definition

    H = constant + sum h1[P,R] a+_P a_R + sum h2[P,Q,R,S] a+_P a+_Q a_R a_S

(spin orbital 2p + s, the 1/2 in h2) -- no generators, no link tables.  The determinant basis is the device solver's:
determinant (Ia, Ib) = alpha creators in ascending order, then beta creators in ascending order, on the vacuum; strings
in the order of itertools.combinations; index Ia * Nb + Ib.  No GPU needed."""

import itertools

import numpy as np

from nbed_amd.ham_builder import SpatialHamiltonian

EPS = np.finfo(float).eps


def synthetic(n: int, seed: int) -> SpatialHamiltonian:
    """(pq|rs)^{st} = sum_L B^s_L,pq B^t_L,rs with B symmetric in pq and scaled by 1/n, alpha != beta;
    two_body[x][p,q,r,s] = 1/2 (ps|qr); one symmetric random one_body per spin: random levels about one apart on the
    diagonal and couplings a sixth of that off it, so that -- as with molecular orbitals -- one determinant dominates
    the ground state and a Davidson iteration started from it has something to converge to."""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((2, n + 1, n, n)) / n
    b = 0.5 * (b + b.transpose(0, 1, 3, 2))
    chem = {(s, t): np.einsum("lpq,lrs->pqrs", b[s], b[t]) for s, t in ((0, 0), (1, 1), (0, 1))}
    two = np.stack([0.5 * chem[k].transpose(0, 2, 3, 1) for k in ((0, 0), (1, 1), (0, 1))])  # [p,q,r,s] = (ps|qr) / 2
    one = rng.standard_normal((2, n, n)) / 6.0
    one = 0.5 * (one + one.transpose(0, 2, 1))
    one[:, np.arange(n), np.arange(n)] = np.arange(n) + 0.3 * rng.standard_normal((2, n))
    return SpatialHamiltonian(0.25 + 0.5 * rng.random(), np.ascontiguousarray(one), np.ascontiguousarray(two))


class Sector:
    """The determinants of n orbitals with (na, nb) electrons: string masks by rank and back."""

    def __init__(self, n, nelec):
        self.n, (self.na, self.nb) = n, (int(nelec[0]), int(nelec[1]))
        self.str_a = [sum(1 << p for p in occ) for occ in itertools.combinations(range(n), self.na)]
        self.str_b = [sum(1 << p for p in occ) for occ in itertools.combinations(range(n), self.nb)]
        self.rank_a = {m: i for i, m in enumerate(self.str_a)}
        self.rank_b = {m: i for i, m in enumerate(self.str_b)}
        self.shape = (len(self.str_a), len(self.str_b))
        self.ndet = len(self.str_a) * len(self.str_b)

    def mask(self, index):
        """Occupation of determinant ``index`` with bit p for alpha orbital p and bit n + p for beta orbital p."""
        ia, ib = divmod(int(index), len(self.str_b))
        return self.str_a[ia] | (self.str_b[ib] << self.n)

    def index(self, mask):
        return self.rank_a[mask & ((1 << self.n) - 1)] * len(self.str_b) + self.rank_b[mask >> self.n]


def _pos(P, n):
    """Bit of spin orbital P = 2p + s in Sector.mask: alpha first."""
    return (P >> 1) + (P & 1) * n


def _remove(det, bit):
    """a_bit |det> -> (sign, det'); the caller knows the bit is set."""
    return (-1 if bin(det & ((1 << bit) - 1)).count("1") & 1 else 1), det & ~(1 << bit)


def _add(det, bit):
    return (-1 if bin(det & ((1 << bit) - 1)).count("1") & 1 else 1), det | (1 << bit)


def row(ham: SpatialHamiltonian, nelec, index: int, sector: Sector | None = None) -> dict:
    """{J: H_IJ} for I = ``index``, the non-zero elements only.  <I| a+_P a+_Q a_R a_S |J> needs P, Q in I and R, S
    outside I - P - Q; then J = I - P - Q + R + S and the sign is what the four operators collect acting on J."""
    n = ham.n
    sec = sector or Sector(n, nelec)
    det = sec.mask(index)
    spin_orbitals = range(2 * n)
    occ = [P for P in spin_orbitals if (det >> _pos(P, n)) & 1]
    out = {index: float(ham.constant)}
    for P in occ:
        rest = det & ~(1 << _pos(P, n))
        for R in spin_orbitals:
            if (P ^ R) & 1 or (rest >> _pos(R, n)) & 1:
                continue
            v = float(ham.one_body[P & 1][P >> 1, R >> 1])
            if v == 0.0:
                continue
            ket = rest | (1 << _pos(R, n))
            s1, mid = _remove(ket, _pos(R, n))
            s2, bra = _add(mid, _pos(P, n))
            assert bra == det
            j = sec.index(ket)
            out[j] = out.get(j, 0.0) + s1 * s2 * v
    for P in occ:
        for Q in occ:
            if P == Q:
                continue
            rest = det & ~(1 << _pos(P, n)) & ~(1 << _pos(Q, n))
            for R in spin_orbitals:
                if (rest >> _pos(R, n)) & 1:
                    continue
                for S in spin_orbitals:
                    if S == R or (rest >> _pos(S, n)) & 1:
                        continue
                    v = ham.h2_element(P, Q, R, S)
                    if v == 0.0:
                        continue
                    ket = rest | (1 << _pos(R, n)) | (1 << _pos(S, n))
                    s1, d1 = _remove(ket, _pos(S, n))
                    s2, d2 = _remove(d1, _pos(R, n))
                    s3, d3 = _add(d2, _pos(Q, n))
                    s4, bra = _add(d3, _pos(P, n))
                    assert bra == det
                    j = sec.index(ket)
                    out[j] = out.get(j, 0.0) + s1 * s2 * s3 * s4 * v
    return out


def dense(ham: SpatialHamiltonian, nelec) -> np.ndarray:
    """The whole matrix from ``row``: for up to a few hundred determinants."""
    sec = Sector(ham.n, nelec)
    mat = np.zeros((sec.ndet, sec.ndet))
    for i in range(sec.ndet):
        for j, v in row(ham, nelec, i, sec).items():
            mat[i, j] = v
    return mat


def row_dot(ham, nelec, index, c, sector=None) -> float:
    """(H c)_I from ``row``."""
    flat = np.asarray(c).reshape(-1)
    return float(sum(v * flat[j] for j, v in row(ham, nelec, index, sector).items()))


def sigma_tolerance(ham: SpatialHamiltonian, nelec, cmax: float) -> float:
    """Per-element bound on a device sigma: (4n^2 + 8) eps s^2 M max|c| with s = na (n - na + 1) + nb (n - nb + 1) the
    non-zeros of a column of D and M = max|one_body| + 2 (n + 1) max|two_body| a bound on every effective integral --
    the standard bound for a length-2n^2 dot product inside a 2n^2-term sum."""
    n, (na, nb) = ham.n, nelec
    s = na * (n - na + 1) + nb * (n - nb + 1)
    m = np.abs(ham.one_body).max() + 2 * (n + 1) * np.abs(ham.two_body).max()
    return (4 * n * n + 8) * EPS * s * s * m * cmax
