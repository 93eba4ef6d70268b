"""Shared by tests/test_host_eigh_cases.py (CPU) and tests/test_gpu_eigh.py (MI355X): operands with controlled spectra,
a certified extended-precision reference that can take clusters, and error bounds for the symmetric eigensolvers
(nbx_eigh / nbx_eigh_warm_ex / nbx_eigh_approx: nbed_amd/csrc/eigh.hip, eigh_lds.hip, eigh_tridiag.hip, eigh_grid.hip,
eigh_refine.hip).  householder_q, jittered_grid, compose, EPS, LD, CERTIFICATE and worst_ratio are matfn_cases'.

Spectra (nrm = max |l|; every modification is applied to jittered_grid(-12, 10, n) and the levels sorted again; one
with a size guard applies from that n on, below it the grid stays as it is).

  spread              the grid
  pairs    (n >= 8)   three close pairs, l[i+1] = l[i] + g 12 with g = 1e-6, 1e-9, 1e-11 at i = n//5, n//2, n-2
  cluster  (n >= 24)  an exactly degenerate level of multiplicity min(12, n//4) from index n//3 on (`mult` widens it),
                      and a triple spaced by 12e-13 at indices 2..4
  graded   (n >= 8)   the top three levels are 1.0e6, 1.1e6, 1.3e6: the mu-shifted Fock matrix
  overlap             logspace(-4, 0, n): positive definite, kappa = 1e4

A = Q diag(l) Q^T is formed in longdouble from three Householder reflectors, symmetrised and rounded to float64.

Groups.  Levels closer than GROUP = 1e-7 nrm to a neighbour form one group; everything about VECTORS is judged per
group (the projector on the group's invariant subspace), so that nothing is ill-posed and nothing is left out: a group
of one is the single vector, sign-free.

Reference.  It is the reference of the ROUNDED matrix.  refine_grouped is matfn_cases.refine (Ogita-Aishima in
longdouble: R = I - X^T X, S = X^T A X, l_i = s_ii / (1 - r_ii), X <- X (I + E)) with one change: for i, j in the same
group E_ij = r_ij / 2 (the paper's rule for multiple eigenvalues: restore orthonormality, leave the basis of the
subspace alone), and E_ij = (s_ij + l_j r_ij) / (l_j - l_i) only ACROSS groups.  Its certificate is max |I - X^T X| and
max |S_ij| over pairs in DIFFERENT groups, held to CERTIFICATE (x nrm).  Reference eigenvalues: the Rayleigh quotient
for a group of one; inside a group of k > 1 the mean of the group's k x k block of S plus the float64 eigenvalues of
(block - mean): the block's spread is O(eps ||A||) or the chosen 1e-9 .. 1e-13 nrm, so float64 is exact enough there.

The kernels' constants, restated.

  ACCEPT = 1e-13   the off-diagonal weight max |offdiag V^T A V| / max |diag| up to which the tridiagonal route is
                   accepted: quality_status_kernel (eigh_tridiag.hip:972, device verdict, 64 <= N <= 196) and
                   nbx_eigh_warm_ex (eigh.hip:383, host verdict, N > 196).  It is the LOOSEST stopping rule of all
                   routes: the Jacobi kernels rotate until a_pq^2 <= eps^2 |a_pp a_qq| (eigh_lds.hip:200), and the
                   refinement accepts at max |E| < RF_TOL = 3e-8 (eigh_refine.hip:45), which leaves ~RF_TOL^2 = 9e-16.
  GRAM = 1e-6      the Gram defect of the inverse-iteration vectors up to which ONE Newton-Schulz step
                   V <- V (3 I - V^T V) / 2 is taken (eigh_tridiag.hip:969, :1035, :927): it leaves 0.75 GRAM^2.
  u = N eps        the backward-error model of matfn_cases (eps = 2^-52).

Bounds, one set for every route (none is fitted to a kernel).

  eigenvalues      |w_i - l_i^ref| <= (ACCEPT + u) nrm
  residual         max |A V - V diag(w)| <= (u + sqrt(N) ACCEPT) nrm, in longdouble: a column of V^T A V - diag has N
                   entries of at most ACCEPT nrm, hence a 2-norm of at most sqrt(N) ACCEPT nrm, and V is orthonormal
  orthonormality   max |V^T V - I| <= 0.75 GRAM^2 + u, in longdouble
  subspaces        for every group g at distance gamma_g from the nearest level outside it
                   max |V_g V_g^T - X_g X_g^T| <= 2 (u + sqrt(N) ACCEPT) nrm / gamma_g + (0.75 GRAM^2 + u):
                   Davis-Kahan with the residual bound (sin theta <= residual / gamma, the projectors differ by at most
                   2 sin theta), plus the orthonormality defect of V_g
  order            w ascending; the operand bit-identical after the call (include/nbx.h: "d_a ... preserved")

Condition.  Every group of every case has a subspace bound below SUBSPACE_MAX = 1e-4 -- asserted when a case is
built -- which is what makes "every group is checked" mean something.

The three whole-chip instances a longdouble reference does not reach in seconds (N = 513, 1025) are built and judged in
float64: float64_operand and float64_ratios."""

from __future__ import annotations

import functools

import numpy as np

from matfn_cases import CERTIFICATE, EPS, LD, compose, householder_q, jittered_grid, worst_ratio  # noqa: F401

# ------------------------------------------------------------------ the kernels' constants, restated (module docstring)
ACCEPT = 1.0e-13     # eigh_tridiag.hip:972, eigh.hip:383
GRAM = 1.0e-6        # eigh_tridiag.hip:969, :1035, :927
RF_TOL = 3.0e-8      # eigh_refine.hip:45
GROUP = 1.0e-7       # x nrm: levels closer than this to a neighbour are judged together
SUBSPACE_MAX = 1.0e-4

SPECTRA = ("spread", "pairs", "cluster", "graded", "overlap")
PAIR_GAPS = (1.0e-6, 1.0e-9, 1.0e-11)
TRIPLE_STEP = 12.0e-13


# ------------------------------------------------------------------ spectra
def cluster_multiplicity(n: int) -> int:
    return min(12, n // 4)


def spectrum(name: str, n: int, seed: int, mult: int | None = None) -> np.ndarray:
    """The n ascending levels of the named spectrum (module docstring)."""
    rng = np.random.default_rng(seed)
    if name == "overlap":
        return np.logspace(-4.0, 0.0, n)
    lam = jittered_grid(-12.0, 10.0, n, rng)
    if name == "pairs" and n >= 8:
        for g, i in zip(PAIR_GAPS, (n // 5, n // 2, n - 2)):
            lam[i + 1] = lam[i] + g * 12.0
    elif name == "cluster" and n >= 24:
        m = cluster_multiplicity(n) if mult is None else mult
        assert 2 <= m <= n // 2
        lam[n // 3:n // 3 + m] = lam[n // 3]
        lam[3] = lam[2] + TRIPLE_STEP
        lam[4] = lam[2] + 2.0 * TRIPLE_STEP
    elif name == "graded" and n >= 8:
        lam[n - 3:] = (1.0e6, 1.1e6, 1.3e6)
    elif name not in SPECTRA:
        raise ValueError(name)
    return np.sort(lam)


def groups_of(lam, nrm: float):
    """[(start, stop)] of the ascending levels lam: neighbours closer than GROUP nrm share a group."""
    lam = np.asarray(lam)
    cut = np.flatnonzero(np.diff(lam) >= GROUP * nrm) + 1
    edges = [0, *cut.tolist(), len(lam)]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:])]


def same_group_mask(n: int, groups) -> np.ndarray:
    """(n, n) bool: i != j in the same group."""
    same = np.zeros((n, n), dtype=bool)
    for a, b in groups:
        same[a:b, a:b] = True
    same[np.eye(n, dtype=bool)] = False
    return same


# ------------------------------------------------------------------ reference
def refine_grouped(a64: np.ndarray, x: np.ndarray, groups, steps: int = 3):
    """matfn_cases.refine with the rule for multiple eigenvalues inside a group (module docstring).
    -> (X, Rayleigh quotients, S = X^T A X, (max |I - X^T X|, max |S_ij| over i, j in different groups))."""
    a = np.asarray(a64, dtype=LD)
    n = a.shape[0]
    eye = np.eye(n, dtype=LD)
    off = ~np.eye(n, dtype=bool)
    same = same_group_mask(n, groups)
    cross = off & ~same
    for step in range(steps + 1):
        r = eye - x.T @ x
        s = x.T @ (a @ x)
        lam = np.diag(s) / (LD(1) - np.diag(r))
        if step == steps:
            break  # (the certificate is taken from R and S as computed)
        r, s = LD(0.5) * (r + r.T), LD(0.5) * (s + s.T)  # (matfn_cases.refine: why)
        d = lam[None, :] - lam[:, None]
        d[~cross] = LD(1)
        e = (s + lam[None, :] * r) / d
        e[same] = r[same] / LD(2)
        e[~off] = np.diag(r) / LD(2)
        x = x + x @ e
    cert = (float(np.max(np.abs(r))), float(np.max(np.abs(s[cross]))) if cross.any() else 0.0)
    return x, lam, s, cert


def group_eigenvalues(lam, s, groups) -> np.ndarray:
    """Reference eigenvalues in longdouble: Rayleigh quotients, and inside a group of k > 1 the mean of the k x k
    block of S plus the float64 eigenvalues of (block - mean)."""
    ref = np.array(lam, dtype=LD)
    for a, b in groups:
        if b - a > 1:
            blk = LD(0.5) * (s[a:b, a:b] + s[a:b, a:b].T)
            mean = np.trace(blk) / LD(b - a)
            ref[a:b] = mean + np.linalg.eigvalsh((blk - mean * np.eye(b - a, dtype=LD)).astype(np.float64)).astype(LD)
    return ref


class Bounds:
    def __init__(self, n: int, nrm: float):
        self.u = n * EPS
        self.eigenvalues = (ACCEPT + self.u) * nrm
        self.residual = (self.u + np.sqrt(n) * ACCEPT) * nrm
        self.orthonormality = 0.75 * GRAM**2 + self.u

    def subspace(self, gamma: float) -> float:
        return 2.0 * self.residual / gamma + self.orthonormality


class Case:
    """One rounded operand with its certified grouped reference."""

    def __init__(self, name: str, n: int, index: int = 0, mult: int | None = None):
        self.name, self.n, self.index, self.mult = name, n, index, mult
        seed = 1000003 * n + 1009 * SPECTRA.index(name) + 17 * index
        self.lam0 = spectrum(name, n, seed + 1, mult)
        self.q = householder_q(n, seed)
        self.nrm = float(np.max(np.abs(self.lam0)))
        self.groups = groups_of(self.lam0, self.nrm)
        self.a = compose(self.q, self.lam0)
        self.a.setflags(write=False)
        self.x, self.rayleigh, self.s, self.cert = refine_grouped(self.a, self.q, self.groups)
        self.lam = group_eigenvalues(self.rayleigh, self.s, self.groups)
        assert np.all(np.diff(self.lam) >= 0), (name, n, index)
        self.bounds = Bounds(n, self.nrm)
        self.gamma = []
        for a, b in self.groups:
            below = float(self.lam[a] - self.lam[a - 1]) if a > 0 else np.inf
            above = float(self.lam[b] - self.lam[b - 1]) if b < n else np.inf
            self.gamma.append(min(below, above))
        self.subspace_bounds = [self.bounds.subspace(g) for g in self.gamma]
        # the condition: every group can be told from its neighbours by a solver that meets the residual bound
        assert max(self.subspace_bounds) < SUBSPACE_MAX, (name, n, index, max(self.subspace_bounds))

    def ident(self) -> str:
        return f"{self.name}-N{self.n}[{self.index}]" + (f"-m{self.mult}" if self.mult else "")

    def ratios(self, w, v) -> dict:
        """error / bound of computed eigenpairs (w ascending, v columns) for the four bounds; NaN or inf: inf."""
        w, v = np.asarray(w), np.asarray(v)
        if not (np.all(np.isfinite(w)) and np.all(np.isfinite(v))):
            return dict.fromkeys(("eigenvalues", "residual", "orthonormality", "subspace"), float("inf"))
        b = self.bounds
        vl, wl = v.astype(LD), w.astype(LD)
        res = self.a.astype(LD) @ vl - vl * wl[None, :]
        gram = vl.T @ vl - np.eye(self.n, dtype=LD)
        sub = 0.0
        for (lo, hi), bound in zip(self.groups, self.subspace_bounds):
            got = vl[:, lo:hi] @ vl[:, lo:hi].T
            ref = self.x[:, lo:hi] @ self.x[:, lo:hi].T
            sub = max(sub, float(np.max(np.abs(got - ref))) / bound)
        return {
            "eigenvalues": worst_ratio(w, self.lam, b.eigenvalues),
            "residual": float(np.max(np.abs(res))) / b.residual,
            "orthonormality": float(np.max(np.abs(gram))) / b.orthonormality,
            "subspace": sub,
        }


@functools.lru_cache(maxsize=None)
def case(name: str, n: int, index: int = 0, mult: int | None = None) -> Case:
    return Case(name, n, index, mult)


# ------------------------------------------------------------------ case tables
# | : the LDS Jacobi solver | the register tridiagonal route, verdict on the device | verdict on the host, one workgroup
# | the whole-chip reduction (tdg_kernel<2,2> up to 256, <4,2> at 257; invit_lds_kernel ends at IVL_MAX_N = 208)
COLD_SIZES = [2, 3, 37, 63, 64, 65, 128, 129, 150, 151, 176, 177, 196, 197, 198, 199, 208, 209, 257]
ALL_SPECTRA_SIZES = [37, 150, 196, 198, 257]
COLD_CASES = [(n, name) for n in COLD_SIZES for name in (SPECTRA if n in ALL_SPECTRA_SIZES else SPECTRA[:2])]
BATCH_ONE_SIZES = [199, 230]          # tdg_kernel<2,1>
# the multiplicity of the clustered matrix at N = 150 is the one at which the device verdict rejects it
# (tests/test_gpu_eigh.py::test_mixed_batch_device_verdict says which was needed)
MIXED_150_MULT = None
MIXED = {150: (("spread", 0, None), ("cluster", 1, MIXED_150_MULT), ("pairs", 2, None)),
         230: (("spread", 0, None), ("cluster", 1, None))}
# ... and at N = 230 the host verdict accepts the table's multiplicity 12; with 20 it rejects the clustered matrix and
# sends the whole batch, the well separated neighbour included, to the polisher: run in ADDITION to the batch above
MIXED_230_REJECTED = (("spread", 0, None), ("cluster", 1, 20))
WARM_SIZES = [37, 148, 196, 230]
WARM_SPECTRA = SPECTRA[:3]
APPROX_SIZES = [37, 150, 230]
FLOAT64_CASES = [(513, 1), (513, 2), (1025, 1)]  # tdg_kernel<4,1>, <8,2>, <8,1>
FLOAT64_SPECTRA = ("pairs", "cluster")


def all_case_keys():
    """Every (name, n, index, mult) the GPU test builds a longdouble reference for."""
    keys = []
    for n, name in COLD_CASES:
        keys += [(name, n, 0, None), (name, n, 1, None)]
    for n in BATCH_ONE_SIZES:
        keys += [(name, n, 0, None) for name in SPECTRA[:2]]
    for n, members in MIXED.items():
        keys += [(name, n, index, mult) for name, index, mult in members]
    keys += [(name, 230, index, mult) for name, index, mult in MIXED_230_REJECTED]
    for n in WARM_SIZES:
        keys += [(name, n, index, None) for name in WARM_SPECTRA for index in (0, 1)]
    for n in APPROX_SIZES:
        keys += [(name, n, index, None) for name in SPECTRA for index in (0, 1)]
    return sorted(set(keys), key=lambda k: (k[1], SPECTRA.index(k[0]), k[2], k[3] or 0))


def expected_group_sizes(name: str, n: int, mult: int | None = None):
    """The intended groups of a spectrum as a sorted list of the sizes above one, or None where the grouping follows
    from the grid (graded: nrm = 1.3e6 puts grid levels closer than 0.13 together)."""
    if name == "pairs" and n >= 8:
        return [2, 2]  # the 1e-6 pair is two levels; the 1e-9 and the 1e-11 pair are one group each
    if name == "cluster" and n >= 24:
        return sorted([3, cluster_multiplicity(n) if mult is None else mult])
    if name == "graded" and n >= 8:
        return None
    return []


# ------------------------------------------------------------------ the sizes judged in float64
def float64_operand(name: str, n: int, index: int = 0):
    """-> (A float64, levels): three float64 reflectors applied to diag(l) as rank-one updates, then symmetrised."""
    seed = 2000003 * n + 1009 * SPECTRA.index(name) + 17 * index
    lam = spectrum(name, n, seed + 1)
    rng = np.random.default_rng(seed)
    a = np.diag(lam)
    for _ in range(3):
        v = rng.standard_normal(n)
        v /= np.linalg.norm(v)
        p = a @ v
        k = float(v @ p)
        a = a - 2.0 * np.outer(v, p) - 2.0 * np.outer(p, v) + (4.0 * k) * np.outer(v, v)  # H A H, H = I - 2 v v^T
    a = np.ascontiguousarray(0.5 * (a + a.T))
    a.setflags(write=False)
    return a, lam


def float64_ratios(a, w, v) -> dict:
    """error / bound with float64 quantities only: eigenvalues against np.linalg.eigvalsh at (ACCEPT + 2 u) nrm
    (LAPACK's own u plus the device's), residual and orthonormality against the bounds above plus u nrm and u for
    the float64 evaluation.  No subspace check."""
    n = a.shape[-1]
    w_ref = np.linalg.eigvalsh(a)
    nrm = float(np.max(np.abs(w_ref)))
    b = Bounds(n, nrm)
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(v))):
        return dict.fromkeys(("eigenvalues", "residual", "orthonormality"), float("inf"))
    return {
        "eigenvalues": float(np.max(np.abs(w - w_ref))) / ((ACCEPT + 2.0 * b.u) * nrm),
        "residual": float(np.max(np.abs(a @ v - v * w[None, :]))) / (b.residual + b.u * nrm),
        "orthonormality": float(np.max(np.abs(v.T @ v - np.eye(n)))) / (b.orthonormality + b.u),
    }
