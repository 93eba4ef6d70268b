"""Shared by tests/test_host_geig_cases.py (CPU) and tests/test_gpu_geig_refine.py (MI355X): pencils (F, S) with
controlled spectra, a certified extended-precision reference of the ROUNDED pencil, error bounds for the pencil
refinement nbx_geig_refine (nbed_amd/csrc/eigh_refine.hip) and a float64 twin of its E kernel.  householder_q,
jittered_grid, compose, EPS, LD, CERTIFICATE and worst_ratio are matfn_cases'; spectrum, groups_of, same_group_mask,
group_eigenvalues, GROUP, SUBSPACE_MAX and RF_TOL are eigh_cases'.

Pencils.  S = Qs diag(sigma) Qs^T with sigma = logspace(-log10 kappa, 0, n), kappa = 1e2 or 1e4, formed in longdouble
from three Householder reflectors, symmetrised and rounded to float64.  C = Qs diag(sigma^-1/2) Qs^T Q with a second
reflector product Q, and F = (S C) diag(l) (S C)^T in longdouble from the ROUNDED S, symmetrised and rounded; l is one
of eigh_cases' spectra spread, pairs, cluster, graded.  nrm = max |l|.

Reference.  eigh_cases.refine_grouped restated for the pencil: G = X^T S X, T = X^T F X, l_i = T_ii / G_ii, R = I - G,
E_ij = (T_ij + l_j R_ij) / (l_j - l_i) ACROSS groups, E_ij = R_ij / 2 inside a group and on the diagonal, X <- X (I + E),
all in longdouble, started from the longdouble C.  Certificate: max |I - G| <= CERTIFICATE max(1, max_ij xsx_ij) and
max |T_ij| over pairs in different groups <= CERTIFICATE nrm, asserted when a case is built (xsx below: the size of the
sums that make G; it is 12 at kappa = 1e2 and 1e3 at kappa = 1e4, where longdouble's own evaluation of G stops at 1e-17
.. 5e-17 however many steps are taken -- 4e3 times below the rounding term of the orthonormality bound).  Reference
eigenvalues: eigh_cases.group_eigenvalues of (l, T).

The kernel's constants, restated (refine_e_kernel, eigh_refine.hip).

  RF_TOL = 3e-8              :45   an accepted update has max |E| below this
  RF_GIVE_UP = 0.25          :46   max |E| from which the matrix is refused
  RF_CLUSTER_NOISE = 1e-14   :47   x ||T||_F: the coupling max |T_ij| tolerated between two levels that are NOT rotated
  RF_NOISE = 8 x 2^-53       :54   x sqrt(N) ||T||_F: numerators below it are "at noise", the second way to be accepted
  RF_NOISE_EMAX = 5e-7       :64   ... taken only with max |E| below this, by the pencil too; the pencil had a limit of
                                   its own, RF_NOISE_EMAX_PENCIL = 1e-3, until these tests (SHIPPED_NOISE_EMAX_PENCIL),
                                   and did not symmetrise G
  u = N eps                        the backward-error model of matfn_cases (eps = 2^-52)

Bounds (none is fitted to a kernel).  X, l: the reference; |.|: entry by entry; xsx = |X|^T |S| |X|, xfx = |X|^T |F| |X|:
the solver has to form G and T as two N-term products each, C^T (C^T S)^T and C^T (C^T F)^T, whose float64 evaluation
has the forward bounds 2 u xsx and 2 u xfx.  W_i = sum_k |l_k - l_i| <= N (l_max - l_min).

  orthonormality   max |C^T S C - I| <= N RF_TOL^2 + 2 u max_ij xsx_ij.  The update C (I + E) with E + E^T = R loses
                   (E^T E)_ij = sum_k E_ki E_kj: N products of two entries below RF_TOL; the second term is the
                   rounding of G itself, below which no fixed point of the iteration can sit.  (With kappa it grows:
                   |X| carries sigma^-1/2.  A flat u sqrt(kappa) is too small.)
  eigenvalues      |w_i - l_i| <= RF_TOL^2 W_i + 2 u (xfx_ii + |l_i| xsx_ii).  w_i is the Rayleigh quotient T_ii / G_ii
                   of the vectors BEFORE the accepted update, x_i + sum_k E_ki x_k: it is off by
                   sum_k E_ki^2 (l_k - l_i) -- the "N RF_TOL^2 nrm" of a first-order method with the levels' own
                   distances -- plus the rounding of T_ii and of l_i G_ii.
  residual         C-PROJECTED: M = C^T F C - C^T S C diag(w), in longdouble,
                   |M_ij| <= 3 RF_TOL^2 max(W_i, W_j) + RF_CLUSTER_NOISE ||l||_2 [i != j] + 2 u (xfx_ij + |l_j| xsx_ij).
                   After C <- C (I + E) the first-order terms of M cancel by the definition of E; what is left are three
                   sums over k of two entries of E times a level distance from i or j (E^T N, N E, E^T diag(l - l_j) E;
                   N the first-order residual); a pair the kernel does not rotate keeps its coupling, accepted up to
                   RF_CLUSTER_NOISE ||T||_F with ||T||_F = ||l||_2 in an S-orthonormal basis; and T, G carry their
                   rounding.  The diagonal M_jj = (l'_j - w_j) G_jj is covered by the same terms.
  subspaces        for every group g at distance gamma_g from the nearest level outside it, with K = X^T S C_g the
                   coefficients of the delivered vectors in the reference's S-orthonormal basis (so that K K^T is the
                   projector C_g C_g^T S and the indicator of g is the reference's X_g X_g^T S, both in that basis):
                   max |K K^T - 1_g| <= 2 max_{j in g} sqrt(sum_{i not in g} (bound(M_ij) / delta_ig)^2) + orthonormality
                   bound, delta_ig the distance of level i from the levels of g: eigh_cases' Davis-Kahan form,
                   2 sin theta plus the orthonormality defect, with sin theta taken row by row -- the component of a
                   delivered vector j of g along the reference vector i outside g is M_ij / (l_j - l_i) to first order.
                   delta_ig >= gamma_g, with which it is eigh_cases' 2 ||column||_2 / gamma_g; the rows keep their own
                   distances because at kappa = 1e4 the rounding of T beside the graded 1e6 levels is 1e-7 per entry,
                   and N of them over the ONE smallest gap would put the condition below out of reach.
  order            w ascending; F, S and C0 bit-identical after the call.

Condition.  Every group of every case has a subspace bound below SUBSPACE_MAX = 1e-4, asserted when a case is built.

Twin.  refine_twin is a float64 numpy restatement of refine_e_kernel's arithmetic and verdict with the sort, in BLAS
summation order, not the device's.  It is for the CPU tests and for printing beside the device's verdict; it is never
the judge of the device.  Its switches restate the shipped constants (symmetrise_g=False, noise_emax=1e-3) and three
mutants of the kernel.

Starts.  (a) the constructed C rounded; (b), (c), (d) scipy's vectors of (F + t S P S, S) with t = 1e-9, 1e-6, 0.3 and P a
random symmetric matrix of spectral norm one.  (d) must be refused with one iteration, and with more wherever 0.3
exceeds the mean level distance 22 / (N - 1); below that it is far but contracting, and converging from it is no failure."""

from __future__ import annotations

import functools

import numpy as np

from eigh_cases import (GROUP, RF_TOL, SUBSPACE_MAX, group_eigenvalues, groups_of, same_group_mask,  # noqa: F401
                        spectrum)
from matfn_cases import CERTIFICATE, EPS, LD, compose, householder_q, worst_ratio  # noqa: F401

# ------------------------------------------------------------------ the kernel's constants, restated (module docstring)
RF_GIVE_UP = 0.25                      # eigh_refine.hip:46
RF_CLUSTER_NOISE = 1.0e-14             # :47
RF_NOISE = 8.0 * 1.1102230246251565e-16  # :54
RF_NOISE_EMAX = 5.0e-7                 # :64
SHIPPED_NOISE_EMAX_PENCIL = 1.0e-3     # the pencil's own limit before it was tested
RF_MAX_ITER = 6                        # :43

SPECTRA = ("spread", "pairs", "cluster", "graded")
KAPPAS = (1.0e2, 1.0e4)
STARTS = {"a": 0.0, "b": 1.0e-9, "c": 1.0e-6, "d": 0.3}
BOUNDS = ("eigenvalues", "residual", "orthonormality", "subspace")


# ------------------------------------------------------------------ reference
def refine_pencil(f64: np.ndarray, s64: np.ndarray, x: np.ndarray, groups, steps: int = 4):
    """eigh_cases.refine_grouped on the pencil (module docstring).
    -> (X, Rayleigh quotients, T = X^T F X, (max |I - G|, max |T_ij| over i, j in different groups))."""
    f, s = np.asarray(f64, dtype=LD), np.asarray(s64, dtype=LD)
    n = f.shape[0]
    eye = np.eye(n, dtype=LD)
    off = ~np.eye(n, dtype=bool)
    same = same_group_mask(n, groups)
    cross = off & ~same
    for step in range(steps + 1):
        r = eye - x.T @ (s @ x)
        t = x.T @ (f @ x)
        lam = np.diag(t) / (LD(1) - np.diag(r))
        if step == steps:
            break  # (the certificate is taken from R and T as computed)
        r, t = LD(0.5) * (r + r.T), LD(0.5) * (t + t.T)
        d = lam[None, :] - lam[:, None]
        d[~cross] = LD(1)
        e = (t + lam[None, :] * r) / d
        e[same] = r[same] / LD(2)
        e[~off] = np.diag(r) / LD(2)
        x = x + x @ e
    cert = (float(np.max(np.abs(r))), float(np.max(np.abs(t[cross]))) if cross.any() else 0.0)
    return x, lam, t, cert


def unit_symmetric(n: int, seed: int) -> np.ndarray:
    """A random symmetric matrix of spectral norm one."""
    g = np.random.default_rng(seed).standard_normal((n, n))
    g = 0.5 * (g + g.T)
    return g / np.max(np.abs(np.linalg.eigvalsh(g)))


class Case:
    """One rounded pencil with its certified grouped reference, its bounds and its starts."""

    def __init__(self, name: str, n: int, kappa: float, index: int = 0, steps: int = 4):
        self.name, self.n, self.kappa, self.index = name, n, kappa, index
        seed = 1000003 * n + 1009 * SPECTRA.index(name) + 17 * index + 5 * int(round(np.log10(kappa)))
        self.seed = seed
        self.lam0 = spectrum(name, n, seed + 1)
        self.nrm = float(np.max(np.abs(self.lam0)))
        self.groups = groups_of(self.lam0, self.nrm)
        q, qs = householder_q(n, seed), householder_q(n, seed + 2)
        sigma = np.logspace(-np.log10(kappa), 0.0, n).astype(LD)
        self.s = compose(qs, sigma)
        self.c_ld = (qs / np.sqrt(sigma)[None, :]) @ (qs.T @ q)
        sc = self.s.astype(LD) @ self.c_ld
        self.f = compose(sc, self.lam0)
        self.s.setflags(write=False)
        self.f.setflags(write=False)
        self._reference(self.c_ld, steps)

    def _reference(self, x0, steps):
        self.x, self.rayleigh, self.t, self.cert = refine_pencil(self.f, self.s, x0, self.groups, steps)
        ax = np.abs(self.x)
        self.xsx = ax.T @ (np.abs(self.s).astype(LD) @ ax)
        self.xfx = ax.T @ (np.abs(self.f).astype(LD) @ ax)
        self.cert_limits = (CERTIFICATE * max(1.0, float(np.max(self.xsx))), CERTIFICATE * self.nrm)
        assert self.cert[0] <= self.cert_limits[0] and self.cert[1] <= self.cert_limits[1], (self.ident(), self.cert)
        self.lam =group_eigenvalues(self.rayleigh, self.t, self.groups)
        assert np.all(np.diff(self.lam) >= 0), self.ident()
        self._bounds()

    def _bounds(self):
        n, u = self.n, self.n * EPS
        al = np.abs(self.lam)
        w = np.sum(np.abs(self.lam[None, :] - self.lam[:, None]), axis=1)
        self.orthonormality = float(n * RF_TOL**2 + 2.0 * u * np.max(self.xsx))
        self.eigenvalues = RF_TOL**2 * w + 2.0 * u * (np.diag(self.xfx) + al * np.diag(self.xsx))
        self.residual = (3.0 * RF_TOL**2 * np.maximum(w[:, None], w[None, :])
                         + RF_CLUSTER_NOISE * np.sqrt(np.sum(self.lam**2)) * (~np.eye(n, dtype=bool))
                         + 2.0 * u * (self.xfx + al[None, :] * self.xsx))
        self.gamma, self.subspace_bounds = [], []
        for a, b in self.groups:
            below = float(self.lam[a] - self.lam[a - 1]) if a > 0 else np.inf
            above = float(self.lam[b] - self.lam[b - 1]) if b < n else np.inf
            self.gamma.append(min(below, above))
            delta = np.maximum(self.lam[a] - self.lam, self.lam - self.lam[b - 1])  # of level i from the group
            outside = np.ones(n, dtype=bool)
            outside[a:b] = False
            sin_theta = np.sqrt(np.sum((self.residual[outside, a:b] / delta[outside, None]) ** 2, axis=0))
            self.subspace_bounds.append(float(2.0 * np.max(sin_theta, initial=0.0) + self.orthonormality))
        # the condition: every group can be told from its neighbours by a solver that meets the residual bound
        assert max(self.subspace_bounds) < SUBSPACE_MAX, (self.ident(), max(self.subspace_bounds))

    def ident(self) -> str:
        return f"{self.name}-N{self.n}-k{self.kappa:g}[{self.index}]"

    @functools.lru_cache(maxsize=None)
    def start(self, label: str) -> np.ndarray:
        """(a) the constructed C rounded; (b), (c), (d): scipy's vectors of (F + t S P S, S) (module docstring)."""
        if label == "a":
            c0 = np.ascontiguousarray(self.c_ld.astype(np.float64))
        else:
            import scipy.linalg

            p = unit_symmetric(self.n, self.seed + 3)
            c0 = np.ascontiguousarray(scipy.linalg.eigh(self.f + STARTS[label] * (self.s @ p @ self.s), self.s)[1])
        c0.setflags(write=False)
        return c0

    def ratios(self, w, c) -> dict:
        """error / bound of computed eigenpairs (w ascending, c columns) for the four bounds; NaN or inf: inf."""
        w, c = np.asarray(w), np.asarray(c)
        if not (np.all(np.isfinite(w)) and np.all(np.isfinite(c))):
            return dict.fromkeys(BOUNDS, float("inf"))
        cl, wl = c.astype(LD), w.astype(LD)
        sc = self.s.astype(LD) @ cl
        g = cl.T @ sc
        t = cl.T @ (self.f.astype(LD) @ cl)
        m = t - g * wl[None, :]
        k = self.x.T @ sc
        sub = 0.0
        for (lo, hi), bound in zip(self.groups, self.subspace_bounds):
            d = k[:, lo:hi] @ k[:, lo:hi].T
            d[np.arange(lo, hi), np.arange(lo, hi)] -= LD(1)
            sub = max(sub, float(np.max(np.abs(d))) / bound)
        self.last_defect = float(np.max(np.abs(g - np.eye(self.n, dtype=LD))))  # max |C^T S C - I| of this call
        return {
            "eigenvalues": float(np.max(np.abs(wl - self.lam) / self.eigenvalues)),
            "residual": float(np.max(np.abs(m) / self.residual)),
            "orthonormality": self.last_defect / self.orthonormality,
            "subspace": sub,
        }

    def gram_defect(self, c) -> float:
        """max |C^T S C - I| in longdouble."""
        cl = np.asarray(c).astype(LD)
        return float(np.max(np.abs(cl.T @ (self.s.astype(LD) @ cl) - np.eye(self.n, dtype=LD))))


class Drifted(Case):
    """The pencil (F + delta, S) of a case, delta symmetric and small against the gaps between the case's groups:
    same groups, the reference refined from `x0` (the case's own, or that of the step before) and certified anew."""

    def __init__(self, base: Case, delta: np.ndarray, x0=None, steps: int = 4):
        self.name, self.n, self.kappa, self.index = base.name, base.n, base.kappa, base.index
        self.nrm, self.groups, self.s = base.nrm, base.groups, base.s
        f = base.f + delta
        self.f = np.ascontiguousarray(0.5 * (f + f.T))
        self.f.setflags(write=False)
        x0 = base.x if x0 is None else x0
        self.x0 = x0
        self._reference(x0, steps)

    def first_update(self, since: np.ndarray) -> float:
        """max |x0_i^T since x0_j / (l_j - l_i)| over pairs in different groups: the update one iteration has to make
        when F has moved by `since` from the pencil whose eigenvectors x0 are."""
        n = self.n
        cross = ~np.eye(n, dtype=bool) & ~same_group_mask(n, self.groups)
        e = (self.x0.T @ (np.asarray(since, dtype=LD) @ self.x0))[cross] / (self.lam[None, :] - self.lam[:, None])[cross]
        return float(np.max(np.abs(e)))

    def ident(self) -> str:
        return Case.ident(self) + "+drift"


@functools.lru_cache(maxsize=None)
def case(name: str, n: int, kappa: float = 1.0e2, index: int = 0) -> Case:
    return Case(name, n, kappa, index)


# ------------------------------------------------------------------ case tables
# the smallest the entry point takes | one 16-wide tile, the first size needing a second | N^2 = RF_WGS RF_THREADS
# RF_UNROLL: one stride, one stride plus a tail | the benchmark size | with batch 2 the last size on the paired small
# GEMM with norm_part, the first on the general GEMMs (the E kernel's own norm pass and hand-over) | general GEMMs
SIZES = [2, 3, 16, 17, 37, 128, 129, 148, 176, 177, 230]
ALL_SPECTRA_SIZES = [37, 148, 177]
BOTH_KAPPA_SIZES = [37, 148]
TABLE = [(n, name, kappa) for n in SIZES for name in (SPECTRA if n in ALL_SPECTRA_SIZES else SPECTRA[:2])
         for kappa in (KAPPAS if n in BOTH_KAPPA_SIZES else KAPPAS[:1])]
BATCH_FIVE_SIZES = [112, 113]  # the same route edge for batch 5
BATCH_FIVE = (("spread", 0), ("pairs", 0), ("spread", 1), ("pairs", 1), ("spread", 2))
MUST_ACCEPT = ("spread", "graded")
CHAIN_STEPS = 8
CHAIN_DRIFTS = (1.0e-7, 1.0e-10)  # of a symmetric matrix of spectral norm one, per step


def table_id(entry) -> str:
    n, name, kappa = entry
    return f"N{n}-{name}-k{kappa:g}"


def pair_route(n: int, batch: int) -> bool:
    """nbx_geig_refine's `pair`: the paired small GEMM that leaves norm_part (gemm.hip: nbx_gemm_small_supported)."""
    tiles = (n + 15) // 16
    return tiles * tiles * 2 * batch <= 512


def all_case_keys():
    """Every (name, n, kappa, index) the GPU test builds a longdouble reference for."""
    keys = [(name, n, kappa, index) for n, name, kappa in TABLE for index in (0, 1)]
    keys += [(name, n, 1.0e2, index) for n in BATCH_FIVE_SIZES for name, index in BATCH_FIVE]
    return sorted(set(keys), key=lambda k: (k[1], SPECTRA.index(k[0]), k[2], k[3]))


# ------------------------------------------------------------------ float64 twin
def refine_twin(f, s, c0, max_iter: int = 1, noise_emax: float = RF_NOISE_EMAX, symmetrise_g: bool = True, *,
                norm_part: bool = False, direct: bool | None = None, ignore_cmax: bool = False,
                flip_sign: bool = False, no_division: bool = False):
    """refine_e_kernel and nbx_geig_refine's loop in float64 numpy -> (w, c, status, log).  status: 1000 + the
    accepting iteration, or <= 0 (-1 not contracting or out of iterations, -3 direct path with levels out of order);
    w and c are what the iteration holds even when refused (the device leaves its outputs untouched then).
    norm_part: omega from ||T - diag||_F as the paired small GEMM leaves it, otherwise from the smaller one-sided
    residual of each pair.  direct: no sorting pass (max_iter == 1 with separate output).  The last three switches
    are mutants: the cluster test removed, the sign of lambda_j G_ij flipped, lambda_i = T_ii without / G_ii.
    log: per iteration (max |E|, cmax, nmax, ||T||_F of the first iteration)."""
    f, s = np.asarray(f, dtype=np.float64), np.asarray(s, dtype=np.float64)
    c = np.array(c0, dtype=np.float64)
    n = f.shape[0]
    direct = (max_iter == 1) if direct is None else direct
    off = ~np.eye(n, dtype=bool)
    st, na, lam, log = 0, 0.0, None, []
    for it in range(max_iter):
        t = c.T @ (c.T @ f).T
        g = c.T @ (c.T @ s).T
        lam = np.diag(t).copy() if no_division else np.diag(t) / np.diag(g)
        li, lj = lam[:, None], lam[None, :]
        # ---- phase 1
        if norm_part:
            off2 = float(np.sum(t[off] ** 2))
        else:
            nm = np.minimum(np.abs(t - lj * g), np.abs(t - li * g))
            off2 = float(np.sum(nm[off] ** 2))
        r2 = float(np.sum((np.eye(n) - g) ** 2))
        if it == 0:
            na = float(np.sqrt(np.sum(t**2)))
        om_s, om_r = 2.0 * np.sqrt(off2), 2.0 * np.sqrt(r2)
        # ---- phase 2
        sx = 0.5 * (t + t.T)
        gg = 0.5 * (g + g.T) if symmetrise_g else g
        d = lj - li
        rot = off & (np.abs(d) > om_s + np.maximum(np.abs(li), np.abs(lj)) * om_r)
        num = sx + lj * gg if flip_sign else sx - lj * gg
        with np.errstate(all="ignore"):
            e = np.where(rot, num / np.where(rot, d, 1.0), -0.5 * gg)
        e[~off] = 0.5 * (1.0 - np.diag(g))
        emax = float(np.max(np.abs(e)))
        nmax = float(np.max(np.abs(num[rot]))) if rot.any() else 0.0
        unrot = off & ~rot
        cmax = float(np.max(np.abs(sx[unrot]))) if unrot.any() and not ignore_cmax else 0.0
        log.append((emax, cmax, nmax, na))
        at_noise = nmax <= RF_NOISE * np.sqrt(float(n)) * na and emax < noise_emax
        if not (emax < RF_GIVE_UP):
            st = -1
        elif (emax < RF_TOL or at_noise) and cmax <= RF_CLUSTER_NOISE * na:
            st = it + 1
        elif it == max_iter - 1:
            st = -1
        if st >= 0:
            c = c @ (np.eye(n) + e)
        if st != 0:
            break
    if direct:
        if st > 0 and np.any(lam[:-1] > lam[1:]):
            st = -3
        return lam, c, (1000 + st if st > 0 else st), log
    order = np.argsort(lam, kind="stable")
    return lam[order], c[:, order], (1000 + st if st > 0 else st), log
