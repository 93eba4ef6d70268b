"""Shared by tests/test_host_matfn_cases.py (CPU) and tests/test_gpu_matfn.py (MI355X): operands, extended-precision
references, error bounds and float64 emulations for the two matrix functions the SCF takes WITHOUT an eigensolver --
the occupied-space projector by SP2 purification (nbx_purify, nbed_amd/csrc/purify.hip) and S^p by the coupled
Newton-Schulz iteration (nbx_sym_pow_ns, nbed_amd/csrc/eigh.hip) -- and for the eigen route nbx_sym_pow behind them.

Operands.  Eigenvectors Q are a product of three Householder reflectors built in np.longdouble (orthogonal to 1e-19,
every entry nonzero), the spectrum is chosen by hand with distinct levels (a jittered grid for the Fock-like matrices,
a logarithmic grid for the overlap-like ones), A = Q L Q^T is formed in longdouble, symmetrised and rounded to float64.

Reference.  It is the reference of the ROUNDED matrix: starting from Q, three Ogita-Aishima refinement steps in
longdouble (R = I - X^T X, S = X^T A X, l_i = s_ii / (1 - r_ii), E_ij = (s_ij + l_j r_ij) / (l_j - l_i), E_ii = r_ii / 2,
X <- X (I + E)); then P_ref = X_occ X_occ^T and S^p_ref = X l^p X^T.  Each carries a certificate, max |I - X^T X| and
max |offdiag(X^T A X)|, which tests/test_host_matfn_cases.py holds to 1e-17 ||A||.

Bounds (eps = 2^-52; none is fitted to a kernel).

* Purification: |P - P_ref| <= 2 PUR_IDEM + N eps (l_max - l_min) / gap elementwise.  2 PUR_IDEM = 4e-12 is what the
  kernel's stopping rule promises (purify.hip: tr(P - P^2) of the step before below PUR_IDEM, "the result is good to
  ~2x this"); the second term is the first-order perturbation of a spectral projector, ||dP|| <= ||dA|| / gap, under
  a backward error N eps ||A|| of the products.  |tr P - n_occ| <= N times that.
* Powers: |got - ref| <= N eps kappa max|ref| for p = -1/2 and p = -1, with sqrt(kappa) for p = +1/2 (the relative
  condition of S^1/2 is set by the SMALL eigenvalues' share of S^1/2 itself, sqrt(l_min)); kappa is the condition
  number of the constructed spectrum.

Emulations.  purify_emulated and newton_schulz_emulated are float64 numpy transcriptions of the two iterations, written
from the formulas in the kernels' header comments: same bounds, same update, same stopping rule.  They are used by the
host test alone, to show that a correct float64 evaluation is accepted on every case and stays inside the bounds."""

from __future__ import annotations

import functools

import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble

# ------------------------------------------------------------------ the kernels' constants, restated (purify.hip, eigh.hip)
PUR_IDEM = 2.0e-12
PUR_MAX_ITER = 72
PUR_ALL_AT_ONCE_MAX_N = 196  # pur_step_kernel: N <= 196 requests all 49 MFMA operands at once, beyond a 16-wide loop
PUR_INIT_GRID_SWITCH = 64    # pur_init_kernel: 1 workgroup per matrix below, 8 from here
PUR_MAX_BATCH = 64
NS_MAX_ITER = 28             # backend.sym_pow_newton_schulz defaults
NS_CHECK_EVERY = 4
NS_ACCEPT_NOW = 2.0 * EPS    # x N: a residual below this is accepted as it is (Z is off by r / 2: within N eps)
NS_ONE_MORE = 1.0e-8        # a residual below this: one more step (3 r^2 / 4) reaches rounding level
NS_TWO_MORE = 1.0e-6         # ... below this: two more
NS_T_GRID_SWITCH = 182      # ns_t_kernel: cdiv(N^2, 256) blocks up to N = 181 (128 blocks), a grid-stride loop from 182
CERTIFICATE = 1.0e-17        # x ||A||: what every reference is held to


# ------------------------------------------------------------------ construction
def householder_q(n: int, seed: int) -> np.ndarray:
    """Product of three Householder reflectors I - 2 v v^T / v^T v, in longdouble."""
    rng = np.random.default_rng(seed)
    q = np.eye(n, dtype=LD)
    for _ in range(3):
        v = rng.standard_normal(n).astype(LD)
        q = q - (q @ v)[:, None] * (LD(2) * v / (v @ v))[None, :]
    return q


def jittered_grid(lo: float, hi: float, n: int, rng) -> np.ndarray:
    """n ascending levels on [lo, hi]: an even grid, each level moved by up to 0.3 spacings (levels stay distinct)."""
    if n == 1:
        return np.array([lo])
    h = (hi - lo) / (n - 1)
    return np.linspace(lo, hi, n) + h * rng.uniform(-0.3, 0.3, size=n)


def fock_spectrum(n: int, nocc: int, gap: float, seed: int) -> np.ndarray:
    """Levels from -12 towards 10 Ha with the distance between level nocc and level nocc + 1 set to ``gap`` (0: a
    degenerate pair).  nocc = 0 or n: nothing to separate, the grid as it is."""
    rng = np.random.default_rng(seed)
    lam = jittered_grid(-12.0, 10.0 - gap, n, rng)
    if 0 < nocc < n:
        lam[nocc:] = lam[nocc:] - lam[nocc] + lam[nocc - 1] + gap
    return lam


def compose(q: np.ndarray, lam: np.ndarray) -> np.ndarray:
    """Q diag(lam) Q^T in longdouble, symmetrised, rounded to float64."""
    a = (q * np.asarray(lam, dtype=LD)[None, :]) @ q.T
    return np.ascontiguousarray((LD(0.5) * (a + a.T)).astype(np.float64))


# ------------------------------------------------------------------ reference
def refine(a64: np.ndarray, x: np.ndarray, steps: int = 3):
    """Ogita-Aishima refinement of the eigenvector matrix x of the float64 matrix a64, in longdouble.
    -> (x, lam, (max |I - X^T X|, max |offdiag X^T A X|)) of the refined x."""
    a = np.asarray(a64, dtype=LD)
    n = a.shape[0]
    eye = np.eye(n, dtype=LD)
    off = ~np.eye(n, dtype=bool)
    for step in range(steps + 1):
        r = eye - x.T @ x
        s = x.T @ (a @ x)
        lam = np.diag(s) / (LD(1) - np.diag(r))
        if step == steps:
            break  # (the certificate is taken from R and S as computed)
        # R and S are symmetric; so must their computed values be: the rounding of an unsymmetric S, divided by a
        # small l_j - l_i, would enter E as a symmetric term, which costs orthogonality in first order
        r, s = LD(0.5) * (r + r.T), LD(0.5) * (s + s.T)
        d = lam[None, :] - lam[:, None]
        d[~off] = LD(1)
        e = (s + lam[None, :] * r) / d
        e[~off] = np.diag(r) / LD(2)
        x = x + x @ e
    cert = (float(np.max(np.abs(r))), float(np.max(np.abs(s[off]))) if n > 1 else 0.0)
    return x, lam, cert


class Reference:
    """The refined eigenpairs of one rounded matrix, with what the tests derive from them."""

    def __init__(self, a64, q, lam0):
        self.a = a64
        self.n = a64.shape[0]
        self.x, self.lam, self.cert = refine(a64, q)
        self.norm = float(np.max(np.abs(lam0)))  # ||A||_2 of the constructed matrix
        self.lam0 = np.asarray(lam0, dtype=np.float64)

    def projector(self, nocc: int) -> np.ndarray:
        xo = self.x[:, :nocc]
        return xo @ xo.T

    def power(self, p: float) -> np.ndarray:
        return (self.x * self.lam[None, :] ** LD(p)) @ self.x.T


# ------------------------------------------------------------------ bounds
def purify_bound(n: int, lam, gap: float) -> float:
    """Elementwise bound of |P - P_ref| (module docstring); inf where there is no gap."""
    width = float(np.max(lam) - np.min(lam))
    if gap <= 0:
        return float("inf")
    return 2.0 * PUR_IDEM + n * EPS * width / gap


def power_bound(n: int, kappa: float, p: float, ref) -> float:
    k = np.sqrt(kappa) if p == 0.5 else kappa
    return float(n * EPS * k * np.max(np.abs(ref)))


def worst_ratio(got, ref, bound: float) -> float:
    """max |got - ref| / bound, the difference taken in longdouble; a NaN or an inf in got counts as inf."""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = float(np.max(np.abs(got.astype(LD) - np.asarray(ref, dtype=LD)))) if got.size else 0.0
    assert bound > 0
    return err / bound


# ------------------------------------------------------------------ purification cases
# (n, occupations -- one per matrix of the batch --, gap): tests/test_gpu_matfn.py runs each as ONE call
PURIFY_CASES = [
    (2, (1, 1), 0.5),            # smallest N
    (16, (3, 3), 0.3),           # one tile
    (20, (1, 19), 0.4),          # very unequal occupations
    (37, (0, 37), 0.3),          # empty and full: rank 0 and rank N
    (63, (7, 7), 0.2),           # one workgroup builds P0; partial tile
    (64, (7, 7), 0.2),           # eight workgroups build P0
    (65, (7, 7), 0.2),           # ... and one row past a tile
    (100, (10, 9), 0.02),        # small gap
    (196, (33, 30), 0.05),       # last size whose operands are requested at once
    (197, (33, 30), 0.05),       # first loop size, tail of 5
    (200, (40,), 0.1),           # batch 1, tail of 8
    (208, (21,), 0.05),          # loop without tail
    (230, (50,), 0.02),
    (37, (5, 5, 5), 0.3),        # batch above two
]
LADDER_SIZES = [(64, 7), (200, 40)]
LADDER_GAPS = [1e-2, 1e-3, 1e-4, 1e-6, 0.0]
LADDER_ACCEPTED = [1e-2, 1e-3]  # what the float64 emulation accepts; the device is REQUIRED to accept only 1e-2


def purify_id(case) -> str:
    n, nocc, gap = case
    return f"N{n}-occ{'_'.join(map(str, nocc))}-gap{gap:g}"


@functools.lru_cache(maxsize=None)
def purify_matrix(n: int, nocc: int, gap: float, index: int = 0):
    """-> (F float64, Reference or None for gap 0, constructed levels)."""
    seed = 1000003 * n + 1009 * nocc + 17 * index + int(round(-np.log10(gap))) if gap > 0 else 1000003 * n + nocc + 5
    q = householder_q(n, seed)
    lam = fock_spectrum(n, nocc, gap, seed + 1)
    f = compose(q, lam)
    f.setflags(write=False)
    return f, (Reference(f, q, lam) if gap > 0 else None), lam


def purify_case(case):
    """-> (F (batch, n, n), P_ref (batch, n, n) longdouble, bound per matrix, references)."""
    n, nocc, gap = case
    mats = [purify_matrix(n, k, gap, i) for i, k in enumerate(nocc)]
    f = np.stack([m[0] for m in mats])
    p_ref = np.stack([m[1].projector(k) for m, k in zip(mats, nocc)])
    bounds = [purify_bound(n, m[2], gap) for m in mats]
    return f, p_ref, bounds, [m[1] for m in mats]


# ------------------------------------------------------------------ power cases
POWER_SIZES = [2, 16, 37, 148, 181, 182, 200]  # 181 | 182: ns_t_kernel's grid switch
EIGEN_SIZES = [37, 148, 196, 197]              # 196 | 197: nbx_eigh's LDS solver | the tridiagonal route
KAPPAS = [1e1, 1e4, 1e6]
POWERS = [-0.5, 0.5, -1.0]
REFUSED_KAPPA = 1e9


@functools.lru_cache(maxsize=None)
def power_matrix(n: int, kappa: float):
    """Overlap-like: levels log-spaced from 1 down to 1 / kappa.  -> (S float64, Reference)."""
    q = householder_q(n, 7919 * n + int(np.log10(kappa)))
    lam = np.logspace(0.0, -np.log10(kappa), n)[::-1].copy()
    s = compose(q, lam)
    s.setflags(write=False)
    return s, Reference(s, q, lam)


@functools.lru_cache(maxsize=None)
def power_reference(n: int, kappa: float, p: float):
    """-> (S^p longdouble, bound)."""
    ref = power_matrix(n, kappa)[1].power(p)
    return ref, power_bound(n, kappa, p, ref)


def refused_ill_conditioned(n: int = 37) -> np.ndarray:
    return compose(householder_q(n, 31), np.logspace(-9.0, 0.0, n))


def refused_indefinite(n: int = 37) -> np.ndarray:
    rng = np.random.default_rng(32)
    return compose(householder_q(n, 33), jittered_grid(-1.0, 1.0, n, rng))


# ------------------------------------------------------------------ float64 emulations
def purify_emulated(f: np.ndarray, nocc: int, max_iter: int = PUR_MAX_ITER):
    """purify.hip's header in numpy: Gershgorin column discs, P0 = (l_max I - F) / (l_max - l_min), then
    P <- P^2 if tr P > nocc else 2 P - P^2, until |tr P_k - tr P_{k-1}| < PUR_IDEM with |tr P_k - nocc| < 1e-6.
    -> (P, status): status = index of the accepting step + 1, -1 (step limit, not finite), -2 (no usable bounds)."""
    n = f.shape[0]
    d = np.diag(f).copy()
    o = np.abs(f)
    np.fill_diagonal(o, 0.0)
    r = o.sum(axis=0)
    lmin, lmax = np.min(d - r), np.max(d + r)
    with np.errstate(all="ignore"):
        inv = 1.0 / (lmax - lmin)
        p = (lmax * np.eye(n) - f) * inv
    if not (lmax > lmin and np.isfinite(inv)):
        return p, -2
    max_iter = PUR_MAX_ITER if max_iter <= 0 or max_iter > PUR_MAX_ITER else max_iter
    prev = None
    for it in range(max_iter):
        t = float(np.sum(np.diag(p)))
        finite = np.isfinite(t)
        if prev is not None and finite and abs(t - prev) < PUR_IDEM and abs(t - nocc) < 1.0e-6:
            return p, it + 1
        if not finite or it == max_iter - 1:
            return p, -1
        prev = t
        with np.errstate(all="ignore"):
            p2 = p @ p
        p = p2 if t > nocc else 2.0 * p - p2
    raise AssertionError("unreachable")


def newton_schulz_emulated(s: np.ndarray, p: float, max_iter: int = NS_MAX_ITER, check_every: int = NS_CHECK_EVERY):
    """eigh.hip's coupled Newton-Schulz in numpy: A = S / c with c = ||S||_inf, Y_0 = A, Z_0 = I, T = 3 I - Z Y,
    Y <- Y T / 2, Z <- T Z / 2; ||I - Z Y||_F examined every check_every steps: below 2 N eps it stops; below 1e-8 (or stagnating below 1e-9) one
    more step is taken and then it stops, below 1e-6 two more (a step takes a residual r to 3 r^2 / 4, and the error
    of Z is r / 2).  -> (S^p or None, steps or -1)."""
    n = s.shape[0]
    c = float(np.abs(s).sum(axis=1).max())
    eye = np.eye(n)
    y, z = s * (1.0 / c), eye.copy()
    prev, last, converged = -1.0, -1, False
    it = 0
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            zy = z @ y
            t = 3.0 * eye - zy
            if it % check_every == check_every - 1 or it == last:
                res = float(np.sqrt(np.sum((eye - zy) ** 2)))
                if not np.isfinite(res) or res > 1.0e300:
                    return None, -1
                if it == last or res < NS_ACCEPT_NOW * n:
                    converged = True
                    break
                if last < 0:
                    if res < NS_ONE_MORE or (prev >= 0.0 and res > 0.5 * prev and res < 1.0e-9):
                        last = it + 1
                    elif res < NS_TWO_MORE:
                        last = it + 2
                prev = res
            y, z = 0.5 * (y @ t), 0.5 * (t @ z)
    if not converged:
        return None, -1
    if p == 0.5:
        src, scale = y, np.sqrt(c)
    elif p == -0.5:
        src, scale = z, 1.0 / np.sqrt(c)
    else:
        src, scale = z @ z, 1.0 / c
    return 0.5 * scale * (src + src.T), it + 1


def eigh_power(s: np.ndarray, p: float) -> np.ndarray:
    """LAPACK's float64 route, the second judge of a device miss."""
    w, u = np.linalg.eigh(s)
    return (u * w**p) @ u.T
