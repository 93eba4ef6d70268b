"""Shared by tests/test_oracle_svd.py (CPU) and tests/test_gpu_svd.py (MI355X): the matrix classes,
the kernel dispatch rule of nbed_amd/csrc/svd.hip restated, the case table, and the contract an SVD
must meet against the extended-precision reference of oracle/svd.py.

The contract (svd.hip header).  Let p = max(m, n), eps = 2^-52 and
floor = p eps ||A||_F (the rank floor of both kernels: a column pair with a column at or below it is
not rotated).  Then, with the reference's sigma_j and kappa = cond of A with its columns scaled to
unit length (Demmel & Veselic 1992: one-sided Jacobi is accurate relative to that, not to cond(A)):

* sigma_j > floor:   |s_j - sigma_j| / sigma_j <= C p eps min(kappa, ||A||_F / sigma_j)
* sigma_j <= floor:  |s_j - sigma_j| <= floor
* right vectors:     sin of the angle to the reference's vector (or of the largest principal angle
                     to its invariant subspace, for a cluster) <= C p eps min(||A||_F, kappa sigma) / gap
* vt orthonormal to C p eps; for m < n, every column of A vt[m:]^T has norm <= floor + eta ||A||_F.

Derivation of C = 32.  One rotation computed in floating point is an exact rotation of the pair
perturbed by at most ~6 eps relative to the pair (c and s carry ~3 eps each; every new entry is
two products and a sum).  A column takes part in n - 1 rotations per sweep and in S <= 16 sweeps;
rounding errors of that many rotations are not correlated and add like a random walk,
sqrt(16 (n - 1)) <= 4 sqrt(p), so the column-wise relative backward error is eta <= 24 sqrt(p) eps.
Column-wise perturbations of relative size eta move sigma_j by at most ||dB|| ||B^-1|| <=
sqrt(p) eta kappa relatively (B = A with unit columns), and by sqrt(p) eta ||A||_F absolutely:
together 24 p eps min(kappa, ||A||_F / sigma_j).  The stopping test |g_p.g_q| <= sqrt(m) eps
||g_p|| ||g_q|| leaves off-diagonal Gram terms whose effect on sigma is second order for separated
values and at most sqrt(m) eps << p eps for a cluster.  Rounding the result to float64 adds eps.
So C = 32 covers 24 + 1 with room for the final norm evaluation; the same eta bounds the vector
angles through the sin-theta theorem with the absolute (||A||_F / gap) or relative
(kappa sigma / gap) gap, and the orthogonality of V, whose rows take the same rotations.
"""

from __future__ import annotations

import numpy as np

from oracle import svd as osvd
from oracle import synth

EPS = np.finfo(np.float64).eps
LD = np.longdouble
C_BOUND = 32.0

# ------------------------------------------------------------------ dispatch (svd.hip svd_lds_fits)
SL_MAX_NP = 196
SL_MAX_ELEMS = 19200


def np_of(n: int) -> int:
    return (n + 1) & ~1


def lds_fits(m: int, n: int) -> bool:
    """svd.hip svd_lds_fits: the LDS kernel takes NP <= 196 and NP * m <= 19200."""
    return np_of(n) <= SL_MAX_NP and np_of(n) * m <= SL_MAX_ELEMS


def kernel_for(m: int, n: int) -> str:
    return "lds" if lds_fits(m, n) else "fallback"


def align256(x: int) -> int:
    return (x + 255) & ~255


def fallback_worksize(m: int, n: int) -> int:
    """nbx_svd_worksize when the global-memory kernel runs: ping-pong G and V, then the status word."""
    p = np_of(n)
    return align256((2 * p * m + 2 * p * p) * 8) + 256


# ------------------------------------------------------------------ matrix classes
def _orth(rng, m, k):
    q, r = np.linalg.qr(rng.standard_normal((m, k)))
    return q * np.sign(np.diag(r))


def gauss(m, n, seed):
    return np.random.default_rng(seed).standard_normal((m, n))


def graded(m, n, seed, lo=1e-12):
    """B diag(d), columns permuted: B with singular values spread over [1, 10] (cond(B) = 10), d from 1
    down to lo.  With the columns in decreasing order a bidiagonalising SVD (LAPACK) is accurate too;
    permuted, it loses the small values (relative errors ~1e-6 at 60 x 60) while Jacobi does not."""
    rng = np.random.default_rng(seed)
    k = min(m, n)
    b = _orth(rng, m, k) @ np.diag(np.linspace(10.0, 1.0, k)) @ _orth(rng, n, k).T
    return (b * np.logspace(0, np.log10(lo), n)[None, :])[:, rng.permutation(n)]


def spectrum(m, n, seed):
    """U diag(s) W^T with clusters (relative width 1e-12 and 1e-9) in a geometric spectrum."""
    rng = np.random.default_rng(seed)
    k = min(m, n)
    s = np.logspace(0, -6, k)
    s[1:4] = s[1] * (1 + np.array([0.0, 1e-12, -1e-12]))
    if k > 10:
        s[k // 2: k // 2 + 3] = s[k // 2] * (1 + np.array([0.0, 1e-9, 2e-9]))
    s = np.sort(s)[::-1]
    return _orth(rng, m, k) @ np.diag(s) @ _orth(rng, n, k).T


def repeats(m, n, seed):
    """blockdiag(X, X, Z) with rows and columns permuted: every sigma of X occurs exactly twice."""
    rng = np.random.default_rng(seed)
    mx, nx = m // 3, n // 3
    x = spectrum(mx, nx, seed + 1)
    a = np.zeros((m, n))
    a[:mx, :nx] = x
    a[mx:2 * mx, nx:2 * nx] = x
    a[2 * mx:, 2 * nx:] = 3.0 * rng.standard_normal((m - 2 * mx, n - 2 * nx))
    return a[rng.permutation(m)][:, rng.permutation(n)]


def low_rank(m, n, seed, r=4):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m, r)) @ rng.standard_normal((r, n))


def zero(m, n, seed):
    return np.zeros((m, n))


def zero_col(m, n, seed):
    a = gauss(m, n, seed)
    a[:, n // 2] = 0.0
    return a


def twin_cols(m, n, seed):
    a = gauss(m, n, seed)
    a[:, n - 1] = a[:, 0]
    return a


def concentric_like(m, n, seed):
    """The shell-0 matrix of concentric localisation, (S_AA^-1 S_AB C)^T S_AB C (n_virt x n_virt, PSD,
    rank n_act), from the synthetic overlap and core Hamiltonian.  m == n == n_virt."""
    assert m == n
    nao = n + 31
    n_act = 40
    s = synth.overlap(nao, seed=synth.SEED + seed)
    _, c = synth.lowdin_orthonormal(s, synth.hcore(nao, seed=synth.SEED + seed))
    cv = c[:, nao - n:]
    sab_c = s[:n_act, :] @ cv
    left = np.linalg.solve(s[:n_act, :n_act], sab_c)
    return left.T @ sab_c


KINDS = {f.__name__: f for f in (gauss, graded, spectrum, repeats, low_rank, zero, zero_col,
                                  twin_cols, concentric_like)}


def make(kind, m, n, seed=7):
    return np.ascontiguousarray(KINDS[kind](m, n, seed), dtype=np.float64)


# ------------------------------------------------------------------ GPU cases: (kind, m, n)
CASES = [
    # square edge: NP * m = 138 * 138 = 19044 | 140 * 139 = 19460, 140 * 140 = 19600
    ("gauss", 138, 138), ("gauss", 139, 139), ("gauss", 140, 140),
    ("graded", 138, 138), ("graded", 139, 139),
    # NP * m edge: 192 * 100 = 19200 exactly | 192 * 101
    ("gauss", 100, 192), ("gauss", 101, 192),
    # NP edge: NP = 196 | NP = 198 (wide, odd n)
    ("gauss", 97, 196), ("gauss", 10, 197), ("zero", 10, 197), ("low_rank", 10, 197),
    # tall, one and two columns
    ("gauss", 9600, 2), ("gauss", 9601, 2), ("gauss", 9601, 1), ("gauss", 5, 1), ("gauss", 7, 2),
    # wide on both kernels
    ("gauss", 5, 8), ("gauss", 50, 300), ("zero_col", 50, 301),
    # odd n on both kernels (the padding column)
    ("zero_col", 40, 31), ("twin_cols", 33, 21), ("zero_col", 141, 141), ("twin_cols", 160, 145),
    ("low_rank", 180, 141), ("zero", 139, 141),
    # the classes on both kernels
    ("spectrum", 80, 60), ("spectrum", 160, 150), ("repeats", 64, 48), ("repeats", 170, 160),
    ("graded", 60, 40), ("graded", 150, 150), ("graded", 90, 60), ("graded", 170, 170),
    ("low_rank", 50, 31), ("zero", 7, 5),
    # the product's shapes: concentric n_virt x n_virt, SPADE n_act_aos x n_occ
    ("concentric_like", 115, 115), ("concentric_like", 169, 169), ("gauss", 60, 33), ("gauss", 150, 140),
    # one large case
    ("spectrum", 400, 200),
]


def case_id(case):
    kind, m, n = case
    return f"{kind}-{m}x{n}-{kernel_for(m, n)}"


# ------------------------------------------------------------------ contract
def column_kappa(a: np.ndarray) -> float:
    """cond of A with its nonzero columns scaled to unit length (inf if they are dependent)."""
    norms = np.linalg.norm(a, axis=0)
    b = a[:, norms > 0] / norms[norms > 0]
    if b.shape[1] == 0:
        return np.inf
    sv = np.linalg.svd(b, compute_uv=False)
    if b.shape[1] > b.shape[0] or sv[-1] == 0:
        return np.inf
    return float(sv[0] / sv[-1])


def reference(a: np.ndarray):
    return osvd.svd_right(a)


def sigma_errors(a, s, ref_s, kappa=None):
    """(relative error / bound) of every sigma above the floor and (absolute error / floor) of every
    sigma below it; the contract holds when both are <= 1."""
    m, n = a.shape
    p = max(m, n)
    fro = float(np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2)))
    floor = p * EPS * fro
    kappa = column_kappa(a) if kappa is None else kappa
    s = np.asarray(s, dtype=LD)
    err = np.abs(s - ref_s)
    above = ref_s > floor
    rs = ref_s[above].astype(np.float64)
    bound = C_BOUND * p * EPS * np.minimum(kappa, fro / rs)
    rel = (err[above] / ref_s[above]).astype(np.float64) / bound
    absr = (err[~above]).astype(np.float64) / floor if floor > 0 else (err[~above] != 0).astype(np.float64)
    return rel, absr, floor


def _vector_blocks(a, ref_s, kappa, floor):
    """Rows of vt grouped into blocks that the contract resolves: a boundary between rows j and j+1 is
    kept when the vector bound there is below 0.1.  Rows at or below the floor (and the extra null
    rows of a wide matrix) form one block.  Returns [(i0, i1, bound)]."""
    m, n = a.shape
    p = max(m, n)
    fro = float(np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2)))
    rs = ref_s.astype(np.float64)
    r = int(np.count_nonzero(rs > floor))
    vals = list(rs[:r]) + [floor]          # the null block sits at the floor (conservatively)

    def vb(hi, lo):
        gap = hi - lo
        if gap <= 0:
            return np.inf
        return C_BOUND * p * EPS * min(fro, kappa * hi) / gap

    cuts = [0]
    gaps = {}
    for j in range(r):
        b = vb(vals[j], vals[j + 1])
        if b < 0.1:
            cuts.append(j + 1)
            gaps[j + 1] = b
    if cuts[-1] != n:
        cuts.append(n)
    blocks = []
    for i0, i1 in zip(cuts[:-1], cuts[1:]):
        blocks.append((i0, i1, gaps.get(i0, 0.0) + gaps.get(i1, 0.0)))
    return blocks


def check_contract(a, s, vt, ref, label=""):
    """Assert the whole contract (module docstring) of a computed (s, vt) against the reference."""
    ref_s, ref_vt = ref
    m, n = a.shape
    p = max(m, n)
    k = min(m, n)
    assert s.shape == (k,) and vt.shape == (n, n), (label, s.shape, vt.shape)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(vt)), label
    kappa = column_kappa(a)
    rel, absr, floor = sigma_errors(a, s, ref_s, kappa)
    assert rel.size == 0 or rel.max() <= 1.0, (label, "relative sigma error / bound", float(rel.max()),
                                                 int(np.argmax(rel)))
    assert absr.size == 0 or absr.max() <= 1.0, (label, "sub-floor sigma error / floor", float(absr.max()))
    assert np.all(np.diff(s) <= 0), (label, "sigma not descending")
    # orthonormal right vectors
    vld = np.asarray(vt, dtype=LD)
    orth = float(np.max(np.abs(vld @ vld.T - np.eye(n, dtype=LD))))
    assert orth <= C_BOUND * p * EPS, (label, "vt orthonormality", orth)
    # vectors and invariant subspaces against the reference
    for i0, i1, bound in _vector_blocks(a, ref_s, kappa, floor):
        if i1 - i0 == n:
            continue  # the whole space: nothing to resolve
        if i1 - i0 == 1:
            x, y = vld[i0], ref_vt[i0]
            d = float(np.linalg.norm(x - np.sign(x @ y) * y))
        else:
            pa = vld[i0:i1].T @ vld[i0:i1]
            pb = ref_vt[i0:i1].T @ ref_vt[i0:i1]
            d = float(np.linalg.norm((pa - pb).astype(np.float64), 2))
        assert d <= bound, (label, f"rows {i0}:{i1}", d, bound)
    if m < n:
        # a null column stops moving once its norm is <= floor; A v_j differs from that computed column
        # by the backward error eta ||A||_F of the rotations (eta = 24 sqrt(p) eps, see above)
        fro = float(np.sqrt(np.sum(np.asarray(a, dtype=LD) ** 2)))
        lim = floor + 24.0 * np.sqrt(p) * EPS * fro
        res = np.linalg.norm(np.asarray(a, dtype=LD) @ vld[m:].T, axis=0)
        assert float(res.max()) <= lim, (label, "||A v_null||", float(res.max()), floor, lim)
