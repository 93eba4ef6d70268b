"""Oracle: singular values and right singular vectors in extended precision.

TEST INFRASTRUCTURE (see oracle/__init__.py).

A textbook one-sided (Hestenes) Jacobi SVD (Hestenes 1958; Demmel & Veselic, SIAM J. Matrix
Anal. Appl. 13, 1204 (1992)) carried out in ``np.longdouble`` (x87 extended: 64-bit
significand, eps = 2^-63 ~ 1.1e-19, exponent range to 1e+-4931) on the float64 input taken
exactly.  The columns of A are orthogonalised pairwise, G = A V, sigma_j = ||g_j||.  A pair
(p, q) is left alone when |g_p . g_q| <= eps_ld ||g_p|| ||g_q|| -- there is no rank floor, so
exactly-zero columns stop at once and tiny ones are still orthogonalised to the working precision.
The pairs of a sweep follow the round-robin tournament ordering (Brent & Luk 1985), which lets
the n/2 disjoint rotations of one step be applied as whole-array operations.

A wide matrix (m < n) is handled through its transpose: Jacobi on A^T (n x m) gives
A^T W = U' diag(sigma), and the columns of U' are the right singular vectors of A for the
nonzero sigma; the rest of V (a basis of the null space) is completed by Gram-Schmidt with
pivoting against the identity.

``svd_right(a)`` mirrors ``nbx_svd_right``: it returns (sigma, vt) with sigma descending,
``min(m, n)`` values, and vt the n x n matrix whose rows are the right singular vectors, all
in ``np.longdouble``.
"""

from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS_LD = np.finfo(LD).eps
MAX_SWEEPS = 60


def _round_robin(npad: int) -> list[np.ndarray]:
    """Row permutations for the npad - 1 steps of a round-robin sweep (circle method: hold one
    player, turn the others).  Rows are kept in the order (top of the table, bottom of the table
    reversed), so the pairs of every step are rows (k, npad/2 + k); entry s is the gather that
    takes the rows from their step-s order to their step-(s+1) order."""
    h = npad // 2
    idx = list(range(npad))

    def rows(ix):
        return ix[:h] + ix[h:][::-1]

    perms = []
    for _ in range(max(npad - 1, 1)):
        nxt = [idx[0]] + [idx[-1]] + idx[1:-1]
        cur, new = rows(idx), rows(nxt)
        where = {lab: r for r, lab in enumerate(cur)}
        perms.append(np.array([where[lab] for lab in new]))
        idx = nxt
    return perms


def _hestenes(a: np.ndarray):
    """One-sided Jacobi on the columns of a (m x n, m >= 1).  Returns (G^T, V^T): the rows of G^T
    are the orthogonalised columns and the rows of V^T the matching right vectors.  An odd n is
    padded with a zero column, which never rotates (its inner products are exactly zero)."""
    m, n = a.shape
    npad = n + (n & 1)
    h = npad // 2
    gt = np.zeros((npad, m), dtype=LD)    # row j = column j of A
    gt[:n] = a.T
    vt = np.eye(npad, dtype=LD)
    lab = np.arange(npad)                 # which column sits in each row
    perms = _round_robin(npad)
    for _ in range(MAX_SWEEPS):
        rotated = False
        for perm in perms:
            gp, gq = gt[:h], gt[h:]
            al = np.einsum("ij,ij->i", gp, gp)
            be = np.einsum("ij,ij->i", gq, gq)
            ga = np.einsum("ij,ij->i", gp, gq)
            act = np.abs(ga) > EPS_LD * np.sqrt(al) * np.sqrt(be)
            if act.any():
                rotated = True
                zeta = (be - al) / (2 * np.where(act, ga, 1))
                t = np.where(zeta < 0, -1, 1) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = np.where(act, 1 / np.sqrt(1 + t * t), 1)[:, None]
                s = np.where(act, t * c[:, 0], 0)[:, None]
                for w in (gt, vt):
                    x, y = w[:h].copy(), w[h:]
                    w[:h] = c * x - s * y
                    w[h:] = s * x + c * y
            gt, vt, lab = gt[perm], vt[perm], lab[perm]
        if not rotated:
            inv = np.argsort(lab)
            return gt[inv][:n], vt[inv][:n, :n]
    raise RuntimeError(f"oracle.svd: no convergence in {MAX_SWEEPS} sweeps for a {m} x {n} matrix")


def _complete(q: np.ndarray, n: int) -> np.ndarray:
    """Rows of q (r x n, orthonormal) extended by n - r orthonormal rows spanning their complement."""
    r = q.shape[0]
    res = np.eye(n, dtype=LD)
    for _ in range(2):  # project out span(q) twice ("twice is enough")
        res = res - (res @ q.T) @ q
    out = []
    for _ in range(n - r):
        j = int(np.argmax(np.einsum("ij,ij->i", res, res)))
        v = res[j] / np.sqrt(res[j] @ res[j])
        for b in [q] + ([np.array(out)] if out else []):
            v = v - (b @ v) @ b
        v = v / np.sqrt(v @ v)
        out.append(v)
        res = res - np.outer(res @ v, v)
    return np.concatenate([q, np.array(out, dtype=LD).reshape(n - r, n)])


def svd_right(a: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(sigma, vt) of the float64 matrix a, in np.longdouble: sigma descending (min(m, n) values),
    vt n x n with the right singular vectors as rows (null-space rows last)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or 0 in a.shape:
        raise ValueError(f"oracle.svd: need a non-empty 2-D matrix, got shape {a.shape}")
    m, n = a.shape
    if m >= n:
        gt, vt = _hestenes(a)
        sig = np.sqrt(np.einsum("ij,ij->i", gt, gt))
        order = np.argsort(-sig, kind="stable")
        return sig[order], vt[order]
    # wide: the right singular vectors of A are the normalised orthogonal columns of A^T W
    ut, _ = _hestenes(a.T)
    sig = np.sqrt(np.einsum("ij,ij->i", ut, ut))
    order = np.argsort(-sig, kind="stable")
    sig, ut = sig[order], ut[order]
    nz = int(np.count_nonzero(sig > 0))
    q = ut[:nz] / sig[:nz, None]
    return sig, _complete(q, n)
