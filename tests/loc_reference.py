"""numpy restatement of the Jacobi-sweep localisation of csrc/localize.hip (Pipek-Mezey and Boys).

Both maximise f(U) = sum_k sum_i ((U^T Q_k U)_ii)^2.  The pairs of a step come from the same tournament ring
(csrc/jacobi_ring.h), all pairs of a step are rotated together, and the angle, the two rounding guards and the
stopping rule are the kernel's, so the two follow the same trajectory up to rounding.
"""

from __future__ import annotations

import numpy as np

LOC_FLAT = 1.0e-13
LOC_NOISE = 1.0e-13


def ring_steps(n: int):
    """[(s[], t[]) per step] of one sweep over n (padded to even) indices: jacobi_ring.h's geometry."""
    npad = n + (n & 1)
    m = npad // 2
    r = npad - 1
    steps = 1 if m == 1 else npad - 1

    def index0(q):
        return 2 * (q + 1) if q <= m - 2 else 2 * (2 * m - 2 - q) + 1

    def index_at(pos, t):
        if pos < 0:
            return 0
        q = pos - t
        if q < 0:
            q += r
        return index0(q)

    out = []
    for t in range(steps):
        s = [index_at(-1 if k == 0 else k - 1, t) for k in range(m)]
        u = [index_at(2 * m - 2 - k, t) for k in range(m)]
        out.append((np.array(s), np.array(u)))
    return out


def pair_terms(qss, qtt, qst):
    """(A, B, P) of pairs from their (nk, npairs) diagonal / off-diagonal elements."""
    d = qss - qtt
    a = np.sum(qst * qst - 0.25 * d * d, axis=0)
    b = np.sum(qst * d, axis=0)
    p = np.sum(qss * qss + qtt * qtt + 2.0 * qst * qst, axis=0)
    return a, b, p


def angles(a, b, p):
    """(c, s, counted |s|) per pair with the kernel's two guards."""
    amp = np.hypot(a, b)
    rot = amp > LOC_FLAT * p
    g = np.where(rot, 0.25 * np.arctan2(b, -a), 0.0)
    s, c = np.sin(g), np.cos(g)
    counted = np.where(rot & (np.abs(s) * amp > LOC_NOISE * p), np.abs(s), 0.0)
    return c, s, counted


def gains(a, b):
    """f(best angle) - f(0) of pairs: A + hypot(A, B), written without cancellation."""
    h = np.hypot(a, b)
    return np.where(a >= 0, a + h, b * b / np.where(h - a > 0, h - a, 1.0))


def pm_matrices(x, y, offsets):
    """Q_A = 1/2 (X_A^T Y_A + Y_A^T X_A) of every atom: (natm, n, n)."""
    out = []
    for a0, a1 in zip(offsets[:-1], offsets[1:]):
        g = x[a0:a1].T @ y[a0:a1]
        out.append(0.5 * (g + g.T))
    return np.array(out)


def boys_matrices(c, r):
    """Q_k = C^T r_k C: (3, n, n)."""
    return np.einsum("pi,kpq,qj->kij", c, r, c)


def functional(q):
    return float(np.sum(np.einsum("kii->ki", q) ** 2))


def all_pair_gains(q):
    """Gain of every pair (s < t) of the stack of symmetric matrices q (nk, n, n)."""
    n = q.shape[-1]
    s, t = np.triu_indices(n, 1)
    a, b, _ = pair_terms(q[:, s, s], q[:, t, t], q[:, s, t])
    return gains(a, b)


def _rotate(mat, s, t, c, sn, axis):
    """Rotate rows (axis=-2) or columns (axis=-1) s, t of mat in place."""
    if axis == -2:
        ms, mt = mat[..., s, :].copy(), mat[..., t, :].copy()
        mat[..., s, :] = c[:, None] * ms + sn[:, None] * mt
        mat[..., t, :] = c[:, None] * mt - sn[:, None] * ms
    else:
        ms, mt = mat[..., :, s].copy(), mat[..., :, t].copy()
        mat[..., :, s] = c * ms + sn * mt
        mat[..., :, t] = c * mt - sn * ms


def localize_pm(x, y, offsets, max_sweeps=1000, tol=1e-10, history=None):
    """U (n, n), sweeps, f, converged for X (nao, n), Y (nao, n) (None: Y = X) and the atom AO offsets."""
    x = np.array(x, dtype=float)
    same = y is None
    y = x if same else np.array(y, dtype=float)
    nao, n = x.shape
    npad = n + (n & 1)
    xt = np.zeros((npad, nao))
    xt[:n] = x.T
    yt = xt if same else np.zeros((npad, nao))
    if not same:
        yt[:n] = y.T
    ut = np.eye(npad)
    ind = np.zeros((len(offsets) - 1, nao))
    for k, (a0, a1) in enumerate(zip(offsets[:-1], offsets[1:])):
        ind[k, a0:a1] = 1.0
    steps = ring_steps(n)
    sweep, converged = 0, n < 2
    while sweep < max_sweeps and not converged:
        smax = 0.0
        for s, t in steps:
            qss = ind @ (xt[s] * yt[s]).T
            qtt = ind @ (xt[t] * yt[t]).T
            qst = 0.5 * ind @ (xt[s] * yt[t] + yt[s] * xt[t]).T
            c, sn, counted = angles(*pair_terms(qss, qtt, qst))
            smax = max(smax, float(counted.max(initial=0.0)))
            _rotate(xt, s, t, c, sn, -2)
            if not same:
                _rotate(yt, s, t, c, sn, -2)
            _rotate(ut, s, t, c, sn, -2)
        sweep += 1
        converged = smax < tol
        if history is not None:
            history.append(functional(pm_matrices(xt[:n].T, yt[:n].T, offsets)))
    u = ut[:n, :n].T.copy()
    return u, sweep, functional(pm_matrices(xt[:n].T, yt[:n].T, offsets)), converged


def localize_boys(q, max_sweeps=1000, tol=1e-10, history=None):
    """U (n, n), sweeps, f, converged for the three symmetric matrices q (3, n, n)."""
    q = np.array(q, dtype=float)
    n = q.shape[-1]
    npad = n + (n & 1)
    w = np.zeros((q.shape[0], npad, npad))
    w[:, :n, :n] = q
    ut = np.eye(npad)
    steps = ring_steps(n)
    sweep, converged = 0, n < 2
    while sweep < max_sweeps and not converged:
        smax = 0.0
        for s, t in steps:
            c, sn, counted = angles(*pair_terms(w[:, s, s], w[:, t, t], w[:, s, t]))
            smax = max(smax, float(counted.max(initial=0.0)))
            _rotate(w, s, t, c, sn, -2)
            _rotate(ut, s, t, c, sn, -2)
            _rotate(w, s, t, c, sn, -1)
        sweep += 1
        converged = smax < tol
        if history is not None:
            history.append(functional(w))
    return ut[:n, :n].T.copy(), sweep, functional(w[:, :n, :n]), converged
