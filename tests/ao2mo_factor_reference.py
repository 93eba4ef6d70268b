"""Extended-precision references, bounds and a numpy checker for the four-index transform from a factor of the integrals
(csrc/ao2mo_factor.hip, HipBackend.ao2mo_factor): shared by tests/test_host_ao2mo_factor.py and
tests/test_gpu_ao2mo_factor.py.

With M_L^x = C_x^T B_L C_x the packed half transform is P[x, L, i (i + 1) / 2 + j] = M_L^x[i, j] (j <= i) and the blocks are
(ij|kl)_xy = sum_L M_L^x[i, j] M_L^y[k, l].  The references are numpy ``np.longdouble`` (64-bit significand on x86).

Bounds (u = 2^-53), none of them fitted to a result:
  stage 1   |P - P_ref| <= e1 A_L^x[i, j],  e1 = 2 (N + 1) u,  A_L^x = |C_x|^T |B_L| |C_x|: the dot-product bound of two
            chained products of length N (gamma_N each), whatever the order of the sums.
  blocks    the computed P carries e1 A, the naux-term sum over products of them gamma_naux more:
            |G - G_ref| <= (2 e1 + e1^2 + (naux + 1) u (1 + e1)^2) sum_L A_L^x[i, j] A_L^y[k, l].
"""

from __future__ import annotations

import numpy as np

from oracle_backend import OracleLookaheadBackend

U = 2.0 ** -53
LD = np.longdouble

# (N, n, naux, nset): N and n off every tile multiple (16 columns, 64 rows per chunk), n = 1, n = N, naux below and above
# one grid wave of 256 compute units; the last one is past N = 444, where the kernel no longer stages C in LDS
SHAPES = [(7, 1, 1, 1), (7, 7, 3, 2), (18, 5, 65, 2), (33, 33, 17, 1), (70, 13, 130, 2), (148, 40, 64, 2), (449, 6, 2, 2)]


def inputs(shape, seed=0):
    """(b (naux, N, N) exactly symmetric, [c_x (N, n)]) for one of SHAPES."""
    big_n, n, naux, nset = shape
    rng = np.random.default_rng(1000 * big_n + 10 * n + naux + seed)
    b = rng.standard_normal((naux, big_n, big_n))
    b = 0.5 * (b + b.transpose(0, 2, 1))
    return b, [rng.standard_normal((big_n, n)) for _ in range(nset)]


def tril_pack(m):
    """(..., n, n) -> (..., n (n + 1) / 2): the pairs j <= i, row-major."""
    i, j = np.tril_indices(m.shape[-1])
    return m[..., i, j]


def pair_index(n):
    """(n, n) integers pair(i, j) = max (max + 1) / 2 + min."""
    i, j = np.indices((n, n))
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    return hi * (hi + 1) // 2 + lo


def half_reference(b, cs, dtype=LD):
    """(P (nset, naux, npair), A (nset, naux, npair)) in ``dtype``: the packed half transform and the magnitudes
    |C|^T |B_L| |C| its bound is made of."""
    bl = np.asarray(b, dtype=dtype)
    ps, mags = [], []
    for c in cs:
        cl = np.asarray(c, dtype=dtype)
        ps.append(tril_pack(np.matmul(cl.T, np.matmul(bl, cl))))
        mags.append(tril_pack(np.matmul(np.abs(cl).T, np.matmul(np.abs(bl), np.abs(cl)))))
    return np.stack(ps), np.stack(mags)


def half_bound(big_n, mags):
    return 2 * (big_n + 1) * U * mags


def expand(g, n):
    """out[i, j, k, l] = g[pair(i, j), pair(k, l)]."""
    pi = pair_index(n)
    return g[pi[:, :, None, None], pi[None, None, :, :]]


def blocks_reference(b, cs, dtype=LD):
    """([aaaa] or [aaaa, bbbb, aabb] (n, n, n, n) chemist order in ``dtype``, the matching bounds in float64)."""
    p, mags = half_reference(b, cs, dtype)
    big_n, naux, n = b.shape[1], b.shape[0], cs[0].shape[1]
    e1 = 2 * (big_n + 1) * U
    eb = 2 * e1 + e1 * e1 + (naux + 1) * U * (1 + e1) ** 2
    outs, bounds = [], []
    for x, y in ((0, 0),) if len(cs) == 1 else ((0, 0), (1, 1), (0, 1)):
        outs.append(expand(np.matmul(p[x].T, p[y]), n))
        bounds.append(expand((eb * np.matmul(mags[x].T, mags[y])).astype(np.float64), n))
    return outs, bounds


def full_pivoting_cholesky(v, tol):
    """(rank, m) rows l with v ~ l^T l and every residual diagonal <= tol: the textbook algorithm, one column per step."""
    v = np.asarray(v, dtype=np.float64)
    d = np.diag(v).copy()
    vecs = np.zeros((0, v.shape[0]))
    while d.max() > tol:
        k = int(np.argmax(d))
        col = (v[:, k] - vecs.T @ vecs[:, k]) / np.sqrt(d[k])
        vecs = np.vstack([vecs, col])
        d -= col * col
    return vecs


def factor_of(eri, tol):
    """(rank, N, N) symmetric slices with |(pq|rs) - sum_L B_L[pq] B_L[rs]| <= tol from the host tensor."""
    n = eri.shape[0]
    b = full_pivoting_cholesky(eri.reshape(n * n, n * n), tol).reshape(-1, n, n)
    return 0.5 * (b + b.transpose(0, 2, 1))


def molecule_bound(tol, cx, cy):
    """(tol + 4e-13) ||c_i||_1 ||c_j||_1 ||c_k||_1 ||c_l||_1 for the block (C_x C_x|C_y C_y), chemist order: the factor
    reproduces every (pq|rs) within tol, the two integral engines agree within 2e-13, and the rounding of either
    transform (4 N u V_max) is below 2e-13 at the sizes tested."""
    a, b = np.abs(cx).sum(axis=0), np.abs(cy).sum(axis=0)
    return (tol + 4e-13) * np.einsum("i,j,k,l->ijkl", a, a, b, b)


class FactorOracleBackend(OracleLookaheadBackend):
    """The numpy checker backend plus the factor routes of HipBackend by their definitions: ``jk_factor``,
    ``ao2mo_factor`` and an ``eri_cholesky`` that factorises the host engine's tensor with full pivoting."""

    name = "factor-oracle"

    def eri_cholesky(self, basis, tol=1e-8, max_rank=None, cutoff=1e-16):
        from nbed_amd import integrals

        self._count("eri_cholesky")
        return self.asarray(factor_of(integrals.two_electron_native(basis, cutoff=cutoff), tol))

    def jk_factor(self, b, dm):
        self._count("jk_factor")
        bn = self._np(b)
        d = self._np(dm).reshape(-1, dm.shape[-1], dm.shape[-1])
        out = np.empty((1 + d.shape[0],) + d.shape[1:])
        out[0] = np.einsum("lpq,l->pq", bn, np.einsum("lpq,pq->l", bn, d.sum(axis=0)))
        for x in range(d.shape[0]):
            out[1 + x] = np.einsum("lpq,qr,lrs->ps", bn, d[x], bn, optimize=True)
        return self.asarray(out)

    def ao2mo_factor(self, b, ca, cb=None, half="fused"):
        self._count("ao2mo_factor")
        cs = [self._np(ca)] + ([self._np(cb)] if cb is not None else [])
        outs, _ = blocks_reference(self._np(b), cs, dtype=np.float64)
        outs = [self.asarray(o) for o in outs]
        return outs[0] if cb is None else tuple(outs)


def rotation_invariants(h1, h2, orbitals=None):
    """(eigenvalues of h1, eigenvalues of h2 as the matrix [(P, S), (Q, R)]) of a spin-orbital Hamiltonian in the
    physicist order of ``HamiltonianBuilder.build()``, restricted to the spatial ``orbitals`` given: what does not change
    when those orbitals are rotated among themselves or change sign, so two runs whose orbitals differ by such a
    rotation can be compared (a perturbation dM of the matrix moves no eigenvalue by more than ||dM||_2)."""
    if orbitals is not None:
        so = np.sort(np.concatenate([2 * np.asarray(orbitals), 2 * np.asarray(orbitals) + 1]))
        h1, h2 = h1[np.ix_(so, so)], h2[np.ix_(so, so, so, so)]
    nq = h1.shape[0]
    m = h2.transpose(0, 3, 1, 2).reshape(nq * nq, nq * nq)
    return np.linalg.eigvalsh(0.5 * (h1 + h1.T)), np.linalg.eigvalsh(0.5 * (m + m.T))


# nbed(config) on water / 6-31G, two active atoms, both projectors, convergence 1e-9: the factor route at tol = 1e-8
# against the dense route, MEASURED on the numpy checker backend (full-pivoting numpy Cholesky against the host tensor;
# tests/test_host_ao2mo_factor.py prints the figures) and rounded up.  The GPU test allows ten times these, for block
# pivoting against full pivoting.  What is compared and why:
#   energies   e_rhf, classical_energy, correction, hf_emb of either projector: 2.9e-10 at most
#   occupied   rotation_invariants of second_quantised on the occupied orbitals, either projector: h1 3.9e-9, h2 2.8e-10
#   all        rotation_invariants of the whole second_quantised, mu projector: h1 1.8e-9, h2 5.6e-8
# The tensors are not compared element by element, and the whole-space ones not for the Huzinaga projector: between two
# routes the embedded object's VIRTUAL orbitals come out rotated among themselves by O(1) (mu) and spanning another
# space (Huzinaga: the whole-space invariants differ by 0.44 and 0.22) under a 1e-8 change of the integrals -- with the
# dense routes as much as with this one -- while the occupied orbitals and every energy move by 1e-9.
E2E_MEASURED = {"energy": 3e-10, "occ_h1": 4e-9, "occ_h2": 3e-10, "all_h1": 2e-9, "all_h2": 6e-8}
E2E_ENERGY_KEYS = ("e_rhf", "classical_energy", "correction", "hf_emb")


def e2e_differences(got, ref):
    """{projector: {name: |difference|}} of two ``nbed(config)`` results with projector="both", the quantities of
    E2E_MEASURED."""
    out = {}
    for proj in ("mu", "huzinaga"):
        ra, rb = getattr(got, proj), getattr(ref, proj)
        d = {"energy": max(abs(ra[k] - rb[k]) for k in E2E_ENERGY_KEYS)}
        d["energy"] = max(d["energy"], abs(ra["second_quantised"][0] - rb["second_quantised"][0]))
        occ = np.flatnonzero(np.asarray(rb["scf"].mo_occ)[0] > 0)
        assert np.array_equal(occ, np.flatnonzero(np.asarray(ra["scf"].mo_occ)[0] > 0))
        spaces = (("occ", occ),) + ((("all", None),) if proj == "mu" else ())
        for name, orbs in spaces:
            ia = rotation_invariants(*ra["second_quantised"][1:], orbs)
            ib = rotation_invariants(*rb["second_quantised"][1:], orbs)
            d[name + "_h1"], d[name + "_h2"] = np.abs(ia[0] - ib[0]).max(), np.abs(ia[1] - ib[1]).max()
        out[proj] = d
    return out
