"""Spin-orbital CCSD of a small second-quantised Hamiltonian (consumer of the path).

The reference runs PySCF's ``cc.CCSD`` on the embedded SCF object (nbed/driver.py:1105-1135,
``run_emb_ccsd``; global reference at :126-137) and reads ``e_tot`` / ``e_corr``.  For the active spaces
of its own examples -- a few orbitals -- the same numbers follow from the coupled-cluster equations
written over the spin orbitals of the Hamiltonian ``HamiltonianBuilder.build()`` returns,

    H = constant + sum_pq h1[p,q] a+_p a_q + sum_pqrs h2[p,q,r,s] a+_p a+_q a_r a_s

(the 1/2 already in h2), with the occupied spin orbitals those of the embedded determinant.  The
equations are the standard ones (Stanton, Gauss, Watts, Bartlett, J. Chem. Phys. 94, 4334 (1991)) for
a general Fock matrix: the virtual orbitals of an embedded object may have been rotated by the
concentric localization, so f is not assumed diagonal.  Host code, dense einsum, meant for a few tens
of spin orbitals; ``driver._run_emb_ccsd`` falls back to it when no PySCF is installed.
"""

from __future__ import annotations

import numpy as np

MAX_SPIN_ORBITALS = 40


class CCSDResult:
    """Duck-typed stand-in for ``pyscf.cc.CCSD``: ``e_tot``, ``e_corr``, ``e_hf``, ``converged``, ``t1``, ``t2``; with
    the perturbative triples asked for, ``e_t`` and ``e_tot_t`` = ``e_tot + e_t`` (both ``None`` otherwise)."""

    def __init__(self, e_hf, e_corr, t1, t2, converged, iterations, e_t=None):
        self.e_hf = float(e_hf)
        self.e_corr = float(e_corr)
        self.e_tot = float(e_hf + e_corr)
        self.t1, self.t2 = t1, t2
        self.converged = bool(converged)
        self.iterations = int(iterations)
        self.e_t = None if e_t is None else float(e_t)
        self.e_tot_t = None if e_t is None else self.e_tot + self.e_t


def antisymmetrized(h2: np.ndarray) -> np.ndarray:
    """<pq||rs> from the two-body tensor of ``build()``:  H_2 = 1/4 sum <pq||rs> a+_p a+_q a_s a_r."""
    w = 2.0 * h2.transpose(0, 1, 3, 2)          # <pq|rs>: a+_p a+_q a_r a_s = (r <-> s relabelled) a+_p a+_q a_s a_r
    g = w - w.transpose(0, 1, 3, 2)
    return 0.5 * (g - g.transpose(1, 0, 2, 3))  # (symmetric under p<->q, r<->s already up to rounding)


def solve(constant: float, h1: np.ndarray, h2: np.ndarray, occupied, conv_tol: float = 1e-10, max_cycle: int = 200,
          diis_space: int = 6, triples: bool = False) -> CCSDResult:
    """CCSD amplitudes and energy for the determinant that occupies the spin orbitals ``occupied``; ``triples``: also
    the (T) energy of ``triples_correction`` from the final amplitudes."""
    nso = h1.shape[0]
    if nso > MAX_SPIN_ORBITALS:
        raise ValueError(f"nbed_amd.ccsd is limited to {MAX_SPIN_ORBITALS} spin orbitals (got {nso})")
    occ = np.array(sorted(int(i) for i in occupied))
    vir = np.array([p for p in range(nso) if p not in set(occ.tolist())])
    g = antisymmetrized(np.asarray(h2, dtype=float))
    f = np.asarray(h1, dtype=float) + np.einsum("piqi->pq", g[:, occ][:, :, :, occ])
    e_hf = constant + np.trace(h1[np.ix_(occ, occ)]) + 0.5 * np.einsum("ijij->", g[np.ix_(occ, occ, occ, occ)])
    o, v = occ, vir
    fov, foo, fvv = f[np.ix_(o, v)], f[np.ix_(o, o)], f[np.ix_(v, v)]
    eo, ev = np.diag(foo), np.diag(fvv)
    d1 = eo[:, None] - ev[None, :]
    d2 = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    oovv = g[np.ix_(o, o, v, v)]
    oooo = g[np.ix_(o, o, o, o)]
    vvvv = g[np.ix_(v, v, v, v)]
    ovvo = g[np.ix_(o, v, v, o)]
    ovov = g[np.ix_(o, v, o, v)]
    ooov = g[np.ix_(o, o, o, v)]
    ovvv = g[np.ix_(o, v, v, v)]
    vvvo = g[np.ix_(v, v, v, o)]
    ovoo = g[np.ix_(o, v, o, o)]
    t1 = np.zeros_like(d1)
    t2 = oovv / d2
    no, nv = len(o), len(v)
    fov_od = fov
    foo_od = foo - np.diag(eo)
    fvv_od = fvv - np.diag(ev)

    def energy(t1, t2):
        return (np.einsum("ia,ia->", fov, t1) + 0.25 * np.einsum("ijab,ijab->", oovv, t2)
                + 0.5 * np.einsum("ijab,ia,jb->", oovv, t1, t1))

    hist_t, hist_e = [], []
    e_old = energy(t1, t2)
    converged = False
    it = 0
    for it in range(1, max_cycle + 1):
        tau_t = t2 + 0.5 * (np.einsum("ia,jb->ijab", t1, t1) - np.einsum("ib,ja->ijab", t1, t1))
        tau = t2 + np.einsum("ia,jb->ijab", t1, t1) - np.einsum("ib,ja->ijab", t1, t1)
        # intermediates (eqs. 3-8 of Stanton et al.), off-diagonal Fock terms kept
        fae = fvv_od - 0.5 * np.einsum("me,ma->ae", fov_od, t1) + np.einsum("mf,mafe->ae", t1, ovvv) \
            - 0.5 * np.einsum("mnaf,mnef->ae", tau_t, oovv)
        fmi = foo_od + 0.5 * np.einsum("ie,me->mi", t1, fov_od) + np.einsum("ne,mnie->mi", t1, ooov) \
            + 0.5 * np.einsum("inef,mnef->mi", tau_t, oovv)
        fme = fov_od + np.einsum("nf,mnef->me", t1, oovv)
        wmnij = oooo + np.einsum("je,mnie->mnij", t1, ooov) - np.einsum("ie,mnje->mnij", t1, ooov) \
            + 0.25 * np.einsum("ijef,mnef->mnij", tau, oovv)
        wabef = vvvv - np.einsum("mb,amef->abef", t1, -ovvv.transpose(1, 0, 2, 3)) \
            + np.einsum("ma,bmef->abef", t1, -ovvv.transpose(1, 0, 2, 3)) \
            + 0.25 * np.einsum("mnab,mnef->abef", tau, oovv)
        wmbej = ovvo + np.einsum("jf,mbef->mbej", t1, ovvv) - np.einsum("nb,mnej->mbej", t1, -ooov.transpose(0, 1, 3, 2)) \
            - np.einsum("jnfb,mnef->mbej", 0.5 * t2 + np.einsum("jf,nb->jnfb", t1, t1), oovv)
        # T1 (eq. 1)
        r1 = fov.copy() + np.einsum("ie,ae->ia", t1, fae) - np.einsum("ma,mi->ia", t1, fmi) \
            + np.einsum("imae,me->ia", t2, fme) - np.einsum("nf,naif->ia", t1, ovov) \
            - 0.5 * np.einsum("imef,maef->ia", t2, ovvv) - 0.5 * np.einsum("mnae,nmei->ia", t2, -ooov.transpose(0, 1, 3, 2))
        # T2 (eq. 2)
        r2 = oovv.copy()
        tmp = np.einsum("ijae,be->ijab", t2, fae - 0.5 * np.einsum("mb,me->be", t1, fme))
        r2 += tmp - tmp.transpose(0, 1, 3, 2)
        tmp = np.einsum("imab,mj->ijab", t2, fmi + 0.5 * np.einsum("je,me->mj", t1, fme))
        r2 -= tmp - tmp.transpose(1, 0, 2, 3)
        r2 += 0.5 * np.einsum("mnab,mnij->ijab", tau, wmnij) + 0.5 * np.einsum("ijef,abef->ijab", tau, wabef)
        tmp = np.einsum("imae,mbej->ijab", t2, wmbej) - np.einsum("ie,ma,mbej->ijab", t1, t1, ovvo)
        r2 += tmp - tmp.transpose(1, 0, 2, 3) - tmp.transpose(0, 1, 3, 2) + tmp.transpose(1, 0, 3, 2)
        tmp = np.einsum("ie,abej->ijab", t1, vvvo)
        r2 += tmp - tmp.transpose(1, 0, 2, 3)
        tmp = np.einsum("ma,mbij->ijab", t1, ovoo)
        r2 -= tmp - tmp.transpose(0, 1, 3, 2)
        t1_new, t2_new = r1 / d1, r2 / d2
        # DIIS on the amplitudes (as PySCF's CCSD does)
        vec = np.concatenate([t1_new.ravel(), t2_new.ravel()])
        err = vec - np.concatenate([t1.ravel(), t2.ravel()])
        hist_t.append(vec)
        hist_e.append(err)
        hist_t, hist_e = hist_t[-diis_space:], hist_e[-diis_space:]
        if len(hist_t) > 1:
            m = len(hist_t)
            b = -np.ones((m + 1, m + 1))
            b[m, m] = 0.0
            for i in range(m):
                for j in range(m):
                    b[i, j] = hist_e[i] @ hist_e[j]
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            try:
                c = np.linalg.solve(b, rhs)[:m]
                vec = sum(ci * ti for ci, ti in zip(c, hist_t))
            except np.linalg.LinAlgError:
                pass
        t1, t2 = vec[: no * nv].reshape(no, nv), vec[no * nv:].reshape(no, no, nv, nv)
        e_new = energy(t1, t2)
        if abs(e_new - e_old) < conv_tol and np.abs(err).max() < max(conv_tol, 1e-9) * 10:
            converged = True
            e_old = e_new
            break
        e_old = e_new
    e_t = triples_correction(h1, h2, occ, t1, t2) if triples else None
    return CCSDResult(e_hf, e_old, t1, t2, converged, it, e_t)


# ---------------------------------------------------------------------------------------------------- (T)
def spin_block_eigh(f: np.ndarray, spins):
    """Eigenvalues and eigenvectors of the symmetric block ``f`` over spin orbitals of the given spins (0 | 1), one
    eigenproblem per spin: ``(eps, u)`` with u[p, q] != 0 only for spin(p) = spin(q), the new orbitals of a spin at the
    positions of the old ones.  Alpha never mixes with beta, degenerate alpha/beta pairs included."""
    spins = np.asarray(spins, dtype=int)
    n = len(spins)
    eps, u = np.zeros(n), np.zeros((n, n))
    for s in (0, 1):
        idx = np.flatnonzero(spins == s)
        if idx.size:
            e, c = np.linalg.eigh(0.5 * (f[np.ix_(idx, idx)] + f[np.ix_(idx, idx)].T))
            eps[idx] = e
            u[np.ix_(idx, idx)] = c
    return eps, u


def semicanonical_blocks(t1, t2, fov, foo, fvv, oovv, ovvv, ovoo, occ_spins, vir_spins) -> dict:
    """What (T) reads, rotated into the basis that diagonalises f_oo and f_vv for each spin: ``t1``, ``t2``, ``fov``,
    ``oovv``, ``ovvv`` (= -<vo||vv> transposed), ``ovoo`` and the eigenvalues ``eo``, ``ev``."""
    eo, uo = spin_block_eigh(np.asarray(foo, dtype=float), occ_spins)
    ev, uv = spin_block_eigh(np.asarray(fvv, dtype=float), vir_spins)
    return {
        "eo": eo, "ev": ev,
        "t1": uo.T @ t1 @ uv,
        "fov": uo.T @ fov @ uv,
        "t2": np.einsum("ijab,ip,jq,ar,bs->pqrs", t2, uo, uo, uv, uv, optimize=True),
        "oovv": np.einsum("ijab,ip,jq,ar,bs->pqrs", oovv, uo, uo, uv, uv, optimize=True),
        "ovvv": np.einsum("iabc,ip,aq,br,cs->pqrs", ovvv, uo, uv, uv, uv, optimize=True),
        "ovoo": np.einsum("iajk,ip,aq,jr,ks->pqrs", ovoo, uo, uv, uo, uo, optimize=True),
    }


def triples_sum(blocks: dict, absolute: bool = False) -> float:
    """sum_{i<j<k} sum_{a<b<c} w (w + t_d) / D over semicanonical ``blocks``, one (i, j, k) cube at a time, with

        w   = P(i/jk) P(a/bc) [ sum_e t_jk^ae <ei||bc> - sum_m t_im^bc <ma||jk> ]
        t_d = P(i/jk) P(a/bc) [ t_i^a <jk||bc> + f_ia t_jk^bc ],    P(p/qr) g(pqr) = g(pqr) - g(qpr) - g(rqp).

    ``absolute``: the same arithmetic on the absolute values of every operand with every sign a plus -- the sum S of
    the forward rounding bound the device tests use."""
    x = (lambda a: np.abs(a)) if absolute else (lambda a: a)
    sg = 1.0 if absolute else -1.0
    t1, t2, fov, oovv, ovvv, ovoo = (x(blocks[k]) for k in ("t1", "t2", "fov", "oovv", "ovvv", "ovoo"))
    eo, ev = blocks["eo"], blocks["ev"]
    no, nv = t1.shape
    if no < 3 or nv < 3:
        return 0.0
    dv = ev[:, None, None] + ev[None, :, None] + ev[None, None, :]
    ia, ib, ic = np.meshgrid(np.arange(nv), np.arange(nv), np.arange(nv), indexing="ij")
    keep = (ia < ib) & (ib < ic)

    def perm_abc(g):  # P(a/bc)
        return g + sg * g.transpose(1, 0, 2) + sg * g.transpose(2, 1, 0)

    def connected(p, q, r):  # (p|qr): -sum_e t2[q,r,a,e] ovvv[p,e,b,c] - sum_m ovoo[m,a,q,r] t2[p,m,b,c]
        return sg * np.einsum("ae,ebc->abc", t2[q, r], ovvv[p]) + sg * np.einsum("ma,mbc->abc", ovoo[:, :, q, r], t2[p])

    def disconnected(p, q, r):
        return t1[p][:, None, None] * oovv[q, r][None] + fov[p][:, None, None] * t2[q, r][None]

    total = 0.0
    for i in range(no):
        for j in range(i + 1, no):
            for k in range(j + 1, no):
                w = perm_abc(connected(i, j, k) + sg * connected(j, i, k) + sg * connected(k, j, i))
                td = perm_abc(disconnected(i, j, k) + sg * disconnected(j, i, k) + sg * disconnected(k, j, i))
                d = (eo[i] + eo[j] + eo[k]) - dv
                if absolute:
                    d = np.abs(d)
                total += float(np.sum((w * (w + td) / d)[keep]))
    return total


def triples_correction(h1: np.ndarray, h2: np.ndarray, occupied, t1: np.ndarray, t2: np.ndarray) -> float:
    """The (T) energy of CCSD amplitudes in ``solve``'s layout for a general (non-HF, non-canonical) reference: the
    fourth-order triples energy with the f_ov term (Watts, Gauss, Bartlett, J. Chem. Phys. 98, 8718 (1993)) after a
    semicanonical rotation of the occupied and virtual spin orbitals, spin by spin.  What PySCF users get from
    ``cc.ccsd_t()`` on the object of nbed/driver.py:1105-1135.  0.0 below three occupied or three virtual spin orbitals."""
    nso = h1.shape[0]
    if nso > MAX_SPIN_ORBITALS:
        raise ValueError(f"nbed_amd.ccsd is limited to {MAX_SPIN_ORBITALS} spin orbitals (got {nso})")
    occ = np.array(sorted(int(i) for i in occupied), dtype=int)
    vir = np.array([p for p in range(nso) if p not in set(occ.tolist())], dtype=int)
    if len(occ) < 3 or len(vir) < 3:
        return 0.0
    g = antisymmetrized(np.asarray(h2, dtype=float))
    f = np.asarray(h1, dtype=float) + np.einsum("piqi->pq", g[:, occ][:, :, :, occ])
    o, v = occ, vir
    blocks = semicanonical_blocks(np.asarray(t1, dtype=float), np.asarray(t2, dtype=float), f[np.ix_(o, v)], f[np.ix_(o, o)],
                                  f[np.ix_(v, v)], g[np.ix_(o, o, v, v)], g[np.ix_(o, v, v, v)], g[np.ix_(o, v, o, o)],
                                  occ & 1, vir & 1)
    return triples_sum(blocks)
