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

    def __init__(self, e_hf, e_corr, t1, t2, converged, iterations, e_t=None, l1=None, l2=None, lambda_converged=None,
                 lambda_iterations=None, dm1=None):
        self.e_hf = float(e_hf)
        self.e_corr = float(e_corr)
        self.e_tot = float(e_hf + e_corr)
        self.t1, self.t2 = t1, t2
        self.converged = bool(converged)
        self.iterations = int(iterations)
        self.e_t = None if e_t is None else float(e_t)
        self.e_tot_t = None if e_t is None else self.e_tot + self.e_t
        # the left-hand state and its density (``solve(..., density=True)``; None otherwise)
        self.l1, self.l2 = l1, l2
        self.lambda_converged = None if lambda_converged is None else bool(lambda_converged)
        self.lambda_iterations = None if lambda_iterations is None else int(lambda_iterations)
        self._dm1 = dm1

    def rdm1(self) -> np.ndarray:
        """(2, n, n): dm1[s, p, q] = <a+_{p s} a_{q s}> of CCSD, the convention of ``FCIResult.rdm1`` (spin orbital
        2p + s, alpha even): the symmetric part of the orbital-unrelaxed response density
        <0|(1 + Lambda) e^{-T} a+_p a_q e^{T}|0>, the occupations of the reference determinant included.  With
        ``triples`` it still is the CCSD density: (T) has none here."""
        if self._dm1 is None:
            raise ValueError("this CCSD result has no density: solve(..., density=True) solves the Lambda equations "
                             "and builds it")
        return self._dm1.copy()

    def natural_occupations(self) -> np.ndarray:
        """Eigenvalues of the spin-summed ``rdm1``, descending (as ``FCIResult.natural_occupations``)."""
        dm = self.rdm1()
        return np.linalg.eigvalsh(dm[0] + dm[1])[::-1].copy()


def antisymmetrized(h2: np.ndarray) -> np.ndarray:
    """<pq||rs> from the two-body tensor of ``build()``:  H_2 = 1/4 sum <pq||rs> a+_p a+_q a_s a_r."""
    w = 2.0 * h2.transpose(0, 1, 3, 2)          # <pq|rs>: a+_p a+_q a_r a_s = (r <-> s relabelled) a+_p a+_q a_s a_r
    g = w - w.transpose(0, 1, 3, 2)
    return 0.5 * (g - g.transpose(1, 0, 2, 3))  # (symmetric under p<->q, r<->s already up to rounding)


def solve(constant: float, h1: np.ndarray, h2: np.ndarray, occupied, conv_tol: float = 1e-10, max_cycle: int = 200,
          diis_space: int = 6, triples: bool = False, density: bool = False) -> CCSDResult:
    """CCSD amplitudes and energy for the determinant that occupies the spin orbitals ``occupied``; ``triples``: also
    the (T) energy of ``triples_correction`` from the final amplitudes; ``density``: also the Lambda amplitudes
    (``solve_lambda``) and the one-particle density of ``CCSDResult.rdm1`` -- CCSD's, with or without ``triples``."""
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
    extra = {}
    if density:
        blocks = dict(oovv=oovv, oooo=oooo, vvvv=vvvv, ovvo=ovvo, ooov=ooov, ovvv=ovvv, vvvo=vvvo)
        l1, l2, l_conv, l_it = solve_lambda(t1, t2, fov, foo_od, fvv_od, d1, d2, blocks, conv_tol, max_cycle, diis_space)
        dm1, _ = spin_resolved_density(density_blocks(t1, t2, l1, l2), occ, vir, nso)
        extra = dict(l1=l1, l2=l2, lambda_converged=l_conv, lambda_iterations=l_it, dm1=dm1)
    return CCSDResult(e_hf, e_old, t1, t2, converged, it, e_t, **extra)


# ---------------------------------------------------------------------------------------------------- Lambda
CROSS_SPIN_TOL = 1e-10


def _p_ij(x):
    return x - x.transpose(1, 0, 2, 3)


def _p_ab(x):
    return x - x.transpose(0, 1, 3, 2)


def lambda_intermediates(t1, t2, fov, foo_od, fvv_od, blocks) -> dict:
    """The elements of e^{-T} H e^{T} the Lambda equations read (Gauss, Stanton, J. Chem. Phys. 103, 3561 (1995),
    spin-orbital form, general Fock matrix), none of which depends on Lambda: they are built once.  ``foo_od`` and
    ``fvv_od`` are f_oo and f_vv without their diagonals, which the denominators carry.  W_abef is not among them, and
    W_abei comes without its t_if W_abef term: both are folded into the ladder of ``lambda_residual``.

        F_me   = f_me + t_nf <mn||ef>
        F_ae   = f_ae - 1/2 f_me t_ma + t_mf <ma||fe> - 1/2 tau~_mnaf <mn||ef> - 1/2 t_ma F_me
        F_mi   = f_mi + 1/2 t_ie f_me + t_ne <mn||ie> + 1/2 tau~_inef <mn||ef> + 1/2 t_ie F_me
        W_mnij = <mn||ij> + P(ij) t_je <mn||ie> + 1/2 tau_ijef <mn||ef>
        W_mbej = <mb||ej> + t_jf <mb||ef> + t_nb <mn||je> - (t_jnfb + t_jf t_nb) <mn||ef>
        W_mnie = <mn||ie> + t_if <mn||fe>
        W_maef = <ma||ef> - t_na <mn||ef>                                          (= -W_amef)
        W_mbij = <ij||mb> - F_me t_ijbe - t_nb W_mnij + 1/2 <mb||ef> tau_ijef
                 + P(ij) [ <mn||ie> t_jnbe + t_ie (<mb||ej> - t_njbf <mn||ef>) ]
        W_abei = <ab||ei> - F_me t_miab - 1/2 <mn||ie> tau_mnab
                 - P(ab) [ <mb||ef> t_miaf + t_ma (<mb||ei> - t_nibf <mn||ef>) ]      (+ t_if W_abef: see above)
    """
    oovv, oooo, ovvo, ooov, ovvv, vvvo = (blocks[k] for k in ("oovv", "oooo", "ovvo", "ooov", "ovvv", "vvvo"))
    pair = np.einsum("ia,jb->ijab", t1, t1)
    tau = t2 + pair - pair.transpose(0, 1, 3, 2)
    tau_t = t2 + 0.5 * (pair - pair.transpose(0, 1, 3, 2))
    fme = fov + np.einsum("nf,mnef->me", t1, oovv)
    fae = fvv_od - 0.5 * np.einsum("me,ma->ae", fov, t1) + np.einsum("mf,mafe->ae", t1, ovvv) \
        - 0.5 * np.einsum("mnaf,mnef->ae", tau_t, oovv) - 0.5 * np.einsum("ma,me->ae", t1, fme)
    fmi = foo_od + 0.5 * np.einsum("ie,me->mi", t1, fov) + np.einsum("ne,mnie->mi", t1, ooov) \
        + 0.5 * np.einsum("inef,mnef->mi", tau_t, oovv) + 0.5 * np.einsum("ie,me->mi", t1, fme)
    wmnij = oooo + np.einsum("je,mnie->mnij", t1, ooov) - np.einsum("ie,mnje->mnij", t1, ooov) \
        + 0.5 * np.einsum("ijef,mnef->mnij", tau, oovv)
    wmbej = ovvo + np.einsum("jf,mbef->mbej", t1, ovvv) + np.einsum("nb,mnje->mbej", t1, ooov) \
        - np.einsum("jnfb,mnef->mbej", t2 + pair, oovv)
    wmnie = ooov + np.einsum("if,mnfe->mnie", t1, oovv)
    wmaef = ovvv - np.einsum("na,mnef->maef", t1, oovv)
    ring = ovvo - np.einsum("njbf,mnef->mbej", t2, oovv)
    wmbij = ooov.transpose(2, 3, 0, 1) - np.einsum("me,ijbe->mbij", fme, t2) - np.einsum("nb,mnij->mbij", t1, wmnij) \
        + 0.5 * np.einsum("mbef,ijef->mbij", ovvv, tau)
    tmp = np.einsum("mnie,jnbe->mbij", ooov, t2) + np.einsum("ie,mbej->mbij", t1, ring)
    wmbij += tmp - tmp.transpose(0, 1, 3, 2)
    wabei = vvvo - np.einsum("me,miab->abei", fme, t2) - 0.5 * np.einsum("mnie,mnab->abei", ooov, tau)
    tmp = np.einsum("mbef,miaf->abei", ovvv, t2) + np.einsum("ma,mbei->abei", t1, ring)
    wabei -= tmp - tmp.transpose(1, 0, 2, 3)
    return dict(tau=tau, fme=fme, fae=fae, fmi=fmi, wmnij=wmnij, wmbej=wmbej, wmnie=wmnie, wmaef=wmaef, wmbij=wmbij,
                wabei=wabei)


def lambda_residual(l1, l2, t1, t2, blocks, im):
    """Right-hand sides (r1, r2) of the Lambda equations, lambda_new = r / D:

        r1_ia   = F_ia + l_ie F_ea - l_ma F_im + l_me W_ieam + 1/2 l_imef W_efam + L_imae t_me - 1/2 l_mnae W_iemn
                  + G_ef W_iefa - G_mn W_mina
        r2_ijab = <ij||ab> + P(ab) l_ijae F_eb - P(ij) l_imab F_jm + 1/2 l_mnab W_ijmn + L_ijab - P(ij) l_ie W_jeab
                  - P(ab) l_ma W_ijmb + P(ij) P(ab) [ l_imae W_jebm + l_ia F_jb ] + P(ab) <ij||ae> G_be
                  - P(ij) <im||ab> G_mj
        G_ae    = -1/2 t_mnef l_mnaf,    G_mi = 1/2 t_mnef l_inef
        L_ijab  = 1/2 l_ijef W_efab = 1/2 l_ijef <ef||ab> + (l_ijef t_mf) <me||ab> + 1/4 (l_ijef tau_mnef) <mn||ab>

    with the W of ``lambda_intermediates`` (W_iefa = W_maef there).  L is the particle-particle ladder: its first
    piece is the only O(o^2 v^4) product, the other two go through an o^3 v and an o^4 intermediate, and L t1 is the
    t_if W_abef term of W_abei in r1."""
    oovv, vvvv, ovvv = blocks["oovv"], blocks["vvvv"], blocks["ovvv"]
    fme, fae, fmi = im["fme"], im["fae"], im["fmi"]
    gae = -0.5 * np.einsum("mnef,mnaf->ae", t2, l2)
    gmi = 0.5 * np.einsum("mnef,inef->mi", t2, l2)
    lad = 0.5 * np.einsum("ijef,efab->ijab", l2, vvvv)
    lad += np.einsum("ijem,meab->ijab", np.einsum("ijef,mf->ijem", l2, t1), ovvv)
    lad += 0.25 * np.einsum("ijmn,mnab->ijab", np.einsum("ijef,mnef->ijmn", l2, im["tau"]), oovv)
    r1 = fme + np.einsum("ie,ea->ia", l1, fae) - np.einsum("ma,im->ia", l1, fmi) \
        + np.einsum("me,ieam->ia", l1, im["wmbej"]) + 0.5 * np.einsum("imef,efam->ia", l2, im["wabei"]) \
        + np.einsum("imae,me->ia", lad, t1) - 0.5 * np.einsum("mnae,iemn->ia", l2, im["wmbij"]) \
        + np.einsum("ef,iefa->ia", gae, im["wmaef"]) - np.einsum("mn,mina->ia", gmi, im["wmnie"])
    r2 = oovv + 0.5 * np.einsum("mnab,ijmn->ijab", l2, im["wmnij"]) + lad
    r2 += _p_ab(np.einsum("ijae,eb->ijab", l2, fae) + np.einsum("ijae,be->ijab", oovv, gae)
                - np.einsum("ma,ijmb->ijab", l1, im["wmnie"]))
    r2 -= _p_ij(np.einsum("imab,jm->ijab", l2, fmi) + np.einsum("imab,mj->ijab", oovv, gmi)
                + np.einsum("ie,jeab->ijab", l1, im["wmaef"]))
    r2 += _p_ij(_p_ab(np.einsum("imae,jebm->ijab", l2, im["wmbej"]) + np.einsum("ia,jb->ijab", l1, fme)))
    return r1, r2


def solve_lambda(t1, t2, fov, foo_od, fvv_od, d1, d2, blocks, conv_tol=1e-10, max_cycle=200, diis_space=6):
    """(l1, l2, converged, cycles): the CCSD Lambda amplitudes, l1 (o, v) and l2 (o, o, v, v) laid out like t1 and t2,
    by the amplitude loop's iteration -- lambda_new = r / D, DIIS of ``diis_space`` from the second stored vector --
    from the first-order left state l1 = t1, l2 = t2, until max |lambda_new - lambda| < 10 max(conv_tol, 1e-9)."""
    im = lambda_intermediates(t1, t2, fov, foo_od, fvv_od, blocks)
    l1, l2 = t1.copy(), t2.copy()
    no, nv = t1.shape
    hist_l, hist_e = [], []
    converged, it = False, 0
    for it in range(1, max_cycle + 1):
        r1, r2 = lambda_residual(l1, l2, t1, t2, blocks, im)
        vec = np.concatenate([(r1 / d1).ravel(), (r2 / d2).ravel()])
        err = vec - np.concatenate([l1.ravel(), l2.ravel()])
        hist_l.append(vec)
        hist_e.append(err)
        hist_l, hist_e = hist_l[-diis_space:], hist_e[-diis_space:]
        if len(hist_l) > 1:
            m = len(hist_l)
            b = -np.ones((m + 1, m + 1))
            b[m, m] = 0.0
            for i in range(m):
                for j in range(m):
                    b[i, j] = hist_e[i] @ hist_e[j]
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            try:
                c = np.linalg.solve(b, rhs)[:m]
                vec = sum(ci * li for ci, li in zip(c, hist_l))
            except np.linalg.LinAlgError:
                pass
        l1, l2 = vec[: no * nv].reshape(no, nv), vec[no * nv:].reshape(no, no, nv, nv)
        if np.abs(err).max() < max(conv_tol, 1e-9) * 10:
            converged = True
            break
    return l1, l2, converged, it


def density_blocks(t1, t2, l1, l2) -> dict:
    """The four blocks of the unrelaxed CCSD response density gamma[p, q] = <0|(1 + Lambda) e^{-T} {a+_p a_q} e^{T}|0>
    over (occupied | virtual) spin orbitals, the reference occupations not included:

        oo[i,j] = -l_ie t_je - 1/2 l_imef t_jmef            vv[a,b] = l_ma t_mb + 1/2 l_mnae t_mnbe
        ov[i,a] = l_ia
        vo[a,i] = t_ia + l_me t_imae - X_mi t_ma - t_ie Y_ae,   X_mi = 1/2 l_mnef t_inef,
                                                                Y_ae = 1/2 l_mnef t_mnaf + l_me t_ma
    """
    x = 0.5 * np.einsum("mnef,inef->mi", l2, t2)
    y = 0.5 * np.einsum("mnef,mnaf->ae", l2, t2) + np.einsum("me,ma->ae", l1, t1)
    return {
        "oo": -np.einsum("ie,je->ij", l1, t1) - 0.5 * np.einsum("imef,jmef->ij", l2, t2),
        "vv": np.einsum("ma,mb->ab", l1, t1) + 0.5 * np.einsum("mnae,mnbe->ab", l2, t2),
        "ov": l1.copy(),
        "vo": t1.T + np.einsum("imae,me->ai", t2, l1) - np.einsum("mi,ma->ai", x, t1) - np.einsum("ie,ae->ai", t1, y),
    }


def spin_resolved_density(blocks: dict, occ, vir, nso: int):
    """(dm1 (2, n, n), max |cross-spin element|) from the blocks of ``density_blocks`` and the spin orbitals they are
    over: the blocks are scattered to the original spin-orbital order, the reference occupations added, the matrix
    symmetrised, and its alpha-alpha and beta-beta parts returned.  The alpha-beta elements vanish for a Hamiltonian of
    the form ``build()`` produces; past ``CROSS_SPIN_TOL`` they are an error, never dropped silently."""
    occ, vir = np.asarray(occ, dtype=int), np.asarray(vir, dtype=int)
    g = np.zeros((nso, nso))
    g[np.ix_(occ, occ)] = blocks["oo"] + np.eye(len(occ))
    g[np.ix_(occ, vir)] = blocks["ov"]
    g[np.ix_(vir, occ)] = blocks["vo"]
    g[np.ix_(vir, vir)] = blocks["vv"]
    cross = float(max(np.abs(g[0::2, 1::2]).max(initial=0.0), np.abs(g[1::2, 0::2]).max(initial=0.0)))
    check_cross_spin(cross)
    g = 0.5 * (g + g.T)
    return np.stack([g[0::2, 0::2], g[1::2, 1::2]]), cross


def check_cross_spin(cross: float) -> None:
    if not cross <= CROSS_SPIN_TOL:
        raise ValueError(f"the CCSD density couples alpha and beta spin orbitals (max |element| {cross:.3e} > "
                         f"{CROSS_SPIN_TOL:g}): the Hamiltonian is not of the spin-block form build() produces")


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
