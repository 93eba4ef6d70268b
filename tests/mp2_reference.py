"""References for nbed_amd.mp2, independent of the code under test.

(a) ``loops``: the definitions of the nbed_amd/mp2.py docstring restated element by element in ``np.longdouble``, as
    plain loops over the spin orbitals of ``(h1, h2, occupied)``, spin case by spin case in the chemist integrals
    (ia|jb) -- not the antisymmetrised all-spin-orbital form ``mp2.solve`` uses.

(b) ``fci_second_order``: no second implementation of MP2 at all.  With H0 the one-body operator f_oo + f_vv of the
    reference determinant and H(l) = H0 + l (H - H0), the ground state of H(l) from the host ``fci`` module gives
        E(2) = 1/2 E''(0)                                   by the symmetric stencil [E(l) - 2 E(0) + E(-l)] / (2 l^2),
        D_vv = [gamma_vv(l) + gamma_vv(-l)] / (2 l^2)       from ``rdm1`` (gamma_vv = l^2 D + O(l^4) in the even part),
    each at the two step sizes ``STEPS``.  Both cover the singles term and a non-canonical reference, since H - H0 holds
    f_ov and nothing assumes f diagonal.
"""

import copy

import numpy as np

from nbed_amd import fci

LD = np.longdouble
H4 = "4\n\nH 0 0 0\nH 0 0 0.9\nH 0 0 1.8\nH 0 0 2.7"  # linear, 0.9 A apart (tests/ccsd_lambda_reference.py)
STEPS = (0.004, 0.002)


# ---------------------------------------------------------------------------------------------------- (a)
def _fock_and_coulomb(h1, h2, occ):
    """f (longdouble) of the determinant and <pq|rs> = 2 h2[p,q,s,r]."""
    h1, h2 = np.asarray(h1, dtype=LD), np.asarray(h2, dtype=LD)
    coul = 2 * h2.transpose(0, 1, 3, 2)  # <pq|rs>
    f = h1.copy()
    for i in occ:
        f += coul[:, i, :, i] - coul[:, i, i, :]
    return f, coul


def _semicanonical(f, idx):
    """Orthogonal u over the spin orbitals ``idx`` (block diagonal in spin, double-precision eigenvectors) and the
    diagonal of u^T f u in longdouble."""
    idx = np.asarray(idx)
    u = np.zeros((len(idx), len(idx)), dtype=LD)
    for s in (0, 1):
        k = np.flatnonzero((idx & 1) == s)
        if k.size:
            blk = np.asarray(f[np.ix_(idx[k], idx[k])], dtype=float)
            u[np.ix_(k, k)] = np.linalg.eigh(0.5 * (blk + blk.T))[1]
    return u


def loops(constant, h1, h2, occupied) -> dict:
    """``e_singles``, ``e_same``, ``e_opposite``, ``e_corr`` (floats) and ``dvv`` (two arrays, the input virtual basis of
    each spin) by the definitions, in longdouble."""
    nso = h1.shape[0]
    occ = np.array(sorted(int(i) for i in occupied))
    vir = np.array([p for p in range(nso) if p not in set(occ.tolist())])
    f, coul = _fock_and_coulomb(h1, h2, occ)
    uo, uv = _semicanonical(f, occ), _semicanonical(f, vir)
    foo = uo.T @ f[np.ix_(occ, occ)] @ uo
    fvv = uv.T @ f[np.ix_(vir, vir)] @ uv
    fov = uo.T @ f[np.ix_(occ, vir)] @ uv
    eo, ev = np.diag(foo), np.diag(fvv)
    # (ia|jb) = <ij|ab> in the semicanonical spin orbitals
    x = coul[np.ix_(occ, occ, vir, vir)]
    x = np.tensordot(uo.T, x, (1, 0))
    x = np.tensordot(uo.T, x, (1, 1)).transpose(1, 0, 2, 3)
    x = np.tensordot(x, uv, (2, 0)).transpose(0, 1, 3, 2)
    x = np.tensordot(x, uv, (3, 0))
    chem = x.transpose(0, 2, 1, 3)  # [i, a, j, b]
    so, sv = occ & 1, vir & 1
    no, nv = len(occ), len(vir)
    e_s = e_same = e_opp = LD(0)
    t1 = np.zeros((no, nv), dtype=LD)
    for i in range(no):
        for a in range(nv):
            if so[i] == sv[a]:
                t1[i, a] = fov[i, a] / (eo[i] - ev[a])
                e_s += fov[i, a] * t1[i, a]
    dens = np.zeros((nv, nv), dtype=LD)
    for a in range(nv):
        for b in range(nv):
            if sv[a] == sv[b]:
                for i in range(no):
                    dens[a, b] += t1[i, a] * t1[i, b]
    t = np.zeros((no, nv, no, nv), dtype=LD)  # t[i, a, j, b], a of the spin of i and b of the spin of j
    for i in range(no):
        for j in range(no):
            for a in range(nv):
                for b in range(nv):
                    if so[i] != sv[a] or so[j] != sv[b]:
                        continue
                    d = ((eo[i] + eo[j]) - ev[a]) - ev[b]
                    if so[i] == so[j]:
                        g = chem[i, a, j, b] - chem[i, b, j, a]
                        t[i, a, j, b] = g / d
                        e_same += t[i, a, j, b] * g / 4
                    else:
                        t[i, a, j, b] = chem[i, a, j, b] / d
                        if so[i] == 0:  # i alpha, J beta: once
                            e_opp += t[i, a, j, b] * chem[i, a, j, b]
    for a in range(nv):
        for b in range(nv):
            if sv[a] != sv[b]:
                continue
            acc = LD(0)
            for i in range(no):
                if so[i] != sv[a]:
                    continue
                for j in range(no):
                    w = LD(0.5) if so[j] == so[i] else LD(1)
                    for c in range(nv):
                        if sv[c] == so[j]:
                            acc += w * t[i, a, j, c] * t[i, b, j, c]
            dens[a, b] += acc
    dens = uv @ dens @ uv.T
    dvv = [np.asarray(dens[np.ix_(np.flatnonzero(sv == s), np.flatnonzero(sv == s))], dtype=float) for s in (0, 1)]
    return {"e_singles": float(e_s), "e_same": float(e_same), "e_opposite": float(e_opp),
            "e_corr": float(e_s + e_same + e_opp), "dvv": dvv}


# ---------------------------------------------------------------------------------------------------- (b)
def fci_second_order(constant, h1, h2, occupied) -> dict:
    """``e_corr`` and ``dvv`` at each step of ``STEPS`` (lists, in that order) from the ground states of H(+-l)."""
    nso = h1.shape[0]
    occ = np.array(sorted(int(i) for i in occupied))
    vir = np.array([p for p in range(nso) if p not in set(occ.tolist())])
    f, _ = _fock_and_coulomb(h1, h2, occ)
    f = np.asarray(f, dtype=float)
    h0 = np.zeros_like(f)
    h0[np.ix_(occ, occ)] = f[np.ix_(occ, occ)]
    h0[np.ix_(vir, vir)] = f[np.ix_(vir, vir)]
    nelec = (int(np.sum(occ % 2 == 0)), int(np.sum(occ % 2 == 1)))

    def state(lam):
        return fci.ground_state(lam * constant, h0 + lam * (np.asarray(h1, dtype=float) - h0), lam * np.asarray(h2, dtype=float), nelec)

    zero = state(0.0)
    dm0 = zero.rdm1()
    ref_occ = np.zeros(nso)
    ref_occ[occ] = 1.0
    got = np.array([dm0[p & 1, p >> 1, p >> 1] for p in range(nso)])
    assert np.max(np.abs(got - ref_occ)) < 1e-10, "the ground state of H0 is not the reference determinant"
    va, vb = vir[vir % 2 == 0] >> 1, vir[vir % 2 == 1] >> 1
    e_corr, dvv = [], []
    for lam in STEPS:
        plus, minus = state(lam), state(-lam)
        e_corr.append((plus.e_tot - 2.0 * zero.e_tot + minus.e_tot) / (2.0 * lam * lam))
        gp, gm = plus.rdm1(), minus.rdm1()
        dvv.append([(gp[s][np.ix_(v, v)] + gm[s][np.ix_(v, v)]) / (2.0 * lam * lam) for s, v in ((0, va), (1, vb))])
    return {"e_corr": e_corr, "dvv": dvv}


# ---------------------------------------------------------------------------------------------------- fixtures' helpers
def occupied_of(scf_obj):
    mo_occ = np.asarray(scf_obj.mo_occ)
    if mo_occ.ndim == 1:
        mo_occ = np.array((mo_occ > 0, mo_occ > 1), dtype=float)
    return [2 * int(i) for i in np.flatnonzero(mo_occ[0] > 0)] + [2 * int(i) + 1 for i in np.flatnonzero(mo_occ[1] > 0)]


def restricted_copy(scf_obj, be):
    """A restricted object (2-D ``mo_coeff``, occupations 0 | 2) with the alpha orbitals of a closed-shell unrestricted
    one, on the same integrals."""
    from nbed_amd.scf import GpuRHF

    occ = np.asarray(scf_obj.mo_occ)
    assert np.array_equal(occ[0], occ[1])
    factor = scf_obj.eri_factor_device()
    kw = dict(eri_factor=factor) if factor is not None else dict(eri=scf_obj.eri_device())
    out = GpuRHF(scf_obj.mol, scf_obj.get_ovlp(), scf_obj.get_hcore(), backend=be, **kw)
    out.mo_coeff = np.array(np.asarray(scf_obj.mo_coeff)[0])
    out.mo_occ = 2.0 * occ[0]
    out.mo_energy = np.array(np.asarray(scf_obj.mo_energy)[0])
    out.e_tot = scf_obj.e_tot
    return out


def random_orthogonal(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def rotated(scf_obj, seed, within=True, angle=0.0):
    """A copy of an unrestricted SCF object with rotated orbitals, different in the two spins: ``within`` -- a random
    orthogonal rotation inside the occupied and inside the virtual space (the determinant is the same one);
    ``angle`` != 0 -- then a rotation exp(angle * A), A antisymmetric between occupied and virtual (another determinant:
    f_ov != 0).  ``(copy, [U_virtual_alpha, U_virtual_beta])`` with C_v' = C_v U_v for the within-space part."""
    rng = np.random.default_rng(seed)
    out = scf_obj.copy()
    c = np.array(np.asarray(scf_obj.mo_coeff), dtype=float)
    occ = np.asarray(scf_obj.mo_occ) > 0
    assert c.ndim == 3
    uvs = []
    for s in (0, 1):
        o, v = np.flatnonzero(occ[s]), np.flatnonzero(~occ[s])
        u = np.eye(c.shape[2])
        if within:
            u[np.ix_(o, o)] = random_orthogonal(len(o), rng)
            u[np.ix_(v, v)] = random_orthogonal(len(v), rng)
        uvs.append(u[np.ix_(v, v)].copy())
        if angle:
            a = np.zeros_like(u)
            a[np.ix_(o, v)] = angle * rng.standard_normal((len(o), len(v)))
            a = a - a.T
            w, z = np.linalg.eigh(1j * a)  # exp(a) of the real antisymmetric a
            u = u @ np.real((z * np.exp(-1j * w)) @ z.conj().T)
        c[s] = c[s] @ u
    out.mo_coeff = c
    out.mo_occ = copy.deepcopy(np.asarray(scf_obj.mo_occ))
    out.e_tot = out.energy_tot()
    return out, uvs
