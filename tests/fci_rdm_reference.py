"""Reference for the FCI densities (nbed_amd/fci_gpu.py, nbed_amd/fci.py): spin-resolved 1- and 2-particle (transition)
density matrices straight from the operator definition

    dm1[s][p,q] = <b| a+_ps a_qs |c>        dm2[x][p,q,r,s] = <b| a+_ps a+_qt a_rt a_ss |c>,  (s,t) = aa, bb, ab

in the determinant basis of tests/fci_reference.py (alpha creators ascending, then beta creators ascending, on the
vacuum; index Ia * Nb + Ib) -- operators applied to bit masks one at a time, no generators, no link tables, no D.
No GPU needed."""

import numpy as np

from fci_reference import EPS, Sector, _add, _remove

BLOCKS = ((0, 0), (1, 1), (0, 1))  # (spin of p and s, spin of q and r) of dm2[x]


def rdm_tolerance(ndet: int, b, c) -> float:
    """Per-element bound on a device density: (ndet + 8) eps |b|_2 |c|_2.  A row of D is a signed sub-permutation of the
    vector, so its 2-norm is at most the vector's; a length-K dot product in any summation order errs by at most
    K eps |row_b| |row_c|; the additions number ndet - 1 however the reduction is cut into chunks and slabs; the 8
    covers the delta subtraction and FMA differences."""
    return (ndet + 8) * EPS * float(np.linalg.norm(np.ravel(b))) * float(np.linalg.norm(np.ravel(c)))


def _flat(sec, v):
    flat = np.asarray(v, dtype=float).reshape(-1)
    assert flat.size == sec.ndet
    return flat


def rdm12(n, nelec, c, bra=None, two_particle=True):
    """(dm1 (2,n,n), dm2 (3,n,n,n,n)), every element; ``bra`` None is the state density of ``c``.  ``two_particle``
    False leaves dm2 zero (dm1 alone, for sectors where all of dm2 would take too long)."""
    sec = Sector(n, nelec)
    ket_v = _flat(sec, c)
    bra_v = ket_v if bra is None else _flat(sec, bra)
    dm1, dm2 = np.zeros((2, n, n)), np.zeros((3, n, n, n, n))
    for j in range(sec.ndet):
        cj = ket_v[j]
        ket = sec.mask(j)
        occ = [bit for bit in range(2 * n) if (ket >> bit) & 1]
        for sbit in occ:  # a_S acts first
            ss, s = divmod(sbit, n)
            s1, d1 = _remove(ket, sbit)
            for p in range(n):
                pbit = p + ss * n
                if (d1 >> pbit) & 1:
                    continue
                s2, out = _add(d1, pbit)
                dm1[ss, p, s] += s1 * s2 * bra_v[sec.index(out)] * cj
            for rbit in occ if two_particle else ():
                sr, r = divmod(rbit, n)
                if rbit == sbit or (ss, sr) not in BLOCKS:
                    continue
                x = BLOCKS.index((ss, sr))
                s2, d2 = _remove(d1, rbit)
                for q in range(n):
                    qbit = q + sr * n
                    if (d2 >> qbit) & 1:
                        continue
                    s3, d3 = _add(d2, qbit)
                    for p in range(n):
                        pbit = p + ss * n
                        if (d3 >> pbit) & 1:
                            continue
                        s4, out = _add(d3, pbit)
                        dm2[x, p, q, r, s] += s1 * s2 * s3 * s4 * bra_v[sec.index(out)] * cj
    return dm1, dm2


def dm1_element(sec: Sector, c, bra, spin, p, q) -> float:
    """<bra| a+_p a_q |c> for one spin."""
    n = sec.n
    ket_v, bra_v = _flat(sec, c), _flat(sec, bra)
    pbit, qbit = p + spin * n, q + spin * n
    acc = 0.0
    for j in range(sec.ndet):
        ket = sec.mask(j)
        if not (ket >> qbit) & 1:
            continue
        s1, d1 = _remove(ket, qbit)
        if (d1 >> pbit) & 1:
            continue
        s2, out = _add(d1, pbit)
        acc += s1 * s2 * bra_v[sec.index(out)] * ket_v[j]
    return acc


def dm2_element(sec: Sector, c, bra, x, p, q, r, s) -> float:
    """<bra| a+_ps a+_qt a_rt a_ss |c> for the block x of BLOCKS."""
    n = sec.n
    ket_v, bra_v = _flat(sec, c), _flat(sec, bra)
    sp, sq = BLOCKS[x]
    pbit, qbit, rbit, sbit = p + sp * n, q + sq * n, r + sq * n, s + sp * n
    if rbit == sbit or pbit == qbit:
        return 0.0
    acc = 0.0
    for j in range(sec.ndet):
        ket = sec.mask(j)
        if not ((ket >> sbit) & 1 and (ket >> rbit) & 1):
            continue
        s1, d1 = _remove(ket, sbit)
        s2, d2 = _remove(d1, rbit)
        if (d2 >> qbit) & 1 or (d2 >> pbit) & 1:
            continue
        s3, d3 = _add(d2, qbit)
        s4, out = _add(d3, pbit)
        acc += s1 * s2 * s3 * s4 * bra_v[sec.index(out)] * ket_v[j]
    return acc
