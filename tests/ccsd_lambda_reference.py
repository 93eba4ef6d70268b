"""Reference for the CCSD one-particle density (nbed_amd/ccsd.py, nbed_amd/ccsd_gpu.py) that needs no second
implementation of the Lambda equations: for fixed orbitals and a fixed determinant the CCSD energy of h1 + x V obeys

    dE/dx at x = 0  =  sum_s tr(V_s dm1[s])

exactly, with dm1 the Lambda-based, orbital-unrelaxed response density.  The derivative is taken from energies of the
amplitude solver converged to 1e-13.  The five-point stencil (8 (E(h) - E(-h)) - (E(2h) - E(-2h))) / 12h at h = 1e-3
and h = 3e-3 agrees to 1e-13 .. 3e-11 on a synthetic Hamiltonian, but only to 6e-10 on the stiffer linear H4 used here
(its truncation error, h^4 E^(5) / 30, is 81 times larger at 3h), so the seven-point stencil

    (45 (E(h) - E(-h)) - 9 (E(2h) - E(-2h)) + (E(3h) - E(-3h))) / 60h,      error h^6 E^(7) / 140,

is used instead: its two step sizes agree to better than ``STENCIL_AGREEMENT`` = 1e-10 on every system below, which
leaves the tolerance of 1e-8 on the density two orders of margin over their difference.  That agreement is asserted,
and both values printed, wherever both step sizes are computed."""

import numpy as np

from nbed_amd import ccsd

TOL = 1e-8                 # |stencil - tr(V dm1)|
STENCIL_AGREEMENT = 1e-10  # |stencil(h) - stencil(3h)|: two orders below TOL
CONV = 1e-13
H4 = "4\n\nH 0 0 0\nH 0 0 0.9\nH 0 0 1.8\nH 0 0 2.7"  # linear, 0.9 A apart


def spin_blocks_to_spin_orbitals(v: np.ndarray) -> np.ndarray:
    """(2, n, n) -> (2n, 2n), alpha on the even indices."""
    n = v.shape[-1]
    out = np.zeros((2 * n, 2 * n))
    out[0::2, 0::2], out[1::2, 1::2] = v[0], v[1]
    return out


def stencil(const, h1, h2, occ, v, h=1e-3):
    """dE/dx of the CCSD energy of h1 + x v (v (2, n, n), symmetric per spin) at x = 0."""
    v_so = spin_blocks_to_spin_orbitals(np.asarray(v, dtype=float))
    e = {k: ccsd.solve(const, h1 + k * h * v_so, h2, occ, conv_tol=CONV).e_tot for k in (-3, -2, -1, 1, 2, 3)}
    return (45.0 * (e[1] - e[-1]) - 9.0 * (e[2] - e[-2]) + (e[3] - e[-3])) / (60.0 * h)


def stencil_checked(const, h1, h2, occ, v, label=""):
    """The stencil at h = 1e-3, after printing it next to h = 3e-3 and asserting that the two agree."""
    d1, d3 = stencil(const, h1, h2, occ, v, 1e-3), stencil(const, h1, h2, occ, v, 3e-3)
    print(f"{label}: stencil h=1e-3 {d1:.12f}  h=3e-3 {d3:.12f}  difference {abs(d1 - d3):.2e}")
    assert abs(d1 - d3) < STENCIL_AGREEMENT, (label, d1, d3)
    return d1


def unit_direction(n, s, p, q):
    """V = E_pq + E_qp in the spin block s: dE/dx = (2 - delta_pq) dm1[s, p, q] for a symmetric dm1."""
    v = np.zeros((2, n, n))
    v[s, p, q] += 1.0
    v[s, q, p] += 1.0
    if p == q:
        v[s, p, p] = 1.0
    return v


def random_direction(n, seed):
    """A seeded symmetric V, different in the two spin blocks, of Frobenius norm 1: the size of the single-element
    directions, so that one step size serves both."""
    v = np.random.default_rng(seed).standard_normal((2, n, n))
    v = 0.5 * (v + v.transpose(0, 2, 1))
    return v / np.linalg.norm(v)


def non_hf_term(n, occupied_spatial, seed=1234, size=0.05):
    """A fixed symmetric one-body term W (the same in both spin blocks), |W| about ``size``, that couples occupied and
    virtual orbitals and the orbitals of either set among themselves: with it f_ov != 0 and f_oo, f_vv are not
    diagonal, as after the concentric localisation."""
    w = np.random.default_rng(seed).uniform(-size, size, (n, n))
    w = 0.5 * (w + w.T)
    assert np.abs(w[:occupied_spatial, occupied_spatial:]).max() > size / 10
    return np.stack([w, w])
