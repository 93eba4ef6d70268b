"""tests/eigh_cases.py on the host: every reference is certified, the groups are the intended ones, every group can be
judged (subspace bound below 1e-4), float64 LAPACK passes every bound with room to spare, and three mutations of a
correct result are caught.  tests/test_gpu_eigh.py holds the device's solvers to the same bounds."""

import numpy as np
import pytest

import eigh_cases as ec
import matfn_cases as mc

KEYS = ec.all_case_keys()
TABLE = sorted({(k[1], k[0]) for k in KEYS}, key=lambda t: (t[0], ec.SPECTRA.index(t[1])))
BOUNDS = ("eigenvalues", "residual", "orthonormality", "subspace")
LAPACK_MAX = 0.25
WORST = dict.fromkeys(BOUNDS, 0.0)


@pytest.mark.parametrize("n,name", TABLE, ids=[f"N{n}-{name}" for n, name in TABLE])
def test_every_case_is_certified_grouped_as_intended_and_passed_by_lapack(n, name):
    for key in (k for k in KEYS if k[1] == n and k[0] == name):
        _, _, index, mult = key
        c = ec.case(*key)
        # the certificate
        assert c.cert[0] <= mc.CERTIFICATE and c.cert[1] <= mc.CERTIFICATE * c.nrm, (c.ident(), c.cert)
        # the groups
        sizes = [b - a for a, b in c.groups]
        assert sum(sizes) == n and c.groups[0][0] == 0 and c.groups[-1][1] == n
        want = ec.expected_group_sizes(name, n, mult)
        if want is not None:
            assert sorted(s for s in sizes if s > 1) == want, (c.ident(), sizes)
        else:  # graded: the three shifted levels stand alone, the grid below is chained by GROUP nrm = 0.13
            assert sizes[-3:] == [1, 1, 1] and c.nrm == 1.3e6
            gaps = np.diff(c.lam0)
            inside = np.ones(n - 1, dtype=bool)
            inside[[a - 1 for a, _ in c.groups[1:]]] = False
            assert np.all(gaps[inside] < ec.GROUP * c.nrm) and np.all(gaps[~inside] >= ec.GROUP * c.nrm)
            if n <= 37:
                assert len(sizes) == n
        if name == "cluster" and n >= 24:
            m = ec.cluster_multiplicity(n) if mult is None else mult
            assert (n // 3, n // 3 + m) in c.groups and (2, 5) in c.groups
            assert np.all(c.lam0[n // 3:n // 3 + m] == c.lam0[n // 3])  # exactly degenerate as constructed
        if name == "pairs" and n >= 8:
            assert (n // 2, n // 2 + 2) in c.groups and (n - 2, n) in c.groups
            assert (n // 5, n // 5 + 1) in c.groups and (n // 5 + 1, n // 5 + 2) in c.groups
        # the condition
        assert max(c.subspace_bounds) < ec.SUBSPACE_MAX, (c.ident(), max(c.subspace_bounds))
        assert min(c.gamma) >= ec.GROUP * c.nrm * (1 - 1e-6)
        # LAPACK
        w, v = np.linalg.eigh(c.a)
        ratios = c.ratios(w, v)
        print(f"{c.ident()}: groups {len(sizes)} (largest {max(sizes)}), certificate {c.cert[0]:.1e} {c.cert[1] / c.nrm:.1e} nrm, "
              f"worst subspace bound {max(c.subspace_bounds):.1e}, LAPACK / bound "
              + " ".join(f"{k} {r:.2e}" for k, r in ratios.items()))
        for k, r in ratios.items():
            WORST[k] = max(WORST[k], r)
            assert r <= LAPACK_MAX, (c.ident(), k, r)
    print("LAPACK worst ratio per bound so far: " + " ".join(f"{k} {r:.2e}" for k, r in WORST.items()))


@pytest.mark.parametrize("n", [37, 198])
def test_mutations_of_a_correct_result_are_caught(n):
    c = ec.case("spread", n, 0)
    w, v = np.linalg.eigh(c.a)
    assert max(c.ratios(w, v).values()) <= LAPACK_MAX
    wide = [g for g, gamma in enumerate(c.gamma) if gamma >= 1e-2 * c.nrm]
    assert len(wide) >= 2
    i, j = c.groups[wide[0]][0], c.groups[wide[-1]][0]
    # a rotation by 1e-5 rad between two vectors of different, well separated groups
    t = 1.0e-5
    rot = v.copy()
    rot[:, i], rot[:, j] = np.cos(t) * v[:, i] - np.sin(t) * v[:, j], np.sin(t) * v[:, i] + np.cos(t) * v[:, j]
    r = c.ratios(w, rot)
    print(f"N={n} rotation: " + " ".join(f"{k} {x:.2e}" for k, x in r.items()))
    assert r["subspace"] > 1.0 and r["residual"] > 1.0
    assert r["orthonormality"] <= LAPACK_MAX  # (still orthonormal: only the subspaces and the residual see it)
    # an eigenvalue moved by 50 bounds
    moved = w.copy()
    moved[i] += 50.0 * c.bounds.eigenvalues
    r = c.ratios(moved, v)
    print(f"N={n} eigenvalue: " + " ".join(f"{k} {x:.2e}" for k, x in r.items()))
    assert 49.0 < r["eigenvalues"] < 51.0
    # a vector scaled by 1 + 1e-11
    scaled = v.copy()
    scaled[:, i] *= 1.0 + 1.0e-11
    r = c.ratios(w, scaled)
    print(f"N={n} scaling: " + " ".join(f"{k} {x:.2e}" for k, x in r.items()))
    assert r["orthonormality"] > 1.0
    # two neighbouring vectors exchanged (the wrong vector for the level): the subspaces see it
    swapped = v.copy()
    swapped[:, [i, i + 1]] = v[:, [i + 1, i]]
    assert c.ratios(w, swapped)["subspace"] > 1.0
    # NaN counts as a miss of every bound
    bad = v.copy()
    bad[0, 0] = np.nan
    assert all(x == float("inf") for x in c.ratios(w, bad).values())


def test_refine_grouped_with_singleton_groups_is_matfn_refine():
    c = ec.case("spread", 37, 0)
    assert all(b - a == 1 for a, b in c.groups)
    x, lam, s, cert = ec.refine_grouped(c.a, c.q, c.groups)
    x0, lam0, cert0 = mc.refine(c.a, c.q)
    np.testing.assert_array_equal(x, x0)
    np.testing.assert_array_equal(lam, lam0)
    assert cert == cert0
    np.testing.assert_array_equal(c.lam, lam0)  # no group above one: the Rayleigh quotients are the reference


def test_group_rule_leaves_the_basis_of_a_cluster_alone_and_certifies_its_subspace():
    """Inside a group E_ij = r_ij / 2: the refined vectors of the degenerate level span the invariant subspace of the
    ROUNDED matrix (cross-group S at the certificate) without diagonalising its O(eps) block, whose eigenvalues the
    reference takes from the block itself."""
    c = ec.case("cluster", 37, 0)
    lo, hi = 37 // 3, 37 // 3 + ec.cluster_multiplicity(37)
    blk = np.asarray(c.s[lo:hi, lo:hi], dtype=np.float64)
    spread = np.max(np.abs(blk - np.mean(np.diag(blk)) * np.eye(hi - lo)))
    assert spread <= 37 * mc.EPS * c.nrm
    assert np.all(np.diff(c.lam[lo:hi]) >= 0) and float(c.lam[hi - 1] - c.lam[lo]) <= 2 * 37 * mc.EPS * c.nrm
    # LAPACK's eigenvalues inside the cluster agree with the block's to rounding
    w = np.linalg.eigvalsh(c.a)
    assert mc.worst_ratio(w[lo:hi], c.lam[lo:hi], c.bounds.eigenvalues) <= LAPACK_MAX


def test_float64_operands_and_their_judge():
    """The operands of the three largest instances: the constructed levels are their spectrum to rounding, and LAPACK's
    eigenpairs pass the float64 bounds."""
    for name in ec.FLOAT64_SPECTRA:
        a, lam = ec.float64_operand(name, 513, 0)
        assert np.array_equal(a, a.T)
        w, v = np.linalg.eigh(a)
        nrm = float(np.max(np.abs(lam)))
        assert np.max(np.abs(w - lam)) <= 513 * mc.EPS * nrm
        r = ec.float64_ratios(a, w, v)
        print(f"{name} N=513 LAPACK / float64 bound: " + " ".join(f"{k} {x:.2e}" for k, x in r.items()))
        assert max(r.values()) <= LAPACK_MAX
        w2 = w.copy()
        w2[100] += 50.0 * (ec.ACCEPT + 2 * 513 * mc.EPS) * nrm
        assert ec.float64_ratios(a, w2, v)["eigenvalues"] > 49.0
