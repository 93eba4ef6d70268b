"""nbx_mp2_pairs (csrc/mp2.hip) on every element, the device MP2 solver and the frozen natural orbitals on the GPU.

The kernel tests take the backend as the fixture ``be`` and use only ``asarray`` / ``to_host`` / ``mp2_pairs`` /
``mp2_pairs_tile`` of it, so tests/test_host_mp2_fno.py imports them and re-runs them on the host build of the kernel."""

import numpy as np
import pytest

import mp2_reference as ref
from test_gpu_ccsd import METHYL, WATER

from nbed_amd import NbedConfig, mp2
from nbed_amd.driver import BuiltinHFProvider, NbedDriver
from nbed_amd.ham_builder import HamiltonianBuilder

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
TL = 32  # the tile edge of csrc/mp2.hip (checked against nbx_mp2_pairs_tile below)
SAME_SHAPES = [(no, nv) for no in (1, 2, 3) for nv in (1, TL - 1, TL, TL + 1, 2 * TL + 1)]
OPPOSITE_SHAPES = [(1, 1, 1, 1), (3, TL + 1, 1, 2), (2, 5, 4, 2 * TL + 1)]


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


# ---------------------------------------------------------------- the kernel, every element
def exact_case(no1, nv1, no2, nv2, same, seed):
    """(V, eo1, ev1, eo2, ev2, t, terms): eigenvalues are multiples of 1/4 (occupied negative, virtual positive), so
    d = ((eo_i + eo_j) - ev_a) - ev_b is an exact multiple of 1/4 however it is associated; V = 4 q d with small integers
    q is integer-valued, and every quotient the kernel forms is the exact integer 4 q (same spin: 4 (q_iajb - q_ibja),
    d being symmetric under a <-> b there).  ``t`` is numpy's, in the kernel's layout [a, i, j, b]; ``terms`` the
    energy terms in longdouble."""
    rng = np.random.default_rng(seed)
    eo1 = -rng.integers(1, 40, no1) / 4.0
    ev1 = rng.integers(1, 40, nv1) / 4.0
    eo2, ev2 = (eo1, ev1) if same else (-rng.integers(1, 40, no2) / 4.0, rng.integers(1, 40, nv2) / 4.0)
    d = ((eo1[:, None, None, None] + eo2[None, None, :, None]) - ev1[None, :, None, None]) - ev2[None, None, None, :]
    q = rng.integers(-5, 6, (no1, nv1, no2, nv2)).astype(float)
    v = 4.0 * q * d
    assert np.array_equal(v, np.round(v)) and np.all(d < 0)
    g = v - v.transpose(0, 3, 2, 1) if same else v
    t = g / d
    assert np.array_equal(t, np.round(t))
    terms = np.asarray(t, dtype=np.longdouble) * np.asarray(g, dtype=np.longdouble) * (np.longdouble(0.25) if same else 1)
    return v, eo1, ev1, eo2, ev2, np.ascontiguousarray(t.transpose(1, 0, 2, 3)), terms


def run_pairs(be, v, eo1, ev1, eo2, ev2, same):
    poison = getattr(be, "_poison", None)
    if poison is not None:
        be._poison = True  # (what the kernel leaves untouched reads as NaN)
    try:
        t, e = be.mp2_pairs(be.asarray(v), be.asarray(eo1), be.asarray(ev1), be.asarray(eo2), be.asarray(ev2), same)
        return np.array(be.to_host(t)), float(np.array(be.to_host(e)).reshape(-1)[0])
    finally:
        if poison is not None:
            be._poison = poison


def check_case(be, no1, nv1, no2, nv2, same, seed):
    v, eo1, ev1, eo2, ev2, want, terms = exact_case(no1, nv1, no2, nv2, same, seed)
    got, energy = run_pairs(be, v, eo1, ev1, eo2, ev2, same)
    assert got.shape == (nv1, no1, no2, nv2)
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} elements untouched or NaN"
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), np.argwhere(got != want)[:5]
    if same:  # a == b: an exact zero
        assert not np.any(got[np.arange(nv1), :, :, np.arange(nv1)])
    bound = terms.size * EPS * float(np.sum(np.abs(terms)))
    assert abs(energy - float(np.sum(terms))) <= bound, (energy, float(np.sum(terms)), bound)
    again, energy2 = run_pairs(be, v, eo1, ev1, eo2, ev2, same)
    assert np.array_equal(again.view(np.int64), got.view(np.int64)) and np.float64(energy2).view(np.int64) == np.float64(energy).view(np.int64)


def test_tile_is_the_kernels(be):
    assert be.mp2_pairs_tile() == TL


@pytest.mark.parametrize("no,nv", SAME_SHAPES)
def test_same_spin_every_element(be, no, nv):
    """T bit for bit, a == b, the energy within count * eps * sum |terms| of the longdouble sum, two calls equal bits:
    one tile, a partial tile, the tile edge and its neighbours, and 2 Tl + 1 (three tiles a side: mirror pairs and
    diagonal tiles, more workgroups than one (i, j) pair has tiles)."""
    check_case(be, no, nv, no, nv, True, 100 * no + nv)


@pytest.mark.parametrize("shape", OPPOSITE_SHAPES)
def test_opposite_spin_every_element(be, shape):
    check_case(be, *shape, False, sum(shape))


def test_same_spin_slice_over_i(be):
    """no1 < no2: rows [1, 3) of a square block give those rows of T and their share of the energy."""
    no, nv = 4, TL + 3
    v, eo, ev, _, _, want, terms = exact_case(no, nv, no, nv, True, 9)
    got, energy = run_pairs(be, np.ascontiguousarray(v[1:3]), eo[1:3], ev, eo, ev, True)
    assert np.array_equal(got.view(np.int64), np.ascontiguousarray(want[:, 1:3]).view(np.int64))
    part = terms[1:3]
    assert abs(energy - float(np.sum(part))) <= part.size * EPS * float(np.sum(np.abs(part)))


def test_empty_block(be):
    """no2 = 0: energy 0, nothing to write."""
    for same, shape in ((False, (3, 4, 0, 5)), (False, (0, 4, 2, 5)), (True, (0, 4, 0, 4))):
        no1, nv1, no2, nv2 = shape
        got, energy = run_pairs(be, np.zeros(shape), np.zeros(no1), np.ones(nv1), np.zeros(no2), np.ones(nv2), same)
        assert got.shape == (nv1, no1, no2, nv2) and energy == 0.0


def test_bad_shapes_are_refused(be):
    v = be.asarray(np.zeros((2, 3, 2, 4)))
    e2, e3, e4 = be.asarray(-np.ones(2)), be.asarray(np.ones(3)), be.asarray(np.ones(4))
    with pytest.raises(ValueError):
        be.mp2_pairs(v, e2, e3, e2, e4, True)  # same spin needs nv1 == nv2
    with pytest.raises(ValueError):
        be.mp2_pairs(v, e2, e3, e2, e3, False)  # ev2 of the wrong length


# ---------------------------------------------------------------- the solver
def host_reference(obj, be):
    const, h1, h2 = HamiltonianBuilder(obj, obj.energy_nuc(), backend=be).build()
    return mp2.solve(const, h1, h2, ref.occupied_of(obj))


def assert_same_mp2(dev, host, tol=1e-11):
    for name in ("e_singles", "e_same", "e_opposite", "e_corr"):
        assert abs(getattr(dev, name) - getattr(host, name)) < tol, (name, getattr(dev, name), getattr(host, name))
    for s in (0, 1):
        assert dev.dvv[s].shape == host.dvv[s].shape
        assert np.max(np.abs(dev.dvv[s] - host.dvv[s]), initial=0.0) < tol, s


@pytest.fixture(scope="module")
def molecules(be):
    """H4 (closed shell) and the methyl radical in STO-3G, each on the tensor and on its Cholesky factor."""
    out = {}
    for name, geometry, spin in (("h4", ref.H4, 0), ("methyl", METHYL, 1)):
        cfg = NbedConfig(geometry=geometry, n_active_atoms=1, basis="sto-3g", xc_functional="hf", convergence=1e-11, spin=spin)
        out[name, "tensor"] = BuiltinHFProvider(be, eri_engine="host").global_hf(cfg)
        out[name, "factor"] = BuiltinHFProvider(be, eri_engine="cholesky", cholesky_tol=1e-10).global_hf(cfg)
    return out


@pytest.mark.parametrize("name", ["h4", "methyl"])
@pytest.mark.parametrize("route", ["tensor", "factor"])
def test_solve_scf_follows_the_host_solver(be, molecules, name, route):
    """Every energy part and every element of dvv to 1e-11 against ``mp2.solve`` on the Hamiltonian of the same
    object -- on the factor route that Hamiltonian is transformed from the same factor, so the Cholesky tolerance does
    not enter."""
    obj = molecules[name, route]
    assert (obj.eri_factor_device() is not None) == (route == "factor")
    dev = mp2.solve_scf(obj, backend=be)
    assert_same_mp2(dev, host_reference(obj, be))
    assert abs(dev.e_scf - obj.e_tot) < 1e-12 and dev.e_corr < -1e-3


@pytest.mark.parametrize("route", ["tensor", "factor"])
def test_solve_scf_non_canonical_and_sliced(be, molecules, route):
    """H4 after a rotation inside the occupied and the virtual space and a small occupied-virtual rotation (f_ov != 0,
    f_oo and f_vv not diagonal), and the same with a plan capacity of one byte: every spin pair is walked one i at a time."""
    obj, _ = ref.rotated(molecules["h4", route], 6, within=True, angle=0.05)
    host = host_reference(obj, be)
    assert abs(host.e_singles) > 1e-4
    assert_same_mp2(mp2.solve_scf(obj, backend=be), host)
    assert mp2.memory_plan(2, 2, None, 1)["rows"] == 1
    assert_same_mp2(mp2.solve_scf(obj, backend=be, capacity=1), host)
    radical, _ = ref.rotated(molecules["methyl", route], 7, within=True, angle=0.03)
    assert_same_mp2(mp2.solve_scf(radical, backend=be, capacity=1), host_reference(radical, be))


def check_restricted(be, obj):
    """A restricted object (one (ia|jb) block feeds the same-spin and the opposite-spin amplitudes) against the
    unrestricted object of the same closed-shell determinant: energies and dvv to 1e-11, unsliced and sliced; its
    truncated copy is restricted too."""
    r = ref.restricted_copy(obj, be)
    want = mp2.solve_scf(obj, backend=be)
    assert_same_mp2(mp2.solve_scf(r, backend=be), want)
    assert_same_mp2(mp2.solve_scf(r, backend=be, capacity=1), want)
    red, info = mp2.frozen_natural_orbitals(r, n_frozen_virt=1, backend=be)
    _, info_u = mp2.frozen_natural_orbitals(obj, n_frozen_virt=1, backend=be)
    n = np.asarray(r.mo_coeff).shape[1]
    assert np.asarray(red.mo_coeff).shape == (n, n - 1) and np.asarray(red.mo_occ).shape == (n - 1,)
    assert np.asarray(red.mo_energy).shape == (n - 1,) and np.array_equal(np.asarray(red.mo_occ)[:2], [2.0, 2.0])
    assert abs(info["e_correction"] - info_u["e_correction"]) < 1e-11 and info["n_kept"] == info_u["n_kept"]


@pytest.mark.parametrize("route", ["tensor", "factor"])
def test_restricted_object(be, molecules, route):
    check_restricted(be, molecules["h4", route])


# ---------------------------------------------------------------- end to end
def fno_end_to_end(be, provider, k=2, n_active_atoms=2):
    """nbed(config) on water / 6-31G with and without FNO; the by-order truncation of the full run's object by the
    same CCSD.  Returns (full result, FNO result, by-order e_ccsd)."""
    cfg = NbedConfig(geometry=WATER, n_active_atoms=n_active_atoms, basis="6-31g", xc_functional="b3lyp", convergence=1e-9,
                     projector="mu", max_hf_cycles=100, max_dft_cycles=100, run_ccsd_emb=True)
    full = NbedDriver(cfg, provider=provider, backend=be)
    full.embed()
    fno = NbedDriver(cfg, provider=provider, backend=be, fno_virtuals=k)
    fno.embed()
    reduced = HamiltonianBuilder(full.mu["scf"], 0.0, n_frozen_virt=k, backend=be)
    reduced.build_spatial_device()  # (leaves the by-order object in reduced.scf_method)
    by_order = full._run_emb_ccsd(reduced.scf_method)[0]
    return full, fno, by_order


def check_fno_end_to_end(full, fno, by_order, k):
    rf, rk = full.mu, fno.mu
    info = rk["fno"]
    occ = np.asarray(info["occupations"])
    assert info["n_kept"] == info["n_virtual"] - k and np.asarray(rk["scf"].mo_coeff).shape[-1] == np.asarray(rf["scf"].mo_coeff).shape[-1] - k
    assert np.all(occ >= -1e-12) and np.all(occ <= 1.0) and np.all(np.diff(occ, axis=-1) <= 1e-14)
    assert abs(info["e_correction"] - (info["e_mp2_full"] - info["e_mp2_kept"])) < 1e-14 and info["e_correction"] <= 1e-12
    e_full = rf["ccsd_emb"]
    err_fno = abs(rk["ccsd_emb"] + info["e_correction"] - e_full)
    err_order = abs((by_order.e_tot - full.e_nuc) - e_full)
    print(f"embedded water / 6-31G, k = {k}: |CCSD(FNO) + dE_FNO - CCSD| = {err_fno:.3e}, by order {err_order:.3e}, "
          f"FNO alone {abs(rk['ccsd_emb'] - e_full):.3e}, E(2) = {info['e_mp2_full']:.6f}")
    # the MP2 keys are composed as the CCSD keys are, and are those of the full virtual space
    assert abs(rk["e_mp2"] - rk["e_rhf"] - info["e_mp2_full"]) < 1e-10
    assert abs(rk["mp2_emb"] - rk["hf_emb"] - info["e_mp2_full"]) < 1e-10 and abs(rk["e_rhf"] - rf["e_rhf"]) < 1e-8
    assert err_fno < err_order


def test_nbed_with_fno_against_truncation_by_order(be):
    """``nbed(config)`` on water / 6-31G, two active atoms, mu projector, ``fno_virtuals=2``: result["fno"] is
    consistent, and |e_ccsd(FNO) + e_correction - e_ccsd(full)| is below the error of n_frozen_virt=2 by order, solved
    by the same CCSD.  (The same inequality holds on the CPU through the checker backend and the host solver:
    tests/test_host_mp2_fno.py.)"""
    provider = BuiltinHFProvider(be)
    full, fno, by_order = fno_end_to_end(be, provider, k=2)
    check_fno_end_to_end(full, fno, by_order, 2)
    check_mp2_switch_alone(be, provider, full, fno)


def check_mp2_switch_alone(be, provider, full, fno):
    """``mp2=True`` without FNO: the MP2 keys are set and composed as the CCSD keys are, nothing is truncated, and
    ``fno_virtuals=0`` is FNO off."""
    cfg = NbedConfig(geometry=WATER, n_active_atoms=2, basis="6-31g", xc_functional="b3lyp", convergence=1e-9,
                     projector="mu", max_hf_cycles=100, max_dft_cycles=100)
    drv = NbedDriver(cfg, provider=provider, backend=be, mp2=True, fno_virtuals=0)
    drv.embed()
    r = drv.mu
    e_corr = fno.mu["fno"]["e_mp2_full"]
    assert "fno" not in r and "e_mp2" not in full.mu and "mp2_emb" not in full.mu
    assert abs(r["e_mp2"] - r["e_rhf"] - e_corr) < 1e-9 and abs(r["mp2_emb"] - r["hf_emb"] - e_corr) < 1e-9
    assert abs(r["e_mp2"] - fno.mu["e_mp2"]) < 1e-8
    assert np.asarray(r["scf"].mo_coeff).shape == np.asarray(full.mu["scf"].mo_coeff).shape
    assert abs(r["hf_emb"] - full.mu["hf_emb"]) < 1e-8
    assert r["second_quantised"][1].shape == full.mu["second_quantised"][1].shape
