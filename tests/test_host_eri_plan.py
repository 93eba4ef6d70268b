"""nbx_eri_plan: the host arithmetic behind the device integral engine (csrc/eri.hip) -- which canonical shell quartets
survive the Schwarz test, how they split into the 25 classes (la + lb, lc + ld), and the LDS and launch geometry of each
class's kernel -- against a recount in Python from the host engine's own tensor.  No GPU."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

from nbed_amd import _nbx, integrals

WATER_XYZ = "3\n\nO   0.0000  0.000  0.115\nH   0.0000  0.754  -0.459\nH   0.0000  -0.754  -0.459"
H2O2_XYZ = ("4\n\nO   0.000  0.734  -0.052\nO   0.000  -0.734  -0.052\nH   0.839  0.881  0.419\n"
            "H   -0.839  -0.881  0.419")
H2_FAR_XYZ = "2\n\nH 0 0 0\nH 0 0 12.0"
CUTOFF = 1e-16
LDS_PER_CU = 160 * 1024  # MI355X: 160 KiB per compute unit, all of which one workgroup may declare

CASES = {"water-631gs": (WATER_XYZ, "6-31g*", False), "water-631gs-cart": (WATER_XYZ, "6-31g*", True),
         "h2o2-631gs": (H2O2_XYZ, "6-31g*", False), "h2-12A-ccpvdz": (H2_FAR_XYZ, "cc-pvdz", False)}


def _plan_raw(nshell, ang, nprim, nfunc, centres, exps, coefs, sph, cutoff=CUTOFF):
    lib = _nbx.load_library()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    counts, grid = (ctypes.c_int64 * 25)(), (ctypes.c_int64 * 25)()
    lds, block = (ctypes.c_int * 25)(), (ctypes.c_int * 25)()
    rc = lib.nbx_eri_plan(nshell, ptr(ang), ptr(nprim), ptr(nfunc), ptr(centres), ptr(exps), ptr(coefs), ptr(sph),
                          float(cutoff), counts, lds, block, grid)
    as55 = lambda a: np.array(a[:]).reshape(5, 5)  # noqa: E731
    return rc, as55(counts), as55(lds), as55(block), as55(grid)


@lru_cache(maxsize=None)
def _case(name):
    xyz, basis, cart = CASES[name]
    bs = integrals.Basis(integrals.parse_geometry(xyz), basis, cart)
    rc, counts, lds, block, grid = _plan_raw(len(bs.shells), *integrals._shell_arrays(bs))
    assert rc == _nbx.NBX_OK
    return bs, counts, lds, block, grid


@lru_cache(maxsize=None)
def _recount(name):
    """The host engine's own test, from its tensor: Schwarz bound sqrt(max |(ab|ab)|) of every shell pair ia >= ib (from
    an unscreened run, so that the diagonal of a weak pair is there to be read; a pair whose primitives are all below
    cutoff * 1e-4 has a bound far below any product that passes), canonical pairs of pairs kl <= ij with
    bound(ij) * bound(kl) >= cutoff, grouped by (la + lb, lc + ld)."""
    bs = _case(name)[0]
    eri = integrals.two_electron_native(bs, nthreads=4, cutoff=0.0)
    n = bs.nao
    diag = np.abs(eri.reshape(n * n, n * n).diagonal()).reshape(n, n)
    off = np.concatenate([[0], np.cumsum([s.sph.shape[0] for s in bs.shells])])
    bound, order = [], []
    for ia in range(len(bs.shells)):
        for ib in range(ia + 1):
            bound.append(np.sqrt(diag[off[ia]:off[ia + 1], off[ib]:off[ib + 1]].max()))
            order.append(bs.shells[ia].ang + bs.shells[ib].ang)
    bound, order = np.array(bound), np.array(order)
    counts = np.zeros((5, 5), dtype=np.int64)
    for ij in range(len(bound)):
        ok = ~(bound[ij] * bound[:ij + 1] < CUTOFF) & (bound[:ij + 1] > 0) & (bound[ij] > 0)
        np.add.at(counts[order[ij]], order[:ij + 1][ok], 1)
    return counts, len(bound)


@pytest.mark.parametrize("name", sorted(CASES))
def test_quartet_counts_match_the_host_engines_own_test(name):
    counts = _case(name)[1]
    ref, npair = _recount(name)
    assert counts.sum() == ref.sum() and 0 < counts.sum() <= npair * (npair + 1) // 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_class_split_is_the_grouping_by_pair_orders(name):
    np.testing.assert_array_equal(_case(name)[1], _recount(name)[0])


def test_compact_molecules_reach_every_class():
    counts, npair = _case("water-631gs")[1], _recount("water-631gs")[1]
    assert counts.sum() == npair * (npair + 1) // 2  # nothing in water falls below 1e-16
    # one d shell: one (dd| pair, so (dd|dd) is that pair with itself, and (dp|dd) cannot be canonical
    assert counts[4, 4] == 1 and counts[3, 4] == 0
    # two d shells on different centres: all 25 classes, three (dd| pairs and their six canonical (dd|dd) quartets
    assert (_case("h2o2-631gs")[1] > 0).all() and _case("h2o2-631gs")[1][4, 4] == 6


def test_stretched_h2_screens_quartets_and_leaves_classes_empty():
    """s and p shells only, 12 A apart: no class with a pair order above 2 exists, and pairs of pairs across the gap fall
    below the cutoff -- the plan reports 0 for the former and launches nothing there."""
    bs, counts, _, _, grid = _case("h2-12A-ccpvdz")
    npair = len(bs.shells) * (len(bs.shells) + 1) // 2
    assert counts[3:].sum() == 0 and counts[:, 3:].sum() == 0
    assert 0 < counts.sum() < npair * (npair + 1) // 2
    assert (grid[counts == 0] == 0).all() and (grid[counts > 0] > 0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_lds_and_geometry_fit_the_compute_unit(name):
    _, counts, lds, block, grid = _case(name)
    assert (lds > 0).all() and (lds <= LDS_PER_CU).all()
    assert lds[4, 4] == lds.max() and lds[0, 0] == lds.min()
    # (dd|dd): two R cubes of edge 9 and w[36][35], the budget DESIGN.md section 12 works out
    assert 8 * (2 * 9 ** 3 + 36 * 35) <= lds[4, 4] <= 8 * (2 * 9 ** 3 + 36 * 35) + 2048
    assert (block == 64).all()
    assert (grid <= counts).all() and (grid <= 256 * (LDS_PER_CU // lds)).all()


def test_plan_refuses_what_the_device_engine_does_not_cover():
    one = np.ones(1)
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    args = lambda ang, nfunc: (1, i32(ang), i32(1), i32(nfunc), np.zeros(3), one, one, np.ones(100))  # noqa: E731
    assert _plan_raw(*args(3, 7))[0] == _nbx.NBX_E_INVALID   # f shells stay on the host engine
    assert _plan_raw(*args(4, 9))[0] == _nbx.NBX_E_INVALID
    assert _plan_raw(*args(2, 4))[0] == _nbx.NBX_E_INVALID   # a d shell has five or six functions
    rc, counts = _plan_raw(*args(0, 1))[:2]
    assert rc == _nbx.NBX_OK and counts[0, 0] == 1 and counts.sum() == 1
    lib = _nbx.load_library()
    assert lib.nbx_eri_plan(1, None, None, None, None, None, None, None, 1e-16, None, None, None, None) == _nbx.NBX_E_INVALID
