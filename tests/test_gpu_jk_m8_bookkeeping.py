"""The 8-fold packed J/K build (csrc/jk_m8.hip) with its range bookkeeping in host-made tables: every output bit as before.

At which tile a workgroup's range starts and in which row that tile lies are functions of (N, p0, np) alone;
jk_m8_kernel reads them from tables made on the host beside M8Ranges::first (M8Tables) instead of computing them in every
wave at every launch, and requests its first chunks before the Dtot' table.  No sum changes its order, so every case
is pinned to tests/golden/jk_m8_bits.json: one SHA-256 per case of the raw bytes of J and K (nbx_jk_packed on the
slab), and for the whole tensor with two densities of F and vhf too (nbx_jk_packed_fock, the entry point of the SCF
cycle: it takes two densities), recorded on the commit before the tables by
    NBX_LIB=<libnbx.so built from that commit> python tools/record_jk_m8_bits.py
(the tests of this file pass on that library too: that is what the hashes are).

Cases (N, p0, p1, ndm) -- the workgroup counts are m8_ranges' for these slabs:
  (100, 0, 100, 2)     the smallest instance, three LDS-DMA instructions per chunk
  (100, 0, 5, 2)       15 tiles, 15 workgroups
  (100, 3, 41, 1)      a slab that starts and ends inside a group of four rows
  (148, 0, 148, 2/1)   the benchmark's build, and with one density
  (148, 116, 148, 2), (148, 0, 67, 2)   the last and the first rows only
  (148, 75, 77, 2)     153 workgroups, 18 of them empty (their table entries are never read)
  (148, 131, 133, 2)   256 workgroups, 8 of them empty
The two slabs with empty workgroups are also added to the slabs before and behind them and their rows held to the C
oracle's whole-tensor J/K (oracle/c/jk_ref.c) at the tolerance of tests/test_gpu_bench_sizes.py."""

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import cref, synth

pytestmark = pytest.mark.gpu

GOLDEN_FILE = Path(__file__).resolve().parent / "golden" / "jk_m8_bits.json"

CASES = [
    (100, 0, 100, 2),
    (100, 0, 5, 2),
    (100, 3, 41, 1),
    (148, 0, 148, 2),
    (148, 0, 148, 1),
    (148, 116, 148, 2),
    (148, 0, 67, 2),
    (148, 75, 77, 2),
    (148, 131, 133, 2),
]
EMPTY_WG_CASES = [(148, 75, 77, 2), (148, 131, 133, 2)]
DM_STREAMS, HV_STREAMS = (532, 533), (570, 571)


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    yield HipBackend()
    _packed.clear()


@pytest.fixture(scope="module")
def gold():
    return json.loads(GOLDEN_FILE.read_text())


def key(case) -> str:
    return "jk_m8/n{}/p{}-{}/d{}".format(*case)


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def densities(n, ndm):
    return np.stack([synth.sym_matrix(s, n) for s in DM_STREAMS[:ndm]])


_packed = {}  # the packed slab last used (the two whole-tensor cases of N = 148 share theirs)


def packed_slab(be, n, p0, p1):
    if (n, p0, p1) not in _packed:
        _packed.clear()
        _packed[(n, p0, p1)] = be.eri_pack(be.synth_eri(n, p0, p1), n, p0, p1)
    return _packed[(n, p0, p1)]


def slab_jk(be, n, p0, p1, ndm):
    """(1 + ndm, N, N): the contributions of the slab's tiles to J and K, on the host."""
    return be.to_host(be.jk_packed(packed_slab(be, n, p0, p1), be.asarray(densities(n, ndm)), p0, p1))


def case_outputs(be, case):
    n, p0, p1, ndm = case
    assert be.lib.nbx_jk_packed_fold(n) == 8, "jk_m8.hip is the kernel under test"
    out = [slab_jk(be, n, p0, p1, ndm)]
    if (p0, p1, ndm) == (0, n, 2):
        hv = np.stack([synth.sym_matrix(s, n) for s in HV_STREAMS])
        fock, vhf = be.jk_packed_fock(packed_slab(be, n, p0, p1), be.asarray(densities(n, 2)), be.asarray(hv))
        out += [be.to_host(fock), be.to_host(vhf)]
    return out


def all_bits(be) -> dict:
    """Every hash of this file, in the order of CASES (tools/record_jk_m8_bits.py writes them out)."""
    return {key(case): sha(*case_outputs(be, case)) for case in CASES}


@pytest.mark.parametrize("case", CASES, ids=key)
def test_jk_m8_bits(be, gold, case):
    assert key(case) in gold, f"{key(case)}: no recorded hash (tools/record_jk_m8_bits.py)"
    out = case_outputs(be, case)
    assert all(np.all(np.isfinite(a)) for a in out)
    assert sha(*out) == gold[key(case)], f"{key(case)}: the bits differ from the recorded ones"


@pytest.mark.parametrize("case", EMPTY_WG_CASES, ids=key)
def test_slabs_with_empty_workgroups_add_up_to_the_oracle(be, case):
    """Slab + the slabs before and behind it = J and K of the whole tensor; the slab's own rows against oracle/c/jk_ref.c
    on those rows of the generated tensor (whose tiles are the slab's, so a partial of the slab that was dropped or read
    from an empty workgroup's unwritten storage shows here at full size)."""
    n, p0, p1, ndm = case
    total = slab_jk(be, n, 0, p0, ndm) + slab_jk(be, n, p0, p1, ndm) + slab_jk(be, n, p1, n, ndm)
    ref = cref.jk(cref.synth_eri(n, p0, p1), densities(n, ndm), p0, p1)  # (1 + ndm, rows, N)
    np.testing.assert_allclose(total[:, p0:p1], ref, rtol=0, atol=1e-11 * (n / 148) ** 2)
    np.testing.assert_array_equal(total[0], total[0].T)


def test_every_case_has_a_recorded_hash(gold):
    assert sorted(key(case) for case in CASES) == sorted(gold)
