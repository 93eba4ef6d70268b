"""huzinaga_fused_kernel of the settled SCF cycle at the sizes where a trip of loads or a wave's role changes, and the
post-Fock chain it runs in.

The kernel is a workgroup of two wavefronts -- wave 0 forms T1 = F[I,:] DS[:,J], wave 1 T2 = F[J,:] DS[:,I], on a
diagonal tile wave 1 only keeps the barriers -- and requests the operands of 160 k in one trip to memory
(csrc/elementwise.hip).  Which wave forms a product and how its loads are batched must not change one bit of any result,
so besides the exact and structural checks every case is pinned to tests/golden/settled_trips_bits.json: one SHA-256
of the raw output bytes per case, recorded by tools/record_settled_bits.py on the kernel as it was before (one
wavefront, both chains, trips of 80 k: the same sequence of floating-point operations per accumulator).

Inputs come from the deterministic generators of scf_kernel_cases."""

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import scf_kernel_cases as sk

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

GOLDEN_FILE = Path(__file__).resolve().parent / "golden" / "settled_trips_bits.json"

# 15 / 16 / 17: one tile, its edge, a second (off-diagonal tiles: wave 1 works); 159 / 160 / 161: one trip, the next
HUZ_NS = [1, 15, 16, 17, 148, 159, 160, 161, 176, 321]
HUZ_KAPPA = 0.75
CHAIN_CASES = [(16, (3, 2)), (148, (40, 39))]


@pytest.fixture(scope="module")
def be():
    from nbed_amd.backend import HipBackend

    return HipBackend()


@pytest.fixture(scope="module")
def gold():
    return json.loads(GOLDEN_FILE.read_text())


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def check_bits(gold, bits: dict):
    assert bits, "no case ran"
    for key, value in bits.items():
        assert key in gold, f"{key}: no recorded hash (tools/record_settled_bits.py)"
        assert value == gold[key], f"{key}: the bits differ from the recorded ones"


# ------------------------------------------------------------------------------------------ huzinaga_fused_kernel
def huz_run(be, kind, N, batch, kappa):
    f3, ds3 = sk.huz_operands(kind, N, batch)
    f, ds = (f3[0], ds3[0]) if batch == 1 else (f3, ds3)  # batch 1 is the 2-D form
    hz_d, fo_d = be.huzinaga_fused(be.asarray(f), be.asarray(ds), kappa, want_fock=True)
    return f, ds, be.to_host(hz_d), be.to_host(fo_d)


def huz_bits(be, N, batch, run=None):
    _, _, hz, fo = run or huz_run(be, "real", N, batch, HUZ_KAPPA)
    return {f"huzinaga_fused/n{N}/b{batch}": sha(hz, fo)}


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("N", HUZ_NS)
def test_huzinaga_fused_trips(be, gold, N, batch):
    real = huz_run(be, "real", N, batch, HUZ_KAPPA)
    check_bits(gold, huz_bits(be, N, batch, real))
    for kappa in (1.0, 0.5):  # integer operands: the reference itself is exact
        f, ds, hz, fo = huz_run(be, "exact", N, batch, kappa)
        hz_ref, fo_ref, _, _ = sk.huz_fused_reference(f, ds, kappa)
        for got, ref in ((hz, hz_ref), (fo, fo_ref)):
            ref64 = np.asarray(ref, dtype=np.float64)
            assert np.all(ref == ref64.astype(sk.LD))
            np.testing.assert_array_equal(got, ref64)
    f, _, hz, fo = real
    np.testing.assert_array_equal(hz, np.swapaxes(hz, -1, -2))  # symmetric to the bit
    np.testing.assert_array_equal(fo, f + hz)  # one rounded addition per element


# ------------------------------------------------------------------------------------------ the chain as a whole
def chain_run(be, N, nocc):
    """nbx_huz_cycle_post on a chosen J/K, cold (guarded) and then tracked from the cold cycle's orbitals."""
    hv, jk, ds, dm_in, s, x = sk.chain_operands(N)
    dts = be.jk_dts_new(N) if N in sk.DTS_SIZES[:2] else None
    h = be.huz_cycle_state(N, nocc, None, be.asarray(hv), be.asarray(ds), be.asarray(np.stack([s, s])), be.asarray(x), dts,
                           eri=None, p0=0, p1=0)
    jk_d, dm_in_d = be.asarray(jk), be.asarray(dm_in)

    def cycle(c_in, out, mode):
        pend = be.huz_cycle(h, dm_in_d, c_in, out, mode, 6, 0, 0, 1, False, reduce=lambda t: t.copy_(jk_d))
        return pend.get()

    cold, out = h.sets[0], h.sets[1]
    results = {}
    for name, c_in, res, mode in (("cold", None, cold, 0), ("tracked", cold["c"], out, 1)):
        scal = cycle(c_in, res, mode)
        be.synchronize()
        results[name] = [be.to_host(h.fock2)] + [be.to_host(res[k]) for k in ("hz", "c", "w", "dm")] + [np.asarray(scal)]
    return results


def chain_bits(be, N, nocc, run=None):
    return {f"huz_cycle_post/n{N}/{name}": sha(*arrays) for name, arrays in (run or chain_run(be, N, nocc)).items()}


@pytest.mark.parametrize("N,nocc", CHAIN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_post_fock_chain_trips(be, gold, N, nocc):
    run = chain_run(be, N, nocc)
    check_bits(gold, chain_bits(be, N, nocc, run))
    for arrays in run.values():
        assert all(np.all(np.isfinite(a)) for a in arrays)


def all_bits(be) -> dict:
    """Every hash of this file, in the order of the tests (tools/record_settled_bits.py writes them out)."""
    bits = {}
    for N in HUZ_NS:
        for batch in (1, 2):
            bits.update(huz_bits(be, N, batch))
    for N, nocc in CHAIN_CASES:
        bits.update(chain_bits(be, N, nocc))
    return bits


def test_every_case_has_a_recorded_hash(gold):
    """Nothing is skipped and nothing stale is kept: the recorded keys are exactly the cases of this file."""
    keys = [f"huzinaga_fused/n{N}/b{b}" for N in HUZ_NS for b in (1, 2)]
    keys += [f"huz_cycle_post/n{N}/{name}" for N, _ in CHAIN_CASES for name in ("cold", "tracked")]
    assert sorted(keys) == sorted(gold)
