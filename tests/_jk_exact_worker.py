"""The packed J/K runs of tests/test_gpu_jk_exact.py (imported by it), and -- run as a script -- the child process of
test_switch_selected_fallbacks_are_exact: the switches NBX_JK_M8 / NBX_JK_M4 / NBX_JK_MX are read once per process, so
the kernels they select (csrc/jk_m4.hip for 97 .. 148, csrc/jk_s4.hip for 97 .. 256) are run here,

    python tests/_jk_exact_worker.py "NBX_JK_M8=0 NBX_JK_M4=0"

with the named setting already in the environment, on the cases jk_cases.SWITCH_CASES keeps for it: every element of
J, K, F and vhf against the factorised references, bit for bit (tests/jk_cases.py says why that is the right
comparison).  The routing query is asked first: a case that no longer reaches the kernel it is there for fails."""

import gc
import os
import sys

import numpy as np

import jk_cases as jc


def fresh_backend():
    """A backend whose outputs and workspaces hold NaN before every call (what a kernel does not write reads as NaN)."""
    from nbed_amd.backend import HipBackend

    be = HipBackend()
    be._poison = True
    return be


def dev(be, x):
    """Host array -> device (a copy first: the operand caches are read-only)."""
    return be.asarray(np.array(x))


def free_device(be):
    import torch

    be.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


def check_symmetric(jk, what):
    jc.assert_exact(jk, jk.transpose(0, 2, 1), what + ": J and K symmetric")


def pack_whole(be, b_dev, n, slabs=None):
    """The packed tensor of the whole range.  slabs None: the dense tensor built, packed in one call and freed.
    Otherwise the dense rows are built a slab at a time and each slab is packed to its place in the tile sequence
    T(p, q) = p (p + 1) / 2 + q (include/nbx.h: the tiles follow each other; nbx_eri_packed_bytes is additive over slabs
    up to the constant it answers for an empty slab)."""
    lib = be.lib
    if slabs is None:
        eri = jc.device_rows(be.torch, b_dev, 0, n)
        packed = be.eri_pack(eri, n)
        del eri
        return packed
    slack = lib.nbx_eri_packed_bytes(n, 0, 0)
    total = lib.nbx_eri_packed_bytes(n, 0, n)
    packed = be.empty((total // 8,))
    for p0, p1 in slabs:
        off = lib.nbx_eri_packed_bytes(n, 0, p0) - slack
        assert off % 16 == 0 and off + lib.nbx_eri_packed_bytes(n, p0, p1) <= total
        assert lib.nbx_eri_packed_bytes(n, 0, p0) + lib.nbx_eri_packed_bytes(n, p0, n) - slack == total
        eri = jc.device_rows(be.torch, b_dev, p0, p1)
        be._call("nbx_eri_pack", n, p0, p1, be._p(eri), be._p(packed[off // 8:]))
        del eri
    return packed


def run_packed_case(be, case, ops=None, slabs_of=jc.equal_work_cuts, with_table=True, lds_nan=False, say=None):
    """Everything the exact test asks of one packed size: two densities, one density, the Fock epilogue with and without
    the Dtot' table of the scalars kernel, row slabs packed on their own (each against its slab reference, and their
    sum).  ops: the operands (default: the plain family).  Returns nothing; raises on the first difference."""
    n = case.n
    lib = be.lib
    got_route = jc.route(lib, n)
    assert got_route == (case.kernel, case.run_as), (case, got_route)
    ops = jc.operands(n) if ops is None else ops
    ref = jc.jk_reference(ops.b, ops.dm)
    ref1 = jc.jk_reference(ops.b, ops.dm[1])
    fock_ref, vhf_ref = jc.fock_reference(ops.b, ops.dm, ops.hv)
    tag = f"{jc.packed_id(case)}"
    free_device(be)
    b_dev, dm, hv = dev(be, ops.b), dev(be, ops.dm), dev(be, ops.hv)
    dm1 = dm[1].clone()  # (an allocation of its own, as a caller's single density is)
    big = n >= jc.SLAB_ONLY_FROM
    packed = pack_whole(be, b_dev, n, jc.dense_slabs(n) if big else None)
    if lds_nan:
        be.debug_fill_lds(float("nan"))
    got = be.to_host(be.jk_packed(packed, dm))
    jc.assert_exact(got, ref, tag + " two densities")
    check_symmetric(got, tag)
    if lds_nan:
        be.debug_fill_lds(float("nan"))
    got1 = be.to_host(be.jk_packed(packed, dm1))
    jc.assert_exact(got1, ref1, tag + " one density")
    check_symmetric(got1, tag + " one density")
    if lds_nan:
        be.debug_fill_lds(float("nan"))
    fock, vhf = be.jk_packed_fock(packed, dm, hv)
    jc.assert_exact(be.to_host(fock), fock_ref, tag + " fock")
    jc.assert_exact(be.to_host(vhf), vhf_ref, tag + " vhf")
    if with_table and lib.nbx_jk_dts_bytes(n) > 0:
        dts = be.jk_dts_new(n)
        zeros = be.zeros((2, n, n))
        be.huz_cycle_scalars_async(hv, None, zeros, zeros, dm, dm, dts=dts).get()
        fock, vhf = be.jk_packed_fock(packed, dm, hv, dts=dts)
        jc.assert_exact(be.to_host(fock), fock_ref, tag + " fock with the scalars kernel's table")
        jc.assert_exact(be.to_host(vhf), vhf_ref, tag + " vhf with the scalars kernel's table")
        del dts
    del packed
    # row slabs, each built and packed on its own
    conv = jc.packed_convention(case.kernel)
    acc, acc1 = np.zeros_like(ref), np.zeros_like(ref1)
    for p0, p1 in (jc.dense_slabs(n) if big else slabs_of(n)):
        eri = jc.device_rows(be.torch, b_dev, p0, p1)
        slab = be.eri_pack(eri, n, p0, p1)
        del eri
        part = be.to_host(be.jk_packed(slab, dm, p0, p1))
        jc.assert_exact(part, jc.slab_reference(ops.b, ops.dm, p0, p1, conv), f"{tag} slab [{p0}, {p1})")
        acc += part
        if big:  # (the slabs of the large sizes are expensive to build: the one-density call shares them)
            part1 = be.to_host(be.jk_packed(slab, dm1, p0, p1))
            jc.assert_exact(part1, jc.slab_reference(ops.b, ops.dm[1], p0, p1, conv), f"{tag} slab [{p0}, {p1}) one density")
            acc1 += part1
        del slab
    jc.assert_exact(acc, ref, tag + " sum of the slabs")
    if big:
        jc.assert_exact(acc1, ref1, tag + " sum of the slabs, one density")
    if say is not None:
        say(f"{tag}: exact ({case.why})")


def main(argv) -> int:
    setting = argv[1]
    for item in setting.split():
        name, value = item.split("=")
        assert os.environ.get(name) == value, f"{item} is not in the environment"
    be = fresh_backend()
    for case in jc.SWITCH_CASES[setting]:
        run_packed_case(be, case, say=print)
    print("JKX OK", setting)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
