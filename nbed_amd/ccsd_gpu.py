"""Spin-orbital CCSD on the device: the equations of ``nbed_amd.ccsd`` with every contraction an ``nbx_gemm``.

The reference runs PySCF's ``cc.CCSD`` on the embedded SCF object (nbed/driver.py:1105-1135).  ``nbed_amd.ccsd`` solves
the same amplitude equations (Stanton, Gauss, Watts, Bartlett, J. Chem. Phys. 94, 4334 (1991), general Fock matrix) with
dense numpy einsum on the host, for up to 40 spin orbitals.  This module is that solver on the MI355X:

* the antisymmetrised blocks <pq||rs> are cut straight out of the three SPATIAL spin blocks of
  ``HamiltonianBuilder.build_spatial()`` (``nbx_ccsd_gather``); the (2n)^4 tensor exists nowhere;
* every term is a permute -> ``gemm`` -> permute (``Contractor``), the permutes one kernel (``nbx_permute4``) that also
  does the P(ij), P(ab) antisymmetrisations of the doubles residual;
* the particle-particle ladder 1/2 sum_ef tau_ijef <ab||ef> -- the only O(o^2 v^4) term -- runs over packed pairs
  i < j, a < b, e < f, and W_abef is never formed: its t1 <ov||vv> pieces go through an o^3 v intermediate and its
  1/4 tau <oo||vv> piece through W_mnij;
* MP2 start, amplitude DIIS (space 6, from the second stored vector) and the convergence rule are those of
  ``ccsd.solve``, so the iterates follow the host solver's and can be compared cycle by cycle;
* ``triples=True``: after the loop the (T) energy of ``ccsd.triples_correction`` from the device-resident amplitudes and
  blocks (``triples_from_blocks``): semicanonical rotation, one v x v^2 cube per occupied triple from six ``nbx_gemm``
  calls, antisymmetriser, denominators and energy sum in ``nbx_ccsd_triples_energy`` (csrc/ccsd_t.hip);
* ``density=True``: after the loop the Lambda equations of ``ccsd.solve_lambda`` on the same device-resident blocks and
  amplitudes (``lambda_from_blocks``: the same ``Contractor``, the same packed ladder against ``vvvv_p``, the same
  update kernel and DIIS, in the amplitude loop's own history buffers) and the one-particle density of
  ``CCSDResult.rdm1`` (``nbx_ccsd_lambda_outer``, ``nbx_ccsd_rdm1``: csrc/ccsd_lambda.hip).

``torch`` only allocates and views; per cycle three groups of scalars reach the host (energy, max |err|, DIIS dots).
"""

from __future__ import annotations

import itertools
import time

import numpy as np

from .ccsd import CCSDResult
from .exceptions import NbedDriverError

# the nine blocks of <pq||rs> the equations read ('o' occupied, 'v' virtual) ...
BLOCKS = ("oovv", "oooo", "ovvo", "ovov", "ooov", "ovvv", "vvvo", "ovoo")
# ... and <vv||vv>, held over packed pairs (a < b, e < f) only


def _npair(n: int) -> int:
    return n * (n - 1) // 2


def block_sizes(no: int, nv: int) -> dict:
    """Doubles of every Hamiltonian block the solver keeps on the device for ``no`` occupied and ``nv`` virtual
    spin orbitals (``vvvv`` over packed pairs)."""
    ext = {"o": no, "v": nv}
    sizes = {name: int(np.prod([ext[c] for c in name], dtype=object)) for name in BLOCKS}
    sizes["vvvv"] = _npair(nv) ** 2
    return sizes


def memory_plan(no: int, nv: int, diis_space: int = 6, density: bool = False) -> dict:
    """Bytes the device solver needs, by group, computed before anything is allocated (host arithmetic):

    blocks     the nine Hamiltonian blocks of ``block_sizes``
    spatial    the (3, n, n, n, n) spatial spin blocks they are gathered from (2n = no + nv)
    amplitudes [t1 | t2] and the residual of the same layout, the DIIS history (2 x space vectors), tau, tau~ and
               the packed tau
    work       the largest set of intermediates and permute buffers alive at once: W_mbej, the 1/2 t2 + t1 t1 of
               its last term, three o^2 v^2 temporaries, two <ov||vv>-sized permute buffers, the packed ladder
               result and its half-unpacked form
    lambda     only with ``density``: what the Lambda loop holds beyond the above -- it reuses the residual, the DIIS
               history and, for its per-cycle temporaries, the work space of the amplitude loop: [l1 | l2], the
               packed l2, W_abei and W_maef with one more <ov||vv>-sized buffer while they are built, W_mbij and
               W_mnie, W_mbej and the ladder L, W_mnij
    """
    n = (no + nv + 1) // 2
    nvec = no * nv + (no * nv) ** 2
    o2v2 = (no * nv) ** 2
    ovvv = no * nv**3
    plan = {
        "blocks": 8 * sum(block_sizes(no, nv).values()),
        "spatial": 8 * 3 * n**4,
        "amplitudes": 8 * (2 * nvec + 2 * diis_space * nvec + 2 * o2v2 + _npair(no) * _npair(nv)),
        "work": 8 * (5 * o2v2 + 2 * ovvv + _npair(no) * _npair(nv) + _npair(no) * nv * nv + no**3 * nv + no**4),
    }
    if density:
        plan["lambda"] = 8 * (nvec + _npair(no) * _npair(nv) + 3 * ovvv + 2 * no**3 * nv + 2 * o2v2 + no**4)
    plan["total"] = sum(plan.values())
    return plan


TRIPLES_TILE = (16, 4, 16)  # cube tile (a, b, c) of nbx_ccsd_triples_energy (csrc/ccsd_t.hip)


def _ntriple(n: int) -> int:
    return n * (n - 1) * (n - 2) // 6


def triples_memory_plan(no: int, nv: int, batch: int) -> dict:
    """Bytes the (T) step needs on top of the blocks and amplitudes the CCSD loop leaves on the device, by group (host
    arithmetic; ``memory_plan`` is the loop's own and does not know about it):

    rotated    the semicanonical t1, f_ov, t2, <oo||vv>, <ov||vv>, <ov||oo>, the (j, k, m, a) copy of the last one the
               hole term reads, and the list of triples
    work       the rotation of <ov||vv>, the largest: its input is one of the loop's blocks, so two intermediates of
               its size and the result of a permuted product on top of what ``rotated`` already counts
    cubes      ``batch`` cubes of nv^3 doubles
    partials   one double per workgroup of the energy kernel and per cube, and the per-batch energies
    """
    if batch < 1:
        raise ValueError("triples_batch must be at least 1")
    ta, tb, tc = TRIPLES_TILE
    tiles = -(-nv // ta) * -(-nv // tb) * -(-nv // tc)
    ntri = _ntriple(no)
    plan = {
        "rotated": 8 * (2 * no * nv + 2 * (no * nv) ** 2 + no * nv**3 + 2 * no**3 * nv) + 4 * 3 * ntri,
        "work": 8 * 3 * no * nv**3,
        "cubes": 8 * batch * nv**3,
        "partials": 8 * (batch * tiles + max(ntri, 1)),  # (a slot per triple: room for any batch, so linear in it)
    }
    plan["total"] = sum(plan.values())
    return plan


def default_triples_batch(no: int, nv: int, free: int) -> int:
    """Cubes in flight when the caller names none: as many as fit into half of the ``free`` bytes the fixed groups of
    ``triples_memory_plan`` leave, at most 64 (past that a batch is GEMM work for every CU many times over) and at most
    the number of triples; at least 1 -- whether one fits is for the caller to check."""
    one, two = triples_memory_plan(no, nv, 1), triples_memory_plan(no, nv, 2)
    per_cube = two["total"] - one["total"]
    room = (free - (one["total"] - per_cube)) // 2
    return int(max(1, min(64, _ntriple(no), room // max(per_cube, 1))))


class Contractor:
    """``out = alpha * einsum(spec, a, b) + beta * out`` for two operands of up to four axes as permute -> gemm -> permute.

    Of the ways to lay the operands out as matrices -- free and contracted axes in the order of either operand or of the
    result, either operand first -- the one that moves the fewest doubles through ``permute4`` is taken; an operand that
    already is (free, contracted) or (contracted, free) is passed to the GEMM as it is, with 'N' or 'T'."""

    def __init__(self, be):
        self.be = be

    @staticmethod
    def _layout(letters, free, contr):
        """('N' | 'T' | None) for an operand with axes ``letters`` used as a (free x contr) matrix."""
        if list(letters) == free + contr:
            return "N"
        if list(letters) == contr + free:
            return "T"
        return None

    def __call__(self, spec, a, b, alpha=1.0, out=None, beta=0.0):
        be = self.be
        ins, lo = spec.split("->")
        la, lb = ins.split(",")
        ext = {}
        for letters, t in ((la, a), (lb, b)):
            if len(letters) != t.dim():
                raise ValueError(f"{spec}: operand of {t.dim()} axes")
            for c, s in zip(letters, t.shape):
                if ext.setdefault(c, int(s)) != int(s):
                    raise ValueError(f"{spec}: extent of {c}")
        contr_set = [c for c in la if c in lb and c not in lo]
        if sorted(lo) != sorted(c for c in la + lb if c not in contr_set) or not contr_set:
            raise ValueError(f"{spec}: not a two-operand contraction")
        shape_out = tuple(ext[c] for c in lo)
        if out is None:
            if beta != 0.0:
                raise ValueError("beta != 0 needs out")
            out = be.empty(shape_out)
        best = None
        for swap in (False, True):
            (l1, t1), (l2, t2) = ((lb, b), (la, a)) if swap else ((la, a), (lb, b))
            f1_opts = {tuple(c for c in l1 if c in lo), tuple(c for c in lo if c in l1)}
            f2_opts = {tuple(c for c in l2 if c in lo), tuple(c for c in lo if c in l2)}
            k_opts = {tuple(c for c in l1 if c in contr_set), tuple(c for c in l2 if c in contr_set)}
            for f1, f2, k in itertools.product(sorted(f1_opts), sorted(f2_opts), sorted(k_opts)):
                f1, f2, k = list(f1), list(f2), list(k)
                lay1, lay2 = self._layout(l1, f1, k), self._layout(l2, f2, k)
                direct = f1 + f2 == list(lo)
                cost = ((0 if lay1 else t1.numel()) + (0 if lay2 else t2.numel()) + (0 if direct else 2 * out.numel()))
                if best is None or cost < best[0]:
                    best = (cost, l1, t1, l2, t2, f1, f2, k, lay1, lay2, direct)
        _, l1, t1, l2, t2, f1, f2, k, lay1, lay2, direct = best
        m = int(np.prod([ext[c] for c in f1], dtype=np.int64))
        n = int(np.prod([ext[c] for c in f2], dtype=np.int64))
        kk = int(np.prod([ext[c] for c in k], dtype=np.int64))
        if lay1 is None:
            t1, lay1 = be.permute4(t1, [l1.index(c) for c in f1 + k]), "N"
        if lay2 is None:
            t2, lay2 = be.permute4(t2, [l2.index(c) for c in f2 + k]), "N"
        ta = lay1  # (m x k) stored as is: 'N'; stored (k x m): 'T'
        tb = "T" if lay2 == "N" else "N"  # the second operand enters the product as (k x n)
        lda = kk if ta == "N" else m
        ldb = kk if lay2 == "N" else n
        if direct:
            be.gemm_raw(ta, tb, m, n, kk, alpha, t1, lda, 0, t2, ldb, 0, beta, out, n, 0, 1)
            return out
        tmp = be.empty((m, n))
        be.gemm_raw(ta, tb, m, n, kk, 1.0, t1, lda, 0, t2, ldb, 0, 0.0, tmp, n, 0, 1)
        order = f1 + f2
        be.permute4(tmp.view(tuple(ext[c] for c in order)), [order.index(c) for c in lo], alpha, beta, out)
        return out


def spatial_from_dense(h1: np.ndarray, h2: np.ndarray):
    """(one_body (2,n,n), two_body (3,n,n,n,n)) of a dense spin-orbital Hamiltonian in the form ``build()`` returns
    (alpha on the even indices; aaaa, bbbb, abba and baab the only non-zero spin blocks, baab the transpose of abba)."""
    h1, h2 = np.asarray(h1, dtype=float), np.asarray(h2, dtype=float)
    nso = h1.shape[0]
    if nso % 2 or h1.shape != (nso, nso) or h2.shape != (nso,) * 4:
        raise ValueError("solve() takes the (2n, 2n) / (2n)^4 spin-orbital tensors of HamiltonianBuilder.build()")
    one = np.stack([h1[0::2, 0::2], h1[1::2, 1::2]])
    two = np.stack([h2[0::2, 0::2, 0::2, 0::2], h2[1::2, 1::2, 1::2, 1::2], h2[0::2, 1::2, 1::2, 0::2]])
    ok = not h1[0::2, 1::2].any() and not h1[1::2, 0::2].any()
    ok = ok and np.array_equal(h2[1::2, 0::2, 0::2, 1::2], two[2].transpose(1, 0, 3, 2))
    ok = ok and np.count_nonzero(h2) == sum(np.count_nonzero(x) for x in two) + np.count_nonzero(two[2])
    if not ok:
        raise ValueError("the dense Hamiltonian is not of the spin-block form HamiltonianBuilder.build() produces")
    return np.ascontiguousarray(one), np.ascontiguousarray(two)


def solve(constant, h1, h2, occupied, conv_tol: float = 1e-10, max_cycle: int = 200, diis_space: int = 6,
          backend=None, triples: bool = False, triples_batch: int | None = None, density: bool = False,
          stats: dict | None = None) -> CCSDResult:
    """``ccsd.solve`` on the device, from the dense spin-orbital tensors of ``build()`` (direct use and tests; the driver
    calls ``solve_spatial``, which never holds a (2n)^4 tensor)."""
    one, two = spatial_from_dense(h1, h2)
    return solve_spatial((constant, one, two), occupied, conv_tol=conv_tol, max_cycle=max_cycle, diis_space=diis_space,
                         backend=backend, triples=triples, triples_batch=triples_batch, density=density, stats=stats)


def _device_backend(backend):
    if backend is None:
        from .backend import get_backend

        backend = get_backend()
    if not hasattr(backend, "ccsd_gather"):
        raise NbedDriverError(f"the device CCSD needs a HipBackend (got {type(backend).__name__})")
    return backend


def _rotate4(c, x, us):
    """x[w,x,y,z] -> sum x[a,b,c,d] u0[a,w] u1[b,x] u2[c,y] u3[d,z], one axis per product."""
    x = c("ap,abcd->pbcd", us[0], x)
    x = c("abcd,bq->aqcd", x, us[1])
    x = c("abcd,cr->abrd", x, us[2])
    return c("abcd,ds->abcs", x, us[3])


def triples_from_blocks(t1, t2, fov, foo, fvv, oovv, ovvv, ovoo, occ_spins, vir_spins, batch: int | None = None,
                        backend=None, stats: dict | None = None) -> float:
    """The (T) energy of ``ccsd.triples_correction`` on the device, from the amplitudes, the Fock blocks and the three
    Hamiltonian blocks it reads (device tensors as the CCSD loop leaves them, or host arrays) in any orbital basis whose
    spin orbitals have the spins ``occ_spins`` / ``vir_spins`` (0 alpha, 1 beta).

    f_oo and f_vv are diagonalised on the host, one eigenproblem per spin (``ccsd.spin_block_eigh``: alpha never mixes
    with beta); the operands are always rotated, on the device, through ``Contractor``.  For every occupied triple
    i < j < k six batched ``nbx_gemm`` calls accumulate the cube W[a,(bc)] -- particle and hole term of (i|jk), (j|ik),
    (k|ji) -- and ``nbx_ccsd_triples_energy`` reduces ``batch`` cubes at a time.  The per-batch energies are added on the
    host in batch order, so one (o, v, batch) always gives the same bits."""
    from .ccsd import spin_block_eigh

    be = _device_backend(backend)
    foo_h, fvv_h = np.asarray(be.to_host(foo), dtype=float), np.asarray(be.to_host(fvv), dtype=float)
    no, nv = int(foo_h.shape[0]), int(fvv_h.shape[0])
    if stats is not None:
        stats.update(triples=_ntriple(no), triples_batch=0, triples_seconds=0.0)
    if no < 3 or nv < 3:
        return 0.0  # no triple excitation: nothing is launched
    ntri = _ntriple(no)
    free = be.free_bytes()
    plan = triples_memory_plan(no, nv, 1)
    if plan["total"] > free:
        raise NbedDriverError(
            f"the (T) step of {no} occupied and {nv} virtual spin orbitals needs {plan['total']} bytes of device memory "
            f"with one cube in flight ({plan['rotated']} for the semicanonical operands, {plan['work']} to rotate them, "
            f"{plan['cubes']} per cube, {plan['partials']} of partial sums); {free} are free")
    if batch is None:
        batch = default_triples_batch(no, nv, free)
    batch = int(batch)
    if batch < 1:
        raise ValueError("triples_batch must be at least 1")
    batch = min(batch, ntri, 65535)
    plan = triples_memory_plan(no, nv, batch)
    if plan["total"] > free:
        raise NbedDriverError(f"the (T) step with {batch} cubes in flight needs {plan['total']} bytes of device memory "
                              f"({plan['cubes']} for the cubes); {free} are free")
    t_start = time.perf_counter()
    c = Contractor(be)
    eo_h, uo_h = spin_block_eigh(foo_h, occ_spins)
    ev_h, uv_h = spin_block_eigh(fvv_h, vir_spins)
    eo, ev, uo, uv = be.asarray(eo_h), be.asarray(ev_h), be.asarray(uo_h), be.asarray(uv_h)
    t1s = c("pa,aq->pq", c("ip,ia->pa", uo, be.asarray(t1)), uv)
    fovs = c("pa,aq->pq", c("ip,ia->pa", uo, be.asarray(fov)), uv)
    t2s = _rotate4(c, be.asarray(t2), (uo, uo, uv, uv))
    oovvs = _rotate4(c, be.asarray(oovv), (uo, uo, uv, uv))
    ovvvs = _rotate4(c, be.asarray(ovvv), (uo, uv, uv, uv))
    ovoo_jkma = be.permute4(_rotate4(c, be.asarray(ovoo), (uo, uv, uo, uo)), [2, 3, 0, 1])
    triples = [(i, j, k) for i in range(no) for j in range(i + 1, no) for k in range(j + 1, no)]
    ijk = be.int_array(np.array(triples, dtype=np.int32).reshape(-1, 3))
    v2, v3, ov = nv * nv, nv**3, no * nv
    cubes = be.empty((batch, nv, v2))
    work = be.empty(max(be.ccsd_triples_work_doubles(nv, batch), 1))
    nbatch = -(-ntri // batch)
    energies = be.empty(nbatch)
    t2f, ovvvf, ovoof, cubesf = t2s.view(-1), ovvvs.view(-1), ovoo_jkma.view(-1), cubes.view(-1)

    def product(trans_a, kk, alpha, a, a_off, sa, b, b_off, sb, beta, slot, count):
        be.gemm_raw(trans_a, "N", nv, v2, kk, alpha, a[a_off:], nv, sa, b[b_off:], v2, sb, beta, cubesf[slot * v3:], v2, v3,
                    count)

    for x in range(nbatch):
        t0 = x * batch
        nb = min(batch, ntri - t0)
        s = 0
        while s < nb:  # runs of triples that share (i, j): k = k0, k0 + 1, ... ride on the GEMM's batch strides
            i, j, k0 = triples[t0 + s]
            n = min(no - k0, nb - s)
            # (i|jk): - sum_e t2[j,k,a,e] ovvv[i,e,(bc)] - sum_m ovoo[m,a,j,k] t2[i,m,(bc)]   (beta = 0: writes the cube)
            product("N", nv, -1.0, t2f, (j * no + k0) * v2, v2, ovvvf, i * v3, 0, 0.0, s, n)
            product("T", no, -1.0, ovoof, (j * no + k0) * ov, ov, t2f, i * no * v2, 0, 1.0, s, n)
            # -(j|ik)
            product("N", nv, 1.0, t2f, (i * no + k0) * v2, v2, ovvvf, j * v3, 0, 1.0, s, n)
            product("T", no, 1.0, ovoof, (i * no + k0) * ov, ov, t2f, j * no * v2, 0, 1.0, s, n)
            # -(k|ji)
            product("N", nv, 1.0, t2f, (j * no + i) * v2, 0, ovvvf, k0 * v3, v3, 1.0, s, n)
            product("T", no, 1.0, ovoof, (j * no + i) * ov, 0, t2f, k0 * no * v2, no * v2, 1.0, s, n)
            s += n
        be.ccsd_triples_energy(no, nv, cubes, ijk[t0:t0 + nb].reshape(-1), t1s, fovs, t2s, oovvs, eo, ev, work,
                               energies[x:x + 1])
    e_t = 0.0
    for part in be.to_host(energies):
        e_t += float(part)
    if stats is not None:
        stats.update(triples_batch=batch, triples_plan=plan, triples_seconds=time.perf_counter() - t_start)
    return e_t


def solve_spatial(spatial, occupied, conv_tol: float = 1e-10, max_cycle: int = 200, diis_space: int = 6, backend=None,
                  stats: dict | None = None, triples: bool = False, triples_batch: int | None = None,
                  density: bool = False) -> CCSDResult:
    """CCSD of the determinant that occupies the spin orbitals ``occupied`` (index 2p + s, alpha even).

    ``spatial``: a ``SpatialHamiltonian``, or ``(constant, one_body (2,n,n), two_body (3,n,n,n,n))`` with the blocks of
    ``build_spatial()`` (thresholded, the two-body ones halved) as host or device arrays.  ``stats``, if given, receives
    the bytes planned and the seconds per cycle.  ``triples``: after the loop, the (T) energy of
    ``triples_from_blocks`` from the device-resident amplitudes and blocks, as ``e_t`` of the result; ``triples_batch``:
    its cubes in flight (default: what ``default_triples_batch`` fits into the free memory).  ``density``: after the
    loop (and before (T) frees what it does not read) the Lambda equations of ``lambda_from_blocks`` and the
    one-particle density: ``l1``, ``l2``, ``lambda_converged`` and ``rdm1()`` of the result.  With ``triples`` as well
    the density still is CCSD's: (T) contributes to the energy only."""
    be = _device_backend(backend)
    if hasattr(spatial, "two_body"):
        constant, one, two = spatial.constant, spatial.one_body, spatial.two_body
    else:
        constant, one, two = spatial
    n = int(one.shape[-1])
    nso = 2 * n
    occ = sorted(int(i) for i in occupied)
    if len(set(occ)) != len(occ) or (occ and (occ[0] < 0 or occ[-1] >= nso)):
        raise ValueError("occupied: distinct spin-orbital indices in [0, 2n) expected")
    vir = [p for p in range(nso) if p not in set(occ)]
    no, nv = len(occ), len(vir)
    if no == 0 or nv == 0:
        raise ValueError("CCSD needs at least one occupied and one virtual spin orbital")
    if not 1 <= diis_space <= 16:
        raise ValueError("diis_space must be between 1 and 16")
    plan = memory_plan(no, nv, diis_space, density=density)
    held = 8 * 3 * n**4 if be.torch.is_tensor(two) and two.is_cuda else 0  # (device blocks are there already)
    free = be.free_bytes()
    if plan["total"] - held > free:
        raise NbedDriverError(
            f"device CCSD of {nso} spin orbitals ({no} occupied, {nv} virtual) needs {plan['total'] - held} bytes of "
            f"device memory ({plan['blocks']} for the Hamiltonian blocks, {plan['amplitudes']} for amplitudes and DIIS "
            f"history, {plan['work']} of work space"
            + (f", {plan['lambda']} for the Lambda amplitudes and their intermediates" if density else "")
            + f"); {free} are free")
    if stats is not None:
        stats.update(plan=plan, nso=nso, nocc=no, nvir=nv)

    c = Contractor(be)
    tb = be.asarray(two)
    one_h = be.to_host(one)
    h1 = np.zeros((nso, nso))
    h1[0::2, 0::2], h1[1::2, 1::2] = one_h[0], one_h[1]
    idx = {"o": be.index_array(occ, nso), "v": be.index_array(vir, nso)}
    f = be.to_host(be.ccsd_fock(tb, be.asarray(h1), idx["o"]))
    e_hf = float(constant) + 0.5 * float(np.sum(np.diag(h1)[occ]) + np.sum(np.diag(f)[occ]))
    fov_h, foo_h, fvv_h = f[np.ix_(occ, vir)], f[np.ix_(occ, occ)], f[np.ix_(vir, vir)]
    eo_h, ev_h = np.diag(foo_h).copy(), np.diag(fvv_h).copy()
    fov, eo, ev = be.asarray(fov_h), be.asarray(eo_h), be.asarray(ev_h)
    foo_od, fvv_od = be.asarray(foo_h - np.diag(eo_h)), be.asarray(fvv_h - np.diag(ev_h))

    g = {name: be.ccsd_gather(tb, *(idx[ch] for ch in name)) for name in BLOCKS}
    vvvv_p = be.ccsd_gather(tb, idx["v"], idx["v"], idx["v"], idx["v"], pack_first=True, pack_last=True)
    del tb
    oovv, oooo, ovvo, ovov, ooov, ovvv, vvvo, ovoo = (g[name] for name in BLOCKS)

    n1, nvec = no * nv, no * nv + (no * nv) ** 2
    hist_t, hist_e = be.empty((diis_space, nvec)), be.empty((diis_space, nvec))
    amp, res = be.empty(nvec), be.empty(nvec)  # [t1 | t2] and the residual [r1 | r2]
    t1, t2 = amp[:n1].view(no, nv), amp[n1:].view(no, no, nv, nv)
    r1, r2 = res[:n1].view(no, nv), res[n1:].view(no, no, nv, nv)
    maxerr = be.empty(1)
    # MP2 start: t1 = 0, t2 = <ij||ab> / D  (the update kernel with r = [0 | oovv] and a scratch error vector)
    res[:n1].zero_()
    r2.copy_(oovv)
    be.ccsd_update(no, nv, res, res, eo, ev, amp, hist_e[0], maxerr)

    ident, swap_ab, swap_ij, swap_both = [0, 1, 2, 3], [0, 1, 3, 2], [1, 0, 2, 3], [1, 0, 3, 2]
    oovv_flat, fov_flat = oovv.view(1, -1), fov.view(1, -1)

    def energy(tau):
        return float(be.dots(t1.reshape(-1), fov_flat)[0] + 0.25 * be.dots(tau.view(-1), oovv_flat)[0])

    tau = be.ccsd_tau(t1, t2, 1.0, 1.0, 1.0)
    e_old = energy(tau)
    bmat = np.zeros((diis_space, diis_space))  # <err_s, err_t> by history slot
    age = []  # history slots, oldest first
    converged, it = False, 0
    cycle_seconds = []
    for it in range(1, max_cycle + 1):
        t_start = time.perf_counter()
        tau_t = be.ccsd_tau(t1, t2, 1.0, 0.5, 0.5)
        # intermediates (eqs. 3-8 of Stanton et al.), off-diagonal Fock terms kept
        fae = be.copy(fvv_od)
        c("me,ma->ae", fov, t1, -0.5, fae, 1.0)
        c("mf,mafe->ae", t1, ovvv, 1.0, fae, 1.0)
        c("mnaf,mnef->ae", tau_t, oovv, -0.5, fae, 1.0)
        fmi = be.copy(foo_od)
        c("ie,me->mi", t1, fov, 0.5, fmi, 1.0)
        c("ne,mnie->mi", t1, ooov, 1.0, fmi, 1.0)
        c("inef,mnef->mi", tau_t, oovv, 0.5, fmi, 1.0)
        del tau_t
        fme = be.copy(fov)
        c("nf,mnef->me", t1, oovv, 1.0, fme, 1.0)
        # W_mnij plus the 1/4 tau <oo||vv> piece of W_abef: 1/2 tau_ijef W_abef contains 1/2 tau_mnab (1/4 tau_ijef <mn||ef>)
        wmnij = be.copy(oooo)
        c("je,mnie->mnij", t1, ooov, 1.0, wmnij, 1.0)
        c("ie,mnje->mnij", t1, ooov, -1.0, wmnij, 1.0)
        c("ijef,mnef->mnij", tau, oovv, 0.5, wmnij, 1.0)
        wmbej = be.copy(ovvo)
        c("jf,mbef->mbej", t1, ovvv, 1.0, wmbej, 1.0)
        c("nb,mnje->mbej", t1, ooov, 1.0, wmbej, 1.0)
        half = be.ccsd_tau(t1, t2, 0.5, 1.0, 0.0)  # 1/2 t2_jnfb + t1_jf t1_nb
        c("jnfb,mnef->mbej", half, oovv, -1.0, wmbej, 1.0)
        del half
        # T1 (eq. 1)
        r1.copy_(fov)
        c("ie,ae->ia", t1, fae, 1.0, r1, 1.0)
        c("ma,mi->ia", t1, fmi, -1.0, r1, 1.0)
        c("imae,me->ia", t2, fme, 1.0, r1, 1.0)
        c("nf,naif->ia", t1, ovov, -1.0, r1, 1.0)
        c("imef,maef->ia", t2, ovvv, -0.5, r1, 1.0)
        c("mnae,nmie->ia", t2, ooov, 0.5, r1, 1.0)
        # T2 (eq. 2)
        r2.copy_(oovv)
        c("mb,me->be", t1, fme, -0.5, fae, 1.0)
        tmp = c("ijae,be->ijab", t2, fae)
        be.permute4(tmp, ident, 1.0, 1.0, r2)
        be.permute4(tmp, swap_ab, -1.0, 1.0, r2)
        c("je,me->mj", t1, fme, 0.5, fmi, 1.0)
        c("imab,mj->ijab", t2, fmi, 1.0, tmp, 0.0)
        be.permute4(tmp, ident, -1.0, 1.0, r2)
        be.permute4(tmp, swap_ij, 1.0, 1.0, r2)
        c("mnab,mnij->ijab", tau, wmnij, 0.5, r2, 1.0)
        # the ladder over packed pairs: sum_{e<f} tau_(ij)(ef) <ab||ef>_(ab)(ef)
        tau_p = be.ccsd_tau(t1, t2, 1.0, 1.0, 1.0, packed=True)
        npo, npv = _npair(no), _npair(nv)
        if npo and npv:
            lad = be.empty((npo, npv))
            be.gemm_raw("N", "T", npo, npv, npv, 1.0, tau_p, npv, 0, vvvv_p, npv, 0, 0.0, lad, npv, 0, 1)
            lad_ab = be.pair_unpack(lad, npo, nv, 1)               # (i<j, a, b)
            be.pair_unpack(lad_ab, 1, no, nv * nv, 1.0, 1.0, r2)   # r2 += (i, j, a, b)
            del lad, lad_ab
        del tau_p
        # the t1 <ov||vv> pieces of W_abef through Z_ijma = 1/2 sum_ef tau_ijef <ma||ef>
        z = c("ijef,maef->ijma", tau, ovvv, 0.5)
        c("ijma,mb->ijab", z, t1, 1.0, tmp, 0.0)
        del z
        be.permute4(tmp, ident, 1.0, 1.0, r2)
        be.permute4(tmp, swap_ab, -1.0, 1.0, r2)
        c("imae,mbej->ijab", t2, wmbej, 1.0, tmp, 0.0)
        y = c("ie,mbej->imbj", t1, ovvo)
        c("ma,imbj->ijab", t1, y, -1.0, tmp, 1.0)
        del y
        be.permute4(tmp, ident, 1.0, 1.0, r2)
        be.permute4(tmp, swap_ij, -1.0, 1.0, r2)
        be.permute4(tmp, swap_ab, -1.0, 1.0, r2)
        be.permute4(tmp, swap_both, 1.0, 1.0, r2)
        c("ie,abej->ijab", t1, vvvo, 1.0, tmp, 0.0)
        be.permute4(tmp, ident, 1.0, 1.0, r2)
        be.permute4(tmp, swap_ij, -1.0, 1.0, r2)
        c("ma,mbij->ijab", t1, ovoo, 1.0, tmp, 0.0)
        be.permute4(tmp, ident, -1.0, 1.0, r2)
        be.permute4(tmp, swap_ab, 1.0, 1.0, r2)
        del tmp, wmbej, wmnij, fae, fmi, fme
        # t_new = r / D and err = t_new - t into the next history slot; DIIS on the amplitudes
        slot = (it - 1) % diis_space
        be.ccsd_update(no, nv, res, amp, eo, ev, hist_t[slot], hist_e[slot], maxerr)
        if slot in age:
            age.remove(slot)
        age.append(slot)
        m = len(age)
        row = be.dots(hist_e[slot], hist_e[:m] if m < diis_space else hist_e)
        bmat[slot, : len(row)] = row
        bmat[: len(row), slot] = row
        err_max = float(be.read_scalars(maxerr)[0])
        coef = None
        if m > 1:
            b = -np.ones((m + 1, m + 1))
            b[m, m] = 0.0
            b[:m, :m] = bmat[np.ix_(age, age)]
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            try:
                sol = np.linalg.solve(b, rhs)[:m]
                coef = np.zeros(m)
                coef[age] = sol
            except np.linalg.LinAlgError:
                pass
        if coef is None:
            amp.copy_(hist_t[slot])
        else:
            be.lincomb(coef, hist_t[:m], out=amp)
        tau = be.ccsd_tau(t1, t2, 1.0, 1.0, 1.0)
        e_new = energy(tau)
        cycle_seconds.append(time.perf_counter() - t_start)
        done = abs(e_new - e_old) < conv_tol and err_max < max(conv_tol, 1e-9) * 10
        e_old = e_new
        if done:
            converged = True
            break
    if stats is not None:
        stats.update(cycle_seconds=cycle_seconds, iterations=it)
    t1_h, t2_h = be.to_host(t1).copy(), be.to_host(t2).copy()
    extra = {}
    if density:
        # the amplitude loop's residual and DIIS history are dead: the Lambda loop runs in them
        extra = lambda_from_blocks(be, occ, vir, amp, fov, foo_od, fvv_od, eo, ev, g, vvvv_p, tau, res, hist_t, hist_e,
                                   conv_tol=conv_tol, max_cycle=max_cycle, stats=stats)
    e_t = None
    if triples:
        # (T) from what is on the device now, after the loop's own memory is handed back: the DIIS history, the packed
        # <vv||vv>, the residual and the blocks (T) does not read
        del hist_t, hist_e, vvvv_p, res, r1, r2, tau, oooo, ovvo, ovov, ooov, vvvo, g
        be.torch.cuda.empty_cache()
        e_t = triples_from_blocks(t1, t2, fov, foo_h, fvv_h, oovv, ovvv, ovoo, [p & 1 for p in occ], [p & 1 for p in vir],
                                  batch=triples_batch, backend=be, stats=stats)
    return CCSDResult(e_hf, e_old, t1_h, t2_h, converged, it, e_t, **extra)


def lambda_from_blocks(be, occ, vir, amp, fov, foo_od, fvv_od, eo, ev, g, vvvv_p, tau, res, hist_l, hist_e,
                       conv_tol: float = 1e-10, max_cycle: int = 200, stats: dict | None = None) -> dict:
    """The CCSD Lambda amplitudes and the one-particle density on the device, from what the amplitude loop of
    ``solve_spatial`` leaves there: the converged ``amp`` = [t1 | t2], the Fock blocks (``foo_od``, ``fvv_od``: without
    their diagonals ``eo``, ``ev``), the Hamiltonian blocks ``g`` and the packed <vv||vv>, tau, and three buffers that
    are dead by now and are overwritten: the residual ``res`` and the DIIS history ``hist_l``, ``hist_e``.

    The equations are those of ``ccsd.lambda_intermediates`` / ``ccsd.lambda_residual``, term by term in their order,
    every product through ``Contractor``.  The intermediates do not depend on Lambda and are built once.  W_abef is
    never formed: 1/2 l_ijef <ef||ab> runs over packed pairs against ``vvvv_p`` (l2 packed by ``pair_pack``), the
    t1 <ov||vv> pieces of the ladder go through Y_ijem = l_ijef t_mf (o^3 v), the 1/4 tau <oo||vv> piece through
    l_ijef tau_mnef (o^4), and the t_if W_abef term of W_abei is the finished ladder times t1.  Start, update
    (``nbx_ccsd_update``: same vector layout, same denominators), DIIS and stopping rule are ``ccsd.solve_lambda``'s.

    Returns the keyword arguments ``CCSDResult`` takes: ``l1``, ``l2``, ``lambda_converged``, ``lambda_iterations``,
    ``dm1``."""
    from . import ccsd as host

    c = Contractor(be)
    no, nv = len(occ), len(vir)
    n1, nvec = no * nv, no * nv + (no * nv) ** 2
    diis_space = int(hist_l.shape[0])
    oovv, oooo, ovvo, ooov, ovvv, vvvo, ovoo = (g[k] for k in ("oovv", "oooo", "ovvo", "ooov", "ovvv", "vvvo", "ovoo"))
    t1, t2 = amp[:n1].view(no, nv), amp[n1:].view(no, no, nv, nv)
    r1, r2 = res[:n1].view(no, nv), res[n1:].view(no, no, nv, nv)
    ident, swap_ab, swap_ij, swap_both = [0, 1, 2, 3], [0, 1, 3, 2], [1, 0, 2, 3], [1, 0, 3, 2]
    t_setup = time.perf_counter()
    # ---- the elements of e^-T H e^T (ccsd.lambda_intermediates)
    tau_t = be.ccsd_tau(t1, t2, 1.0, 0.5, 0.5)
    fme = be.copy(fov)
    c("nf,mnef->me", t1, oovv, 1.0, fme, 1.0)
    fae = be.copy(fvv_od)
    c("me,ma->ae", fov, t1, -0.5, fae, 1.0)
    c("mf,mafe->ae", t1, ovvv, 1.0, fae, 1.0)
    c("mnaf,mnef->ae", tau_t, oovv, -0.5, fae, 1.0)
    c("ma,me->ae", t1, fme, -0.5, fae, 1.0)
    fmi = be.copy(foo_od)
    c("ie,me->mi", t1, fov, 0.5, fmi, 1.0)
    c("ne,mnie->mi", t1, ooov, 1.0, fmi, 1.0)
    c("inef,mnef->mi", tau_t, oovv, 0.5, fmi, 1.0)
    c("ie,me->mi", t1, fme, 0.5, fmi, 1.0)
    del tau_t
    wmnij = be.copy(oooo)
    c("je,mnie->mnij", t1, ooov, 1.0, wmnij, 1.0)
    c("ie,mnje->mnij", t1, ooov, -1.0, wmnij, 1.0)
    c("ijef,mnef->mnij", tau, oovv, 0.5, wmnij, 1.0)
    wmbej = be.copy(ovvo)
    c("jf,mbef->mbej", t1, ovvv, 1.0, wmbej, 1.0)
    c("nb,mnje->mbej", t1, ooov, 1.0, wmbej, 1.0)
    full = be.ccsd_tau(t1, t2, 1.0, 1.0, 0.0)  # t2_jnfb + t1_jf t1_nb
    c("jnfb,mnef->mbej", full, oovv, -1.0, wmbej, 1.0)
    del full
    wmnie = be.copy(ooov)
    c("if,mnfe->mnie", t1, oovv, 1.0, wmnie, 1.0)
    wmaef = be.copy(ovvv)
    c("na,mnef->maef", t1, oovv, -1.0, wmaef, 1.0)
    ring = be.copy(ovvo)  # <mb||ej> - t_njbf <mn||ef>
    c("njbf,mnef->mbej", t2, oovv, -1.0, ring, 1.0)
    wmbij = be.copy(ovoo)  # <mb||ij> = <ij||mb>
    c("me,ijbe->mbij", fme, t2, -1.0, wmbij, 1.0)
    c("nb,mnij->mbij", t1, wmnij, -1.0, wmbij, 1.0)
    c("mbef,ijef->mbij", ovvv, tau, 0.5, wmbij, 1.0)
    tmp = c("mnie,jnbe->mbij", ooov, t2)
    c("ie,mbej->mbij", t1, ring, 1.0, tmp, 1.0)
    be.permute4(tmp, ident, 1.0, 1.0, wmbij)
    be.permute4(tmp, swap_ab, -1.0, 1.0, wmbij)  # (the last two axes: i <-> j)
    wabei = be.copy(vvvo)
    c("me,miab->abei", fme, t2, -1.0, wabei, 1.0)
    c("mnie,mnab->abei", ooov, tau, -0.5, wabei, 1.0)
    tmp = c("mbef,miaf->abei", ovvv, t2)
    c("ma,mbei->abei", t1, ring, 1.0, tmp, 1.0)
    be.permute4(tmp, ident, -1.0, 1.0, wabei)
    be.permute4(tmp, swap_ij, 1.0, 1.0, wabei)  # (the first two axes: a <-> b)
    del tmp, ring
    be.read_scalars(fme.view(-1)[:1])  # (synchronises: the seconds below are the intermediates', not their launches')
    setup_seconds = time.perf_counter() - t_setup

    # ---- the loop (ccsd.solve_lambda): first-order left state, lambda_new = r / D, DIIS
    lam = be.empty(nvec)
    lam.copy_(amp)
    l1, l2 = lam[:n1].view(no, nv), lam[n1:].view(no, no, nv, nv)
    maxerr = be.empty(1)
    npo, npv = _npair(no), _npair(nv)
    lad = be.empty((no, no, nv, nv))
    bmat = np.zeros((diis_space, diis_space))
    age = []
    converged, it = False, 0
    cycle_seconds = []
    for it in range(1, max_cycle + 1):
        t_start = time.perf_counter()
        gae = c("mnef,mnaf->ae", t2, l2, -0.5)
        gmi = c("mnef,inef->mi", t2, l2, 0.5)
        # the ladder L_ijab = 1/2 l_ijef W_efab: packed pairs against <vv||vv>, then the two pieces of W_abef - <vv||vv>
        if npo and npv:
            l2_p = be.pair_pack(be.pair_pack(l2, no * no, nv, 1), 1, no, npv)  # (i<j, e<f)
            lad_p = be.empty((npo, npv))
            be.gemm_raw("N", "N", npo, npv, npv, 1.0, l2_p, npv, 0, vvvv_p, npv, 0, 0.0, lad_p, npv, 0, 1)
            lad_ab = be.pair_unpack(lad_p, npo, nv, 1)                 # (i<j, a, b)
            be.pair_unpack(lad_ab, 1, no, nv * nv, 1.0, 0.0, lad)      # (i, j, a, b)
            del l2_p, lad_p, lad_ab
        else:
            lad.zero_()
        y = c("ijef,mf->ijem", l2, t1)
        c("ijem,meab->ijab", y, ovvv, 1.0, lad, 1.0)
        x = c("ijef,mnef->ijmn", l2, tau)
        c("ijmn,mnab->ijab", x, oovv, 0.25, lad, 1.0)
        del y, x
        # Lambda_1
        r1.copy_(fme)
        c("ie,ea->ia", l1, fae, 1.0, r1, 1.0)
        c("ma,im->ia", l1, fmi, -1.0, r1, 1.0)
        c("me,ieam->ia", l1, wmbej, 1.0, r1, 1.0)
        c("imef,efam->ia", l2, wabei, 0.5, r1, 1.0)
        c("imae,me->ia", lad, t1, 1.0, r1, 1.0)
        c("mnae,iemn->ia", l2, wmbij, -0.5, r1, 1.0)
        c("ef,iefa->ia", gae, wmaef, 1.0, r1, 1.0)
        c("mn,mina->ia", gmi, wmnie, -1.0, r1, 1.0)
        # Lambda_2
        r2.copy_(oovv)
        be.permute4(lad, ident, 1.0, 1.0, r2)
        c("mnab,ijmn->ijab", l2, wmnij, 0.5, r2, 1.0)
        tmp = c("ijae,eb->ijab", l2, fae)
        c("ijae,be->ijab", oovv, gae, 1.0, tmp, 1.0)
        c("ma,ijmb->ijab", l1, wmnie, -1.0, tmp, 1.0)
        be.permute4(tmp, ident, 1.0, 1.0, r2)
        be.permute4(tmp, swap_ab, -1.0, 1.0, r2)
        c("imab,jm->ijab", l2, fmi, 1.0, tmp, 0.0)
        c("imab,mj->ijab", oovv, gmi, 1.0, tmp, 1.0)
        c("ie,jeab->ijab", l1, wmaef, 1.0, tmp, 1.0)
        be.permute4(tmp, ident, -1.0, 1.0, r2)
        be.permute4(tmp, swap_ij, 1.0, 1.0, r2)
        c("imae,jebm->ijab", l2, wmbej, 1.0, tmp, 0.0)
        be.permute4(tmp, ident, 1.0, 1.0, r2)
        be.permute4(tmp, swap_ij, -1.0, 1.0, r2)
        be.permute4(tmp, swap_ab, -1.0, 1.0, r2)
        be.permute4(tmp, swap_both, 1.0, 1.0, r2)
        be.ccsd_lambda_outer(l1, fme, r2)  # P(ij) P(ab) l_ia F_jb
        del tmp, gae, gmi
        slot = (it - 1) % diis_space
        be.ccsd_update(no, nv, res, lam, eo, ev, hist_l[slot], hist_e[slot], maxerr)
        if slot in age:
            age.remove(slot)
        age.append(slot)
        m = len(age)
        row = be.dots(hist_e[slot], hist_e[:m] if m < diis_space else hist_e)
        bmat[slot, : len(row)] = row
        bmat[: len(row), slot] = row
        err_max = float(be.read_scalars(maxerr)[0])
        coef = None
        if m > 1:
            b = -np.ones((m + 1, m + 1))
            b[m, m] = 0.0
            b[:m, :m] = bmat[np.ix_(age, age)]
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            try:
                sol = np.linalg.solve(b, rhs)[:m]
                coef = np.zeros(m)
                coef[age] = sol
            except np.linalg.LinAlgError:
                pass
        if coef is None:
            lam.copy_(hist_l[slot])
        else:
            be.lincomb(coef, hist_l[:m], out=lam)
        cycle_seconds.append(time.perf_counter() - t_start)
        if err_max < max(conv_tol, 1e-9) * 10:
            converged = True
            break
    # ---- the density (ccsd.density_blocks), assembled and checked by nbx_ccsd_rdm1
    xmi = c("mnef,inef->mi", l2, t2, 0.5)
    yae = c("mnef,mnaf->ae", l2, t2, 0.5)
    c("me,ma->ae", l1, t1, 1.0, yae, 1.0)
    goo = c("ie,je->ij", l1, t1, -1.0)
    c("imef,jmef->ij", l2, t2, -0.5, goo, 1.0)
    gvv = c("ma,mb->ab", l1, t1)
    c("mnae,mnbe->ab", l2, t2, 0.5, gvv, 1.0)
    gvo = be.permute4(t1, [1, 0])
    c("imae,me->ai", t2, l1, 1.0, gvo, 1.0)
    c("mi,ma->ai", xmi, t1, -1.0, gvo, 1.0)
    c("ie,ae->ai", t1, yae, -1.0, gvo, 1.0)
    dm1, cross = be.ccsd_rdm1(occ, vir, goo, l1, gvo, gvv)
    cross_h = float(be.read_scalars(cross)[0])
    host.check_cross_spin(cross_h)
    if stats is not None:
        stats.update(lambda_cycle_seconds=cycle_seconds, lambda_iterations=it, lambda_setup_seconds=setup_seconds,
                     lambda_cross_spin=cross_h)
    return dict(l1=be.to_host(l1).copy(), l2=be.to_host(l2).copy(), lambda_converged=converged, lambda_iterations=it,
                dm1=np.array(be.to_host(dm1), dtype=float))
